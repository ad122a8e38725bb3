// Lane maps of v_mfma_i32_16x16x64_i8 on gfx950, checked with exact, asymmetric integer data (the forward transforms' matrix-
// pipe body, kernels.hip ntt_forward_quarter3<true>, relies on them):
//   A  lane l holds row l & 15,    K slots 16 (l >> 4) + b in byte b = 0..15 of its four registers
//   B  lane l holds column l & 15, the SAME K slots
//   D  lane l holds column l & 15, rows 4 (l >> 4) + register
// Only "A and B enumerate K in the same (lane >> 4, byte) order" matters to the kernel: it is free to call that order k.
// The probe fills A and B with distinct non-symmetric values under this hypothesis, compares all 256 outputs with a host
// product, and then reports, for one-hot A entries, which B entry each one multiplies -- the map itself, if the hypothesis fails.
//     build: hipcc --offload-arch=gfx950 -O2 -o mfma_i8_map_probe mfma_i8_map_probe.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

typedef int v4i __attribute__((ext_vector_type(4)));

__global__ void k_mfma(const v4i* a, const v4i* b, const v4i* c, v4i* d) {
    const unsigned l = threadIdx.x;
    d[l] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[l], b[l], c[l], 0, 0, 0);
}

static void run(const std::vector<int8_t>& A, const std::vector<int8_t>& B, const std::vector<int>& C, std::vector<int>& D, void* dev) {
    char* p = (char*)dev;
    hipMemcpy(p, A.data(), 1024, hipMemcpyHostToDevice);
    hipMemcpy(p + 1024, B.data(), 1024, hipMemcpyHostToDevice);
    hipMemcpy(p + 2048, C.data(), 1024, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_mfma, dim3(1), dim3(64), 0, 0, (const v4i*)p, (const v4i*)(p + 1024), (const v4i*)(p + 2048), (v4i*)(p + 3072));
    hipMemcpy(D.data(), p + 3072, 1024, hipMemcpyDeviceToHost);
}

int main() {
    void* dev;
    if (hipMalloc(&dev, 4096) != hipSuccess) { printf("no device\n"); return 2; }
    std::vector<int8_t> A(1024), B(1024);
    std::vector<int> C(256), D(256);
    // logical matrices: a[row][k], b[k][col], c[row][col]; lane images under the hypothesis
    auto a_of = [](int row, int k) { return (int)((row * 37 + k * 11 + 5) % 127); };
    auto b_of = [](int k, int col) { return (int)((k * 29 + col * 53 + 3) % 127) - (k & 1 ? 100 : 0); };   // signed values too
    auto c_of = [](int row, int col) { return row * 1000 - col * 77; };
    for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 16; ++e) {
            A[l * 16 + e] = (int8_t)a_of(l & 15, 16 * (l >> 4) + e);
            B[l * 16 + e] = (int8_t)b_of(16 * (l >> 4) + e, l & 15);
        }
    for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r) C[l * 4 + r] = c_of(4 * (l >> 4) + r, l & 15);
    run(A, B, C, D, dev);
    int bad = 0;
    for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * (l >> 4) + r, col = l & 15;
            long long ref = c_of(row, col);
            for (int k = 0; k < 64; ++k) ref += (long long)(int8_t)a_of(row, k) * (int8_t)b_of(k, col);
            if (ref != D[l * 4 + r]) ++bad;
        }
    printf("hypothesis (A row = lane & 15, B column = lane & 15, K slot = 16 (lane >> 4) + byte for both, D row = 4 (lane >> 4) + reg): %d of 256 outputs differ -> %s\n",
           bad, bad ? "FAIL" : "PASS");
    // the map itself: A one-hot at (lane la, byte ea); B[lane][byte] = lane >> 4 (run 1) / byte (run 2) / lane & 15 (run 3)
    int shown = 0, odd = 0;
    for (int la = 0; la < 64; ++la)
        for (int ea = 0; ea < 16; ++ea) {
            std::vector<int8_t> A1(1024, 0);
            A1[la * 16 + ea] = 1;
            std::vector<int> Z(256, 0), D1(256), D2(256);
            std::vector<int8_t> B1(1024), B2(1024);
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 16; ++e) { B1[l * 16 + e] = (int8_t)(1 + (l >> 4)); B2[l * 16 + e] = (int8_t)(1 + e); }
            run(A1, B1, Z, D1, dev);
            run(A1, B2, Z, D2, dev);
            // every non-zero output sits in the row this A entry belongs to; its value names the B group / byte
            int row = -1, grp = -1, byte = -1, rows = 0;
            for (int l = 0; l < 64; ++l)
                for (int r = 0; r < 4; ++r)
                    if (D1[l * 4 + r]) { const int rw = 4 * (l >> 4) + r; if (rw != row) { row = rw; ++rows; } grp = D1[l * 4 + r] - 1; byte = D2[l * 4 + r] - 1; }
            const bool expect = rows == 1 && row == (la & 15) && grp == (la >> 4) && byte == ea;
            if (!expect) { ++odd; if (shown++ < 16) printf("  A(lane %2d, byte %2d): row %d (x%d), pairs with B(group %d, byte %d)\n", la, ea, row, rows, grp, byte); }
        }
    printf("one-hot scan: %d of 1024 A entries off the hypothesis\n", odd);
    hipFree(dev);
    return (bad || odd) ? 1 : 0;
}
