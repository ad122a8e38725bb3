// devmem_selftest.cpp -- csrc/devmem.hpp alone, on the host: the ten HIP entry points the header calls are defined HERE, on
// top of malloc, with a set of live allocations, a log of the calls and a switch that makes the k-th call fail.  Built by the
// host compiler (sanitizers where it has them) without the HIP runtime; see tests/test_devmem_standalone.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../../openfhe-boolean-circuit-evaluator_amd/csrc/devmem.hpp"

using bce::DevBuf;
using bce::StagedUpload;

namespace {

enum Fn { MALLOC, HOSTMALLOC, FREE, HOSTFREE, EVCREATE, EVDESTROY, EVRECORD, EVSYNC, MEMCPY, STREAMSYNC };

std::map<void*, size_t> g_dev, g_host;   // live allocations and their sizes
std::set<void*> g_events;
std::vector<Fn> g_log;                   // every call since the last clear, in order
std::vector<hipStream_t> g_synced;       // streams handed to hipStreamSynchronize
size_t g_calls = 0, g_fail_at = 0;       // calls so far; the call with this number (1-based) fails, 0 = none
int g_failed = -1;                       // the Fn that was made to fail
size_t g_last_size = 0;                  // bytes of the last allocation

size_t live() { return g_dev.size() + g_host.size() + g_events.size(); }

void die(const char* what, int line) {
    std::fprintf(stderr, "devmem selftest: line %d: %s\n", line, what);
    std::exit(1);
}
#define CHECK(cond) do { if (!(cond)) die(#cond, __LINE__); } while (0)

// counts the call; true when it is the one that has to fail
bool enter(Fn f) {
    g_log.push_back(f);
    if (++g_calls != g_fail_at) return false;
    g_failed = f;
    return true;
}
void clear_log() { g_log.clear(); g_synced.clear(); }
bool log_is(std::initializer_list<Fn> want) { return g_log == std::vector<Fn>(want); }

hipError_t allocate(Fn f, std::map<void*, size_t>& where, void** ptr, size_t size) {
    if (enter(f)) return hipErrorOutOfMemory;
    *ptr = std::malloc(size ? size : 1);
    where[*ptr] = size;
    g_last_size = size;
    return hipSuccess;
}
// a release happens even when its call is the one that reports failure: the owners cannot do anything about it
hipError_t release(Fn f, std::map<void*, size_t>& where, void* ptr) {
    const bool fail = enter(f);
    if (!where.erase(ptr)) die("freed what was not allocated this way", __LINE__);
    std::free(ptr);
    return fail ? hipErrorInvalidValue : hipSuccess;
}
bool inside(const std::map<void*, size_t>& where, const void* p, size_t bytes) {
    for (const auto& a : where)
        if (p == a.first) return bytes <= a.second;
    return false;
}

}  // namespace

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) { return allocate(MALLOC, g_dev, ptr, size); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) { return allocate(HOSTMALLOC, g_host, ptr, size); }
hipError_t hipFree(void* ptr) { return release(FREE, g_dev, ptr); }
hipError_t hipHostFree(void* ptr) { return release(HOSTFREE, g_host, ptr); }
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned flags) {
    if (enter(EVCREATE)) return hipErrorOutOfMemory;
    CHECK(flags == hipEventDisableTiming);
    *event = static_cast<hipEvent_t>(std::malloc(1));
    g_events.insert(*event);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) {
    const bool fail = enter(EVDESTROY);
    CHECK(g_events.erase(event) == 1);
    std::free(event);
    return fail ? hipErrorInvalidValue : hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t) {
    if (enter(EVRECORD)) return hipErrorInvalidValue;
    CHECK(g_events.count(event) == 1);
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t event) {
    if (enter(EVSYNC)) return hipErrorInvalidValue;
    CHECK(g_events.count(event) == 1);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    if (enter(MEMCPY)) return hipErrorInvalidValue;
    CHECK(kind == hipMemcpyHostToDevice && inside(g_dev, dst, bytes) && inside(g_host, src, bytes));
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
    g_synced.push_back(stream);
    return enter(STREAMSYNC) ? hipErrorInvalidValue : hipSuccess;
}
}  // extern "C"

namespace {

int g_dummy_stream, g_dummy_sync;
const hipStream_t S = reinterpret_cast<hipStream_t>(&g_dummy_stream);      // the stream of the uploads
const hipStream_t SYNC = reinterpret_cast<hipStream_t>(&g_dummy_sync);    // the stream a growth waits for

void fill(void* p, size_t bytes, unsigned seed) {
    for (size_t i = 0; i < bytes; ++i) static_cast<unsigned char*>(p)[i] = (unsigned char)(seed + 31 * i);
}
bool holds(const void* p, size_t bytes, unsigned seed) {
    for (size_t i = 0; i < bytes; ++i)
        if (static_cast<const unsigned char*>(p)[i] != (unsigned char)(seed + 31 * i)) return false;
    return true;
}

void test_devbuf() {
    {
        DevBuf<int> b;
        CHECK(!b.get() && b.capacity() == 0);
        clear_log();
        CHECK(b.alloc(10) == hipSuccess && log_is({MALLOC}) && g_last_size == 10 * sizeof(int));
        CHECK(b.get() && b.capacity() == 10 && live() == 1);
        int* const first = b.get();
        clear_log();
        CHECK(b.grow(10, 99, SYNC) == hipSuccess && b.grow(0, 99, nullptr) == hipSuccess && log_is({}));   // large enough: no call
        CHECK(b.get() == first && b.capacity() == 10);
        CHECK(b.grow(11, 32, SYNC) == hipSuccess && log_is({STREAMSYNC, FREE, MALLOC}));   // the one wait comes before the free
        CHECK(g_synced.size() == 1 && g_synced[0] == SYNC && g_last_size == 32 * sizeof(int) && b.capacity() == 32 && live() == 1);
        clear_log();
        CHECK(b.grow(40, 40, nullptr) == hipSuccess && log_is({FREE, MALLOC}) && b.capacity() == 40);    // no stream: no wait
        DevBuf<int> c(std::move(b));
        CHECK(!b.get() && b.capacity() == 0 && c.capacity() == 40 && live() == 1);
        DevBuf<int> d;
        CHECK(d.alloc(3) == hipSuccess && live() == 2);
        d = std::move(c);   // what d held is released with c, at the latest
        CHECK(d.capacity() == 40);
        clear_log();
        d.reset();
        CHECK(log_is({FREE}) && !d.get() && d.capacity() == 0);
        d.reset();
        CHECK(log_is({FREE}));   // empty: no call
        DevBuf<double, true> h;
        clear_log();
        CHECK(h.alloc(7) == hipSuccess && log_is({HOSTMALLOC}) && g_last_size == 7 * sizeof(double) && g_host.size() == 1);
        CHECK(h.grow(8, 16, nullptr) == hipSuccess && log_is({HOSTMALLOC, HOSTFREE, HOSTMALLOC}) && h.capacity() == 16);
    }
    CHECK(live() == 0);
    // every call of a growth fails once: the buffer is empty afterwards, and grows again
    for (size_t k = 1; k <= 3; ++k) {
        {
            DevBuf<int> b;
            CHECK(b.alloc(4) == hipSuccess);
            g_calls = 0; g_fail_at = k; g_failed = -1;
            const hipError_t e = b.grow(5, 8, SYNC);
            g_fail_at = 0;
            CHECK(g_failed >= 0);
            if (g_failed == FREE) CHECK(e == hipSuccess && b.capacity() == 8);   // a failed free is not the buffer's failure
            else CHECK(e != hipSuccess && !b.get() && b.capacity() == 0);
            CHECK(b.grow(5, 8, SYNC) == hipSuccess && b.get() && b.capacity() == 8);
        }
        CHECK(live() == 0);
    }
}

void test_staged_upload() {
    {
        StagedUpload u;
        CHECK(!u.host() && !u.device() && u.capacity() == 0);
        clear_log();
        CHECK(u.reserve(100, 256, SYNC) == hipSuccess && log_is({STREAMSYNC, MALLOC, HOSTMALLOC, EVCREATE}));
        CHECK(u.capacity() == 256 && g_dev.begin()->second == 256 && g_host.begin()->second == 256 && live() == 3);
        const void* const dev = u.device();
        clear_log();
        CHECK(u.reserve(256, 999, SYNC) == hipSuccess && u.reserve(1, 1, SYNC) == hipSuccess && log_is({}));   // large enough, not busy: no call
        CHECK(u.device() == dev && u.capacity() == 256);
        fill(u.host(), 100, 1);
        CHECK(u.send(100, S) == hipSuccess && log_is({MEMCPY, EVRECORD}) && holds(u.device(), 100, 1));
        clear_log();
        CHECK(u.reserve(100, 256, SYNC) == hipSuccess && log_is({EVSYNC}));    // busy: one wait for the event ...
        CHECK(u.reserve(100, 256, SYNC) == hipSuccess && log_is({EVSYNC}));    // ... and none the second time
        fill(u.host(), 50, 2);
        clear_log();
        CHECK(u.copy(50, S) == hipSuccess && log_is({MEMCPY}) && holds(u.device(), 50, 2));
        CHECK(u.mark(S) == hipSuccess && log_is({MEMCPY, EVRECORD}));
        clear_log();
        // busy and too small: the event, then ONE wait for the stream before the first free, then the pair
        CHECK(u.reserve(300, 512, SYNC) == hipSuccess && log_is({EVSYNC, STREAMSYNC, FREE, MALLOC, HOSTFREE, HOSTMALLOC}));
        CHECK(g_synced.size() == 1 && g_synced[0] == SYNC && u.capacity() == 512 && g_dev.begin()->second == 512 && g_host.begin()->second == 512);
        fill(u.host(), 300, 3);
        CHECK(u.send(300, S) == hipSuccess && holds(u.device(), 300, 3));
        StagedUpload v(std::move(u));   // buffers, event and the busy flag move
        CHECK(!u.host() && !u.device() && u.capacity() == 0 && v.capacity() == 512 && live() == 3);
        clear_log();
        CHECK(v.reserve(1, 1, nullptr) == hipSuccess && log_is({EVSYNC}));
        CHECK(u.reserve(8, 8, nullptr) == hipSuccess && live() == 6);   // the moved-from object starts again from nothing
        u = std::move(v);
        CHECK(u.capacity() == 512);
        clear_log();
        u.reset();
        CHECK(log_is({FREE, HOSTFREE, EVDESTROY}) && u.capacity() == 0);
    }
    CHECK(live() == 0);
}

// One scripted life of a StagedUpload: grows twice, sends, marks, moves.  Any one call may fail (g_fail_at): a failed
// reserve leaves the object empty (or, when only the wait for its event failed, as it was), and the next reserve works.
void reserve_checked(StagedUpload& u, size_t bytes, size_t cap, hipStream_t sync) {
    const size_t before = u.capacity();
    const void* const dev = u.device();
    g_failed = -1;
    const hipError_t e = u.reserve(bytes, cap, sync);
    if (e != hipSuccess) {
        CHECK(g_failed >= 0);
        if (g_failed == EVSYNC) CHECK(u.capacity() == before && u.device() == dev);
        else CHECK(u.capacity() == 0 && !u.device() && !u.host());
        CHECK(u.reserve(bytes, cap, sync) == hipSuccess);   // the switch fails one call only
    }
    CHECK(u.capacity() >= bytes && u.device() && u.host());
    if (before < bytes) CHECK(u.capacity() == cap);
}
void scripted_life() {
    StagedUpload u;
    reserve_checked(u, 64, 128, SYNC);
    fill(u.host(), 64, 4);
    if (u.send(64, S) == hipSuccess) CHECK(holds(u.device(), 64, 4));
    reserve_checked(u, 1000, 1024, SYNC);
    fill(u.host(), 1000, 5);
    if (u.copy(1000, S) == hipSuccess) CHECK(holds(u.device(), 1000, 5));
    (void)u.mark(S);
    StagedUpload v(std::move(u));
    reserve_checked(v, 10, 10, SYNC);
    StagedUpload w;
    reserve_checked(w, 16, 16, nullptr);
    w = std::move(v);
    reserve_checked(w, 5000, 8192, nullptr);
    fill(w.host(), 5000, 6);
    if (w.send(5000, S) == hipSuccess) CHECK(holds(w.device(), 5000, 6));
}
void test_fault_injection() {
    g_calls = 0; g_fail_at = 0;
    scripted_life();
    const size_t total = g_calls;
    CHECK(live() == 0 && total >= 20);
    for (size_t k = 1; k <= total; ++k) {
        g_calls = 0; g_fail_at = k; g_failed = -1;
        scripted_life();
        CHECK(g_calls >= k);   // the k-th call happened, and failed
        CHECK(live() == 0);
    }
    g_fail_at = 0;
}

}  // namespace

int main() {
    test_devbuf();
    test_staged_upload();
    test_fault_injection();
    std::printf("devmem selftest ok\n");
    return 0;
}
