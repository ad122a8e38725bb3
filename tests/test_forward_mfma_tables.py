"""Host-built tables of the matrix-pipe forward body (csrc/fwd_mfma.hpp, bce_forward_mfma_tables: no context, no GPU)
against a plain numpy model written here.

The model applies the six radix-2 Cooley-Tukey stages on position bits 9..4 (merged order, tw[m + i] = psi^brv(m + i)) to the
balanced digits d - 2^(gBits-1) of random digit rows and checks that the result equals the four limb products recombined
mod Q, in both forms:  ((S2 + S3 2^7) 2^14 + S0 + S1 2^7 + C[h']) mod Q  with  S_i = limb_i(M6) X  on the raw digits, and
the same without C on the signed digits (what the kernel runs).  All in plain integers.
Bounds are the ones of the number formats: a limb sum is at most 64 * 127 * 127 (64 terms of two 7-bit factors), which the
i32 accumulator holds exactly; low and high parts must fit 32 bits.
"""
import numpy as np

Q128 = 134215681      # STD128 / STD128_OPT ring modulus (27 bits), N = 1024, gadget base 2^7, four digits
N = 1024


def _brv(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2)


def _six_stages(rows, psi, Q):
    """rows: int64 [..., 1024] residues; the stages on bits 9..4 in place order (output at the butterfly's own positions)."""
    x = np.array(rows, dtype=object) % Q
    tw = [pow(psi, _brv(i, 10), Q) for i in range(64)]
    for B in range(9, 3, -1):
        m = 1 << (9 - B)
        for p in range(N):
            if p & (1 << B):
                continue
            w = tw[m + (p >> (B + 1))]
            X, T = x[..., p], (x[..., p | (1 << B)] * w) % Q
            x[..., p], x[..., p | (1 << B)] = (X + T) % Q, (X - T) % Q
    return x


def _tables(bce, Q=Q128, gBits=7, dG=4, n=N):
    return bce.forward_mfma_tables(Q, n, gBits, dG)


def test_matrix_limbs_and_balance_words_reproduce_the_six_stages(bce):
    st, T = _tables(bce)
    assert st == 1
    Q, psi, M6, C = Q128, T["psi"], T["M6"].astype(object), T["C"].astype(object)
    assert pow(psi, N, Q) == Q - 1                                   # a primitive 2N-th root
    assert int(T["M6"].max()) < Q and int(T["C"].max()) < Q
    rng = np.random.default_rng(2026)
    digits = rng.integers(0, 128, size=(4, N))                       # raw gadget digits of four rows
    digits[0, :64] = 127                                             # and the extremes
    digits[1, :64] = 0
    ref = _six_stages(digits.astype(object) - 64, psi, Q)            # the transform's input is the balanced digit
    X = digits.reshape(4, 64, 16).astype(object)                     # [row][h = p >> 4][j = p & 15]
    limbs = [(M6 >> (7 * i)) & 127 for i in range(4)]
    assert sum(l << (7 * i) for i, l in enumerate(limbs)).tolist() == M6.tolist() and max(int(l.max()) for l in limbs) <= 127
    S = [np.einsum("ab,rbj->raj", l, X) for l in limbs]              # plain integers
    biggest = max(int(s.max()) for s in S)
    print("largest limb sum %d (bound %d)" % (biggest, 64 * 127 * 127))
    assert biggest <= 64 * 127 * 127 < 2 ** 31
    lo = S[0] + (S[1] << 7) + C[None, :, None]
    hi = S[2] + (S[3] << 7)
    assert 0 <= int(lo.min()) and int(lo.max()) < 2 ** 32 and 0 <= int(hi.min()) and int(hi.max()) < 2 ** 32
    got = ((hi << 14) + lo) % Q
    assert got.reshape(4, N).tolist() == ref.tolist()                # all 4 x 1024 words, raw digits + balance words
    # the form the kernel runs: signed digits as the i8 operand, accumulators starting at (Q, 0, Q, 0)
    Xs = X - 64
    assert int(Xs.min()) == -64 and int(Xs.max()) == 63
    Ss = [np.einsum("ab,rbj->raj", l, Xs) for l in limbs]
    L = 64 * 127 * 64
    assert max(abs(int(s.min())) for s in Ss) <= L and max(int(s.max()) for s in Ss) <= L <= 64 * 127 * 127
    assert T["limb_sum_max"] == L and 129 * L < Q
    lo, hi = Q + Ss[0] + (Ss[1] << 7), Q + Ss[2] + (Ss[3] << 7)
    assert 0 < int(lo.min()) and int(lo.max()) <= T["lo_max"] == Q + 129 * L < 2 ** 32
    assert 0 < int(hi.min()) and int(hi.max()) <= T["hi_max"] == Q + 129 * L
    assert (((hi << 14) + lo) % Q).reshape(4, N).tolist() == ref.tolist()
    # the kernel's recombination: lazy Shoup product by 2^14 with the low part as its addend, in 32-bit arithmetic
    w, ws = T["w14"]
    assert w == (1 << 14) % Q and ws == (w << 32) // Q
    word = (hi * w - ((hi * ws) >> 32) * Q + lo)
    assert int(word.min()) >= 0 and int(word.max()) < T["out_max"] == 2 * Q + T["lo_max"] <= 13 * Q and T["out_max"] < 2 ** 32
    assert (word % Q).reshape(4, N).tolist() == ref.tolist()


def test_device_image_holds_the_limbs_in_operand_order(bce):
    """[quarter][tile][lane][16 bytes]: the A operand of tile i (row l & 15 = (o, limb), K slots 16 (l >> 4) + b with
    position h = (k >> 2) + 16 (k & 3)); the balance words of the raw-digit form are -64 times M6's row sums."""
    st, T = _tables(bce)
    assert st == 1
    M6, C, tab = T["M6"], T["C"], T["table"]
    img = tab.view(np.uint8).reshape(4, 4, 64, 16)
    assert C.tolist() == [(-64 * int(M6[h].astype(object).sum())) % Q128 for h in range(64)]
    for q in range(4):
        for l in range(64):
            o, limb, g = (l & 15) >> 2, l & 3, l >> 4
            for i in range(4):
                hp = 16 * q + 4 * i + o
                ks = 16 * g + np.arange(16)
                want = (M6[hp, (ks >> 2) + 16 * (ks & 3)] >> (7 * limb)) & 127
                assert np.array_equal(img[q, i, l], want.astype(np.uint8))


def test_enable_predicate(bce):
    assert _tables(bce)[0] == 1
    assert _tables(bce, gBits=6)[0] == 1                              # smaller digits: tighter sums
    assert _tables(bce, gBits=8) == (0, None)                         # digits would not fit a non-negative i8
    assert _tables(bce, dG=3) == (0, None)
    assert _tables(bce, n=512) == (0, None) and _tables(bce, n=2048) == (0, None)
    assert _tables(bce, Q=Q128 + 2) == (0, None)                      # not 1 mod 2N
    # a modulus above 2^28 would need a fifth limb
    assert _tables(bce, Q=(1 << 28) + 2048 * 3 + 1)[0] == 0
    # a small prime of the class (24 bits, 1 mod 2N): tables are built, but 129 L >= Q (low and high part could be negative)
    # refuses the body
    q = (1 << 23) + 1
    while any(q % p == 0 for p in range(3, 4096, 2)):
        q += 2048
    st, T = _tables(bce, Q=q)
    assert 129 * T["limb_sum_max"] >= q and st == -1
