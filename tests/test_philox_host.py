"""CPU tests of the host restatement of the device generator (tests/philox_ref.py).

  * Philox4x32-10: the three Random123 known answers, asserted literally, and
    equality with a scalar Python-integer restatement on random counters/keys;
  * normal2 against mpmath at 50 digits: rtol 1e-12 (the suite's float64 bar,
    test_bp_gpu.py::test_lxor_lxfb_on_device), the largest error printed in
    ulps, plus the edges of u1 and the quadrant points of u2, where the zeros
    must be exact;
  * layout: a row does not depend on the batch size, the bit and noise domains
    differ, awgn and bpsk_llr draw the same normals.
"""
import mpmath
import numpy as np

import philox_ref as pr

SEED, STREAM = 0xFEDCBA9876543210, (7 << 32) | 5


def _philox_int(c, k, rounds=10):
    """Philox4x32 on Python integers, one counter at a time."""
    c, k = list(c), list(k)
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


KNOWN_ANSWERS = [  # Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF),
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for c, k, want in KNOWN_ANSWERS:
        got = pr.philox4x32_10(*c, *k)
        assert all(g.dtype == np.uint32 for g in got)
        assert tuple(int(g) for g in got) == want
        assert tuple(_philox_int(c, k)) == want
    # all three in one vectorised call
    cs = np.array([c for c, _, _ in KNOWN_ANSWERS], dtype=np.uint64).T
    ks = np.array([k for _, k, _ in KNOWN_ANSWERS], dtype=np.uint64).T
    got = np.stack(pr.philox4x32_10(*cs, *ks), axis=1)
    assert np.array_equal(got, np.array([w for _, _, w in KNOWN_ANSWERS], dtype=np.uint32))


def test_philox_vectorised_equals_scalar():
    rng = np.random.default_rng(11)
    n = 3000
    w = rng.integers(0, 1 << 32, (6, n), dtype=np.uint64)
    w[:, :6] = np.eye(6, dtype=np.uint64) * np.uint64(0xFFFFFFFF)  # one saturated word at a time
    got = np.stack(pr.philox4x32_10(*w), axis=1)
    for i in range(n):
        v = [int(x) for x in w[:, i]]
        assert [int(x) for x in got[i]] == _philox_int(v[:4], v[4:]), i
    # broadcasting a scalar key, as the kernels' restatements do
    one = pr.philox4x32_10(w[0], w[1], 3, 4, 5, 6)
    assert [int(x[7]) for x in one] == _philox_int([int(w[0, 7]), int(w[1, 7]), 3, 4], [5, 6])


def _c_from_k(k1, k2):
    """Philox words whose 53-bit integers are (k1, k2); the 11 low bits of
    words 1 and 3, which the normals ignore, are set."""
    k1, k2 = np.asarray(k1, dtype=np.uint64), np.asarray(k2, dtype=np.uint64)
    lo, sh21, sh11 = np.uint64(0x1FFFFF), np.uint64(21), np.uint64(11)
    fill = np.uint64(0x7FF)
    return k1 >> sh21, ((k1 & lo) << sh11) | fill, k2 >> sh21, ((k2 & lo) << sh11) | fill


def _mp_normal2(k1, k2):
    with mpmath.workdps(50):
        u1 = mpmath.mpf(int(k1) + 1) / mpmath.mpf(2) ** 53
        u2 = mpmath.mpf(int(k2)) / mpmath.mpf(2) ** 53
        r = mpmath.sqrt(-2 * mpmath.log(u1))
        return r * mpmath.cospi(2 * u2), r * mpmath.sinpi(2 * u2)


def _ulps(got, want):
    """|got - want| in units of the float64 spacing at want (mpmath)."""
    with mpmath.workdps(50):
        if want == 0:
            return 0.0 if got == 0 else float("inf")
        return float(abs(mpmath.mpf(float(got)) - want) / mpmath.mpf(float(np.spacing(abs(float(want))))))


def _assert_close(got, want, where):
    with mpmath.workdps(50):
        err = abs(mpmath.mpf(float(got)) - want)
        assert err <= mpmath.mpf("1e-12") * abs(want), (where, float(got), float(want))


TOP = (1 << 53) - 1
QUADRANTS = [0, 1 << 51, 1 << 52, 3 << 51]  # u2 = 0, 1/4, 1/2, 3/4


def test_normal2_against_mpmath():
    rng = np.random.default_rng(12)
    k1 = [int(v) for v in rng.integers(0, 1 << 53, 300)]
    k2 = [int(v) for v in rng.integers(0, 1 << 53, 300)]
    # u1 at its ends and next to them, a small and a large radius on every special angle
    edge_k2 = sorted({(q + d) % (1 << 53) for q in QUADRANTS for d in (-1, 0, 1)})
    for a in (0, 1, TOP - 1, TOP, 12345678901234):
        for b in edge_k2:
            k1.append(a)
            k2.append(b)
    g0, g1 = pr.normal2(_c_from_k(k1, k2))
    worst = 0.0
    for i, (a, b) in enumerate(zip(k1, k2)):
        w0, w1 = _mp_normal2(a, b)
        _assert_close(g0[i], w0, (a, b, "g0"))
        _assert_close(g1[i], w1, (a, b, "g1"))
        worst = max(worst, _ulps(g0[i], w0), _ulps(g1[i], w1))
    print(f"normal2 vs mpmath (50 digits), {len(k1)} outputs: largest error {worst:.3f} ulp "
          f"= {worst * 2.0 ** -52:.2e} relative at most; bar 1e-12")
    assert worst < 16  # the restatement's own share of the 1e-12 budget (4500 ulp) stays negligible


def test_normal2_edges_exact():
    # the 11 ignored low bits do not matter
    a = pr.normal2(_c_from_k([5], [9]))
    c = [np.asarray(w) & np.uint64(0xFFFFF800) if i in (1, 3) else w for i, w in enumerate(_c_from_k([5], [9]))]
    b = pr.normal2(c)
    assert a[0][0] == b[0][0] and a[1][0] == b[1][0]
    # u1: k = 0 is 2^-53, the largest radius; k = 2^53 - 1 is u1 = 1 and radius 0
    k1, k2 = pr.uniforms53(_c_from_k([0, TOP], [0, TOP]))
    assert [int(v) for v in k1] == [0, TOP] and [int(v) for v in k2] == [0, TOP]
    g0, g1 = pr.normal2(_c_from_k([0, TOP, TOP], [0, 0, 12345]))
    assert g0[0] == np.sqrt(-2.0 * np.log(2.0 ** -53)) and 8.57 < g0[0] < 8.58 and g1[0] == 0.0
    assert g0[1] == 0.0 and g1[1] == 0.0 and g0[2] == 0.0 and g1[2] == 0.0
    # u2 on the quadrant points: exact zeros, and the radius itself on the other axis
    r = float(np.sqrt(-2.0 * np.log((777 + 1.0) * 2.0 ** -53)))
    g0, g1 = pr.normal2(_c_from_k([777] * 4, QUADRANTS))
    assert list(g0) == [r, 0.0, -r, 0.0]
    assert list(g1) == [0.0, r, 0.0, -r]
    # one step either side of a zero the value is a sine of about 7e-16, not 0 (and not cos(2 pi u2)'s 1e-16 noise)
    step = float(r * np.sin(np.pi * 2.0 ** -52))
    g0, g1 = pr.normal2(_c_from_k([777] * 4, [(1 << 51) - 1, (1 << 51) + 1, (1 << 52) - 1, (1 << 52) + 1]))
    assert list(g0[:2]) == [step, -step] and list(g1[2:]) == [step, -step]


def test_rows_do_not_depend_on_batch_size():
    bits5, bits2 = pr.rng_bits(SEED, STREAM, 5, 300), pr.rng_bits(SEED, STREAM, 2, 300)
    assert bits5.dtype == np.uint8 and bits5.shape == (5, 300) and set(np.unique(bits5)) == {0, 1}
    assert np.array_equal(bits5[:2], bits2)
    assert len({r.tobytes() for r in bits5}) == 5
    g5, g2 = pr.awgn_normals(SEED, STREAM, 5, 301), pr.awgn_normals(SEED, STREAM, 2, 301)
    assert np.array_equal(g5[:2], g2)
    # a shorter row is a prefix of a longer one (the counter is the element block alone)
    assert np.array_equal(pr.rng_bits(SEED, STREAM, 2, 129), bits2[:, :129])
    assert np.array_equal(pr.awgn_normals(SEED, STREAM, 2, 7), g2[:, :7])


def test_bit_layout():
    """Bit j of row b is bit j % 32 of word (j % 128) // 32 of Philox((j // 128, b, stream), seed ^ 0xB175)."""
    bits = pr.rng_bits(SEED, STREAM, 3, 300)
    for b, j in [(0, 0), (0, 31), (1, 32), (2, 127), (1, 128), (2, 299)]:
        w = _philox_int([j // 128, b, STREAM & 0xFFFFFFFF, STREAM >> 32],
                        [(SEED & 0xFFFFFFFF) ^ 0xB175, SEED >> 32])
        assert bits[b, j] == (w[(j % 128) // 32] >> (j % 32)) & 1, (b, j)


def test_normal_layout():
    """Samples 2q, 2q + 1 of row b are the normals of Philox((q, b, stream), seed ^ 0x0A1E)."""
    g = pr.awgn_normals(SEED, STREAM, 3, 11)
    for b, q in [(0, 0), (2, 3), (1, 5)]:
        w = _philox_int([q, b, STREAM & 0xFFFFFFFF, STREAM >> 32], [(SEED & 0xFFFFFFFF) ^ 0x0A1E, SEED >> 32])
        g0, g1 = pr.normal2([np.array([x], dtype=np.uint64) for x in w])
        assert g[b, 2 * q] == g0[0]
        if 2 * q + 1 < 11:
            assert g[b, 2 * q + 1] == g1[0]


def test_domains_seed_and_stream_words_all_count():
    base = pr.rng_bits(SEED, STREAM, 2, 256)
    # the noise domain's words are not the bit domain's
    (s_lo, s_hi), (t_lo, t_hi) = pr._split(SEED), pr._split(STREAM)
    wb = pr.philox4x32_10(0, 0, t_lo, t_hi, s_lo ^ pr.BITS_DOMAIN, s_hi)
    wn = pr.philox4x32_10(0, 0, t_lo, t_hi, s_lo ^ pr.NOISE_DOMAIN, s_hi)
    assert [int(x) for x in wb] != [int(x) for x in wn]
    # each 32-bit half of seed and stream changes the draw
    for seed, stream in [(SEED ^ 1, STREAM), (SEED ^ (1 << 32), STREAM), (SEED, STREAM ^ 1), (SEED, STREAM ^ (1 << 32))]:
        assert not np.array_equal(pr.rng_bits(seed, stream, 2, 256), base)
        assert not np.array_equal(pr.awgn_normals(seed, stream, 2, 8), pr.awgn_normals(SEED, STREAM, 2, 8))


def test_awgn_and_bpsk_llr_share_their_normals():
    B, n, sigma2 = 3, 7, 0.8
    g = pr.awgn_normals(SEED, STREAM, B, n)
    assert np.array_equal(pr.awgn(np.zeros((B, n)), 1.0, SEED, STREAM), g)
    cw = np.random.default_rng(3).integers(0, 2, (B, n)).astype(np.uint8)
    llr = pr.bpsk_llr(cw, sigma2, SEED, STREAM)
    assert np.array_equal(llr, (2.0 / sigma2) * ((1.0 - 2.0 * cw) + np.sqrt(sigma2) * g))
    x = np.random.default_rng(4).standard_normal((B, n)).astype(np.float32)
    assert np.array_equal(pr.awgn(x, 0.7, SEED, STREAM), x.astype(np.float64) + 0.7 * g)


def test_gen_A_layout_and_moments():
    n, LM = 3, 6  # 18 elements: the last Philox call is used by half
    A32 = pr.gen_A_float(SEED, n, LM)
    assert A32.dtype == np.float32 and A32.shape == (n, LM)
    assert np.array_equal(A32.reshape(-1), pr.gen_A_float(SEED, 1, 20).reshape(-1)[:18])
    w = _philox_int([4, 0, 0x5EED5EED, 0], [SEED & 0xFFFFFFFF, SEED >> 32])  # elements 16 .. 19
    u1, u2 = (w[0] + 1.0) / 4294967297.0, w[1] / 4294967296.0
    r = np.sqrt(-2.0 * np.log(u1))
    assert A32.reshape(-1)[16] == np.float32(r * np.cos(2.0 * np.pi * u2))
    assert A32.reshape(-1)[17] == np.float32(r * np.sin(2.0 * np.pi * u2))
    A = pr.gen_A(SEED, n, LM)
    assert A.dtype == np.float64 and np.array_equal(A, A32.astype(np.float64) * (1.0 / np.sqrt(3.0)))
    assert not np.array_equal(pr.gen_A_float(SEED ^ (1 << 32), n, LM), A32)
    big = pr.gen_A_float(5, 64, 1024).astype(np.float64)
    assert abs(big.mean()) < 5 / np.sqrt(big.size) and abs(big.var() - 1) < 5 * np.sqrt(2 / big.size)
