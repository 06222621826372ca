"""GPU tests that pin the device Monte-Carlo generator (csrc/philox.hpp,
channel.hip, gen_A_kernel of dense.hip, bp_count_kernel of bp.hip) to its
host restatement, tests/philox_ref.py, value for value.

Bars:
  * bits, section indices, encoder, error counts: exact;
  * float64 normals, AWGN and BPSK LLRs: |dev - ref| <= 1e-12 * (sum of the
    magnitudes of the terms), the suite's float64 bar (F64_BAR below); the
    compiler may contract the multiply-add, so equality is not asked;
  * float32 outputs: within one float32 step (np.nextafter) of
    float32(restatement): the double error is far below half a float32 ulp,
    so only a rounding tie can move the result, and by one step;
  * random design: the kernel rounds each unit normal to float32 before the
    scale, so the float32 intermediate may sit one step either side of the
    restatement's; an entry must lie between the two neighbours' images
    (times the scale, rounded to the plan's type).

Seed and stream have both 32-bit halves nonzero and distinct.  Every output
buffer the tests allocate carries a guard tail (GUARD bytes of 0xA5) that must
come back untouched; sg_dense_plan_create_random writes into the plan's own
allocation, which has no tail to check.
"""
import ctypes as ct

import numpy as np
import pytest

import philox_ref as pr
from ldpc_sparc_amd import _native, montecarlo
from ldpc_sparc_amd.ldpc import code

pytestmark = pytest.mark.gpu

SEED, STREAM = 0xFEDCBA9876543210, (7 << 32) | 5
GUARD, FILL = 64, 0xA5
F32, F64 = _native.SG_F32, _native.SG_F64

# The float64 bar of the suite (test_bp_gpu.py::test_lxor_lxfb_on_device, test_amp_encode_device).
F64_BAR = 1e-12
# Largest |dev - ref| / |ref| of the device normals (sg_awgn_device, f64, x = 0, sigma = 1) against
# philox_ref.awgn_normals observed on an MI355X over the cases of test_awgn_f64_returns_the_normals
# (printed by that test): 2.4 ulp, 1900 times below the bar.  The restatement itself is within 2.4 ulp =
# 5.3e-16 of mpmath (test_philox_host.py), so the device's log / sqrt / sincospi are as good as the host's.
# A record, not a bar: the bar stays F64_BAR.
F64_NORMALS_OBSERVED = 5.366e-16


def _lib():
    return _native.lib()


def _dtype(prec):
    return np.float64 if prec == F64 else np.float32


class Out:
    """A device output buffer of nbytes, pre-filled with FILL (or zeros), with a guard tail of FILL."""

    def __init__(self, nbytes, zero=False):
        self.n = int(nbytes)
        host = np.full(self.n + GUARD, FILL, np.uint8)
        if zero:
            host[:self.n] = 0
        self.buf = _native.DeviceBuffer.from_array(host)
        self.ptr = self.buf.ptr

    def read(self, shape, dtype=np.uint8):
        _native.synchronize()
        raw = self.buf.download(np.empty(self.n + GUARD, np.uint8))
        assert np.all(raw[self.n:] == FILL), "guard tail overwritten"
        out = raw[:self.n].view(dtype).reshape(shape)
        assert out.nbytes == self.n
        return out


def _assert_f64(dev, ref, mag, what):
    """|dev - ref| <= F64_BAR * mag, NaN-free."""
    err = np.abs(dev - ref)
    assert np.all(err <= F64_BAR * mag), (what, float(np.max(err / np.maximum(mag, 1e-300))))


def _assert_f32_step(dev, ref64, what):
    """dev (float32) within one float32 step of float32(ref64)."""
    r = ref64.astype(np.float32)
    lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
    bad = ~((dev >= lo) & (dev <= hi))
    assert not bad.any(), (what, int(bad.sum()), dev[bad][:4], r[bad][:4])


# ---------------------------------------------------------------- sg_rng_bits_device
def _dev_bits(seed, stream, B, nbits):
    o = Out(B * nbits)
    _native.check(_lib().sg_rng_bits_device(seed, stream, B, nbits, o.ptr, None))
    return o.read((B, nbits))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nbits", [1, 127, 128, 129, 324, 1000])
def test_rng_bits_exact(nbits, B):
    assert np.array_equal(_dev_bits(SEED, STREAM, B, nbits), pr.rng_bits(SEED, STREAM, B, nbits))


def test_rng_bits_stride_loop():
    """128 (1024 * 256) + 129 bits: the grid of 1024 workgroups covers 1024 * 256 blocks of 128 bits,
    so two threads take a second turn of the loop, the last one on a block of one bit."""
    nbits = 128 * (1024 * 256) + 129
    assert np.array_equal(_dev_bits(SEED, STREAM, 1, nbits), pr.rng_bits(SEED, STREAM, 1, nbits))


def test_rng_bits_rows_do_not_depend_on_batch():
    a, b = _dev_bits(SEED, STREAM, 5, 324), _dev_bits(SEED, STREAM, 2, 324)
    assert a[:2].tobytes() == b.tobytes()
    assert np.array_equal(a, pr.rng_bits(SEED, STREAM, 5, 324))


# ---------------------------------------------------------------- sg_awgn_device
def _dev_awgn(prec, x, sigma, seed=SEED, stream=STREAM):
    dt = _dtype(prec)
    x = np.ascontiguousarray(x, dtype=dt)
    B, n = x.shape
    d_x = _native.DeviceBuffer.from_array(x)
    o = Out(x.nbytes)
    _native.check(_lib().sg_awgn_device(prec, seed, stream, d_x.ptr, B, n, float(sigma), o.ptr, None))
    return o.read((B, n), dt)


AWGN_SHAPES = [(3, 1), (3, 2), (3, 3), (3, 257), (3, 1001), (1, 2 * 1024 * 256 + 3)]  # the last: stride loop


def test_awgn_f64_returns_the_normals():
    """x = 0, sigma = 1: y is the device normal itself (0 + 1 * g is exact)."""
    worst = 0.0
    for B, n in AWGN_SHAPES:
        y = _dev_awgn(F64, np.zeros((B, n)), 1.0)
        g = pr.awgn_normals(SEED, STREAM, B, n)
        rel = np.abs(y - g) / np.maximum(np.abs(g), np.finfo(np.float64).tiny)
        worst = max(worst, float(np.max(rel)))
        assert np.all(np.abs(y - g) <= F64_BAR * np.abs(g)), (B, n, float(np.max(rel)))
    print(f"device normals vs philox_ref, f64: largest relative deviation {worst:.3e} (bar {F64_BAR:g})")


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("B,n", AWGN_SHAPES)
def test_awgn_general(prec, B, n):
    sigma = 0.7
    x = np.random.default_rng(n).standard_normal((B, n)).astype(_dtype(prec))
    y = _dev_awgn(prec, x, sigma)
    ref = pr.awgn(x, sigma, SEED, STREAM)
    if prec == F64:
        g = pr.awgn_normals(SEED, STREAM, B, n)
        _assert_f64(y, ref, np.abs(x) + sigma * np.abs(g), (B, n))
    else:
        _assert_f32_step(y, ref, (B, n))


def test_awgn_sigma_zero_is_a_copy():
    x = np.random.default_rng(0).standard_normal((3, 7))
    assert np.array_equal(_dev_awgn(F64, x, 0.0), x)


# ---------------------------------------------------------------- sg_bpsk_awgn_llr_device
@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("N", [1, 7, 648])
def test_bpsk_llr(prec, N):
    B, sigma2 = 3, 0.8
    cw = np.random.default_rng(N).integers(0, 2, (B, N)).astype(np.uint8)
    d_c = _native.DeviceBuffer.from_array(cw)
    o = Out(B * N * np.dtype(_dtype(prec)).itemsize)
    _native.check(_lib().sg_bpsk_awgn_llr_device(prec, SEED, STREAM, d_c.ptr, B, N, sigma2, o.ptr, None))
    llr = o.read((B, N), _dtype(prec))
    ref = pr.bpsk_llr(cw, sigma2, SEED, STREAM)
    if prec == F64:
        g = pr.awgn_normals(SEED, STREAM, B, N)
        _assert_f64(llr, ref, (2.0 / sigma2) * (1.0 + np.sqrt(sigma2) * np.abs(g)), N)
    else:
        _assert_f32_step(llr, ref, N)


# ---------------------------------------------------------------- sg_dense_plan_create_random
# (n, L, M): the constructor takes any n, L > 0 and M a power of two; the f32 plan also needs L M % 32 == 0.
DENSE_F64 = [(1, 1, 1), (3, 3, 2), (5, 1, 2), (2, 1, 4), (7, 3, 8)]  # n L M = 1, 18, 10: no multiple of 4
DENSE_F32 = [(1, 1, 32), (3, 1, 32), (5, 3, 32), (2, 16, 2)]


@pytest.mark.parametrize("seed", [SEED, 5])
@pytest.mark.parametrize("prec,shape", [(F64, s) for s in DENSE_F64] + [(F32, s) for s in DENSE_F32])
def test_random_design(prec, shape, seed):
    """Every entry within one float32 step (of the intermediate) of philox_ref.gen_A.  In f64 the
    shapes include n L M = 1, 10 and 18, where the last thread writes fewer than four entries; the
    f32 constructor only takes L M % 32 == 0, so n L M is always a multiple of 4 there."""
    n, L, M = shape
    lib, dt = _lib(), _dtype(prec)
    plan = ct.c_void_p()
    _native.check(lib.sg_dense_plan_create_random(n, L, M, 1.0, seed, prec, ct.byref(plan)))
    try:
        d_A = ct.c_void_p()
        _native.check(lib.sg_dense_plan_matrix_device(plan, ct.byref(d_A)))
        A = np.empty((n, L * M), dt)
        _native.check(lib.sg_memcpy_d2h(_native.ptr(A), d_A, A.nbytes, None))
    finally:
        lib.sg_dense_plan_destroy(plan)
    a32, scale = pr.gen_A_float(seed, n, L * M), pr.gen_A_scale(n)
    lo = (np.nextafter(a32, np.float32(-np.inf)).astype(np.float64) * scale).astype(dt)
    hi = (np.nextafter(a32, np.float32(np.inf)).astype(np.float64) * scale).astype(dt)
    assert np.all((A >= lo) & (A <= hi)), (shape, int(np.sum(~((A >= lo) & (A <= hi)))))
    # The double values under the float32 rounding differ by a few double ulps between the device's and
    # numpy's log / cos / sin, so a different float32 needs a value within about 1e-8 of a float32 ulp of
    # a rounding boundary: over these few hundred entries the restatement's own value is the rule.
    if A.size >= 32:
        assert np.mean(A == pr.gen_A(seed, n, L * M).astype(dt)) >= 0.9


# ---------------------------------------------------------------- bits -> section indices
@pytest.mark.parametrize("L", [1, 33, 257])
@pytest.mark.parametrize("logM", [1, 9, 30])
def test_bits_to_sections(logM, L):
    """MSB first, only bit 0 of an input byte counts (inputs are 0xFE / 0xFF); the strided form
    with both strides longer than a row leaves the gaps of the output alone."""
    lib, B = _lib(), 3
    row = L * logM
    bits = np.random.default_rng(logM * 1000 + L).integers(0, 2, (B, row)).astype(np.uint8)
    want = (bits.reshape(B, L, logM).astype(np.int64) @ (1 << np.arange(logM)[::-1])).astype(np.int32)
    bit_stride, idx_stride = row + 13, L + 5
    padded = np.full((B, bit_stride), 0xFF, np.uint8)  # gap bytes would read as 1 if the stride were ignored
    padded[:, :row] = bits | 0xFE
    d_b = _native.DeviceBuffer.from_array(padded)
    o = Out(B * idx_stride * 4)
    _native.check(lib.sg_bits_to_sections_strided_device(d_b.ptr, bit_stride, B, L, logM, o.ptr, idx_stride, None))
    got = o.read((B, idx_stride), np.int32)
    assert np.array_equal(got[:, :L], want)
    assert np.all(got[:, L:].view(np.uint8) == FILL), "gap between index rows overwritten"
    d_b = _native.DeviceBuffer.from_array(bits | 0xFE)
    o = Out(B * L * 4)
    _native.check(lib.sg_bits_to_sections_device(d_b.ptr, B, L, logM, o.ptr, None))
    assert np.array_equal(o.read((B, L), np.int32), want)


# ---------------------------------------------------------------- sg_ldpc_encode_device
def _high_bits(bits, rng):
    """The same bits with random values in bits 1..7 of every byte."""
    return (bits | (rng.integers(0, 128, bits.shape) << 1)).astype(np.uint8)


def test_encoder_802_16():
    c = code("802.16", "1/2", 24)
    rng = np.random.default_rng(16)
    B = 5
    info = rng.integers(0, 2, (B, c.K)).astype(np.uint8)
    d_i = _native.DeviceBuffer.from_array(_high_bits(info, rng))
    o = Out(B * c.N)
    c.encode_device(d_i.ptr, B, o.ptr)
    cw = o.read((B, c.N))
    assert np.array_equal(cw, c.encode_batch(info).astype(np.uint8))
    assert np.array_equal(cw[:, :c.K], info)
    assert not np.any((cw.astype(np.int64) @ c.pcmat().T) % 2)


@pytest.mark.parametrize("R", [1, 300])  # 300 parity bits: more than the 256 threads of the workgroup
@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
def test_encoder_synthetic(K, R):
    lib, B = _lib(), 5
    rng = np.random.default_rng(K * 1000 + R)
    P = rng.integers(0, 2, (K, R)).astype(np.uint8)
    info = rng.integers(0, 2, (B, K)).astype(np.uint8)
    info[0] = 1  # every word of the packed information row full up to bit K - 1
    enc = ct.c_void_p()
    _native.check(lib.sg_ldpc_encoder_create(_native.ptr(P), K, K + R, ct.byref(enc)))
    try:
        d_i = _native.DeviceBuffer.from_array(_high_bits(info, rng))
        o = Out(B * (K + R))
        _native.check(lib.sg_ldpc_encode_device(enc, d_i.ptr, B, o.ptr, None))
        cw = o.read((B, K + R))
    finally:
        lib.sg_ldpc_encoder_destroy(enc)
    want = np.concatenate([info, (info.astype(np.int64) @ P.astype(np.int64) % 2).astype(np.uint8)], axis=1)
    assert np.array_equal(cw, want)


# ---------------------------------------------------------------- error counters
def _random_graph(vdegs, nv, rng, cmax=8, cmin=2):
    vdeg = np.array([vdegs[v % len(vdegs)] for v in range(nv)], dtype=np.int64)
    E = int(vdeg.sum())
    cdeg, left = [], E
    while left > 0:
        d = int(min(left, rng.integers(cmin, cmax + 1)))
        if left - d == 1:
            d += 1
        cdeg.append(d)
        left -= d
    return vdeg, np.array(cdeg, dtype=np.int64), rng.permutation(E).astype(np.int64)


@pytest.fixture(scope="module", params=[300, 301], ids=["nv300", "nv301"])
def graph(request):
    """nv = 300: rows of four f32 values (the vector path); nv = 301: the scalar path."""
    nv = request.param
    vdeg, cdeg, intrlv = _random_graph([3, 2, 4], nv, np.random.default_rng(nv))
    g = ct.c_void_p()
    _native.check(_lib().sg_ldpc_graph_create(_native.ptr(vdeg), _native.ptr(cdeg), _native.ptr(intrlv),
                                              len(vdeg), len(cdeg), len(intrlv), ct.byref(g)))
    yield g, nv
    _lib().sg_ldpc_graph_destroy(g)


def _count_case(B, nv, dt, rng):
    """app with every special value next to the decision app < 0, the bits, the iteration counts."""
    tiny = np.finfo(dt).smallest_subnormal
    special = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, tiny, -tiny, 100 * tiny, -100 * tiny], dtype=dt)
    app = rng.standard_normal((B, nv)).astype(dt)
    mask = rng.random((B, nv)) < 0.3
    app[mask] = special[rng.integers(0, len(special), int(mask.sum()))]
    x = rng.integers(0, 2, (B, nv)).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        hard = (app < 0).astype(np.uint8)
    x[0] = 1 - hard[0]  # row 0: every bit in error, so the count over the first k bits is k itself
    if B > 1:
        x[1] = hard[1]  # row 1: no error
    its = rng.integers(0, 200, B).astype(np.int32)
    return app, x, hard, its


@pytest.mark.parametrize("B", [1, 3, 4, 5, 1025])  # 1025: past the 4 * 256 wavefronts of the grid
@pytest.mark.parametrize("prec", [F32, F64])
def test_count_errors(graph, prec, B):
    g, nv = graph
    lib, dt = _lib(), _dtype(prec)
    app, x, hard, its = _count_case(B, nv, dt, np.random.default_rng(B * 10 + prec))
    err = (hard != x).astype(np.int64)
    per_cw = err.sum(axis=1)
    assert per_cw[0] == nv and (B == 1 or per_cw[1] == 0)
    d_app, d_x, d_it = (_native.DeviceBuffer.from_array(a) for a in (app, x, its))
    # the same values one element further on: the f32 rows are no longer 16-byte aligned (scalar path)
    shifted = _native.DeviceBuffer.from_array(np.concatenate([np.zeros(1, dt), app.reshape(-1)]))
    for k in (0, 1, 2, 3, 5, nv - 1, nv):
        want = np.array([per_cw.sum(), np.count_nonzero(per_cw), err[:, :k].sum(), its.sum()], dtype=np.int64)
        for a_ptr in (d_app.ptr, _native.offset(shifted.ptr, np.dtype(dt).itemsize)):
            cnt = Out(32, zero=True)
            _native.check(lib.sg_ldpc_count_errors_device(g, prec, a_ptr, d_x.ptr, d_it.ptr, B, k, cnt.ptr, None))
            assert np.array_equal(cnt.read(4, np.int64), want), (k, "first call")
            _native.check(lib.sg_ldpc_count_errors_device(g, prec, a_ptr, d_x.ptr, None, B, k, cnt.ptr, None))
            want2 = 2 * want
            want2[3] = want[3]  # d_it = NULL adds no iterations
            assert np.array_equal(cnt.read(4, np.int64), want2), (k, "counters accumulate")
    for a_ptr in (d_app.ptr, _native.offset(shifted.ptr, np.dtype(dt).itemsize)):
        be = Out(B * 4)
        _native.check(lib.sg_ldpc_codeword_errors_device(g, prec, a_ptr, d_x.ptr, B, be.ptr, None))
        assert np.array_equal(be.read(B, np.int32), per_cw)


# ---------------------------------------------------------------- stream derivation, end to end
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_ldpc_trial_streams(precision):
    """LdpcTrial(rng='device') draws block blk of point p from Philox stream (p << 32) | blk, bits
    and noise, at the block's offset in the batch: pinned without a decoder."""
    c = code("802.11n", "1/2", 27)
    point, first, n_blocks, block, sigma2 = 1, 3, 2, 8, 0.8
    tr = montecarlo.LdpcTrial(c, [1.0, 2.0], precision=precision, seed=SEED, rng="device")
    d_x, d_ch, B = tr._device_batch(point, first, n_blocks, block, sigma2)
    assert B == n_blocks * block
    _native.synchronize()
    dt = np.float64 if precision == "f64" else np.float32
    x = d_x.download(np.zeros((B, c.N), np.uint8))
    ch = d_ch.download(np.zeros((B, c.N), dt))
    for i in range(n_blocks):
        sid = (point << 32) | (first + i)
        rows = slice(i * block, (i + 1) * block)
        want = c.encode_batch(pr.rng_bits(SEED, sid, block, c.K)).astype(np.uint8)
        assert np.array_equal(x[rows], want), i
        ref = pr.bpsk_llr(want, sigma2, SEED, sid)
        if precision == "f64":
            g = pr.awgn_normals(SEED, sid, block, c.N)
            _assert_f64(ch[rows], ref, (2.0 / sigma2) * (1.0 + np.sqrt(sigma2) * np.abs(g)), i)
        else:
            _assert_f32_step(ch[rows], ref, i)
