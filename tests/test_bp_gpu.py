"""GPU parity tests of the batched BP kernels (bp.hip) through the C ABI,
against the reference vectors (tests/golden/ldpc_golden_p*.npz, produced by the
reference's own c_ldpc.c) and the CPU restatement oracle/bp_oracle.c.

Bars: double-precision min-sum is bit-identical to the (index-corrected)
reference; sum-product variants use transcendental functions whose device
implementations may differ from glibc in the last ulp, so they must give the
same iteration counts and hard decisions with app within 1e-9 relative."""
import ctypes as ct

import numpy as np
import pytest

from ldpc_sparc_amd import _native
from ldpc_sparc_amd.ldpc import code
from oracle import bp

pytestmark = pytest.mark.gpu

ALL_CODES = [("802.16", r, z, p) for z in (3, 27, 54, 81)
             for (r, p) in [("1/2", "A"), ("2/3", "A"), ("2/3", "B"), ("3/4", "A"), ("3/4", "B"),
                            ("5/6", "A")]] + \
            [("802.11n", r, z, "A") for z in (27, 54, 81) for r in ("1/2", "2/3", "3/4", "5/6")]


def _awgn_batch(c, ebn0, B, rng):
    R = c.K / c.N
    s2 = 1 / (2 * R * 10 ** (ebn0 / 10))
    X = c.encode_batch(rng.integers(0, 2, (B, c.K)))
    y = (1 - 2 * X) + np.sqrt(s2) * rng.standard_normal(X.shape)
    return X, 2 * y / s2


def _cases(g):
    for ci in range(3):
        std, rate, z = [str(s) for s in g[f"c{ci}_meta"]]
        yield ci, std, rate, int(z)


@pytest.mark.parametrize("standard,rate,z,ptype", ALL_CODES)
def test_reference_noiseless_semantics(standard, rate, z, ptype):
    """test_ldpc.py:56-69 on the GPU: y = 10(0.5 - x) decodes in 0 iterations, exactly."""
    c = code(standard, rate, z, ptype)
    rng = np.random.default_rng(z + 1)
    X = c.encode_batch(rng.integers(0, 2, (16, c.K)))
    Y = np.array(10 * (.5 - X), dtype=float)
    for dt in ("sumprod", "sumprod2", "minsum"):
        app, it = c.decode_batch(Y, 200, dt)
        assert np.all(it == 0), dt
        assert np.array_equal((app < 0).astype(int), X), dt


@pytest.mark.parametrize("dectype", ["sumprod2", "sumprod"])
def test_sumproduct_vs_reference_vectors(ldpc_golden, dectype):
    for ci, std, rate, z in _cases(ldpc_golden):
        c = code(std, rate, z)
        for ei in range(3):
            ch = ldpc_golden[f"c{ci}_e{ei}_ch"]
            for mi in (5, 50, 200):
                key = f"c{ci}_e{ei}_{dectype}_{mi}"
                app, it = c.decode_batch(ch, mi, dectype)
                assert np.array_equal(it, ldpc_golden[key + "_it"]), key
                hard = (app < 0).astype(np.uint8)
                if mi == 200:
                    assert np.array_equal(hard, ldpc_golden[key + "_hard"]), key
                else:
                    ref = ldpc_golden[key + "_app"]
                    fin = np.isfinite(ref)
                    assert np.array_equal(fin, np.isfinite(app)), key
                    np.testing.assert_allclose(app[fin], ref[fin], rtol=1e-9, atol=1e-9, err_msg=key)
                    assert np.array_equal(hard[fin], (ref[fin] < 0).astype(np.uint8)), key


@pytest.mark.parametrize("std,rate,z", [("802.11n", "1/2", 81), ("802.11n", "1/2", 27),
                                        ("802.16", "3/4", 54), ("802.11n", "5/6", 27),
                                        ("802.16", "1/2", 96)])
def test_minsum_f64_bitexact_vs_oracle(std, rate, z):
    c = code(std, rate, z)
    rng = np.random.default_rng(11)
    for ebn0 in (1.0, 1.5, 2.0, 3.0):
        X, ch = _awgn_batch(c, ebn0, 24, rng)
        for mi in (1, 5, 50):
            app, it = c.decode_batch(ch, mi, "minsum", 0.7)
            oapp, oit = bp.decode_batch("minsum", ch, c.vdeg, c.cdeg, c.intrlv, mi, 0.7)
            assert np.array_equal(it, oit)
            assert np.array_equal(app, oapp)


def test_minsum_other_factor_and_golden_refbug_codes(ldpc_golden):
    """Corrected minsum at factor 1.0 and 0.8 (any factor is passed through, ldpc.py:463)."""
    c = code("802.11n", "1/2", 27)
    ch = ldpc_golden["c1_e1_ch"]
    for f in (1.0, 0.8):
        app, it = c.decode_batch(ch, 50, "minsum", f)
        oapp, oit = bp.decode_batch("minsum", ch, c.vdeg, c.cdeg, c.intrlv, 50, f)
        assert np.array_equal(app, oapp) and np.array_equal(it, oit)


def test_f32_minsum_matches_f64_statistically():
    c = code("802.11n", "1/2", 81)
    rng = np.random.default_rng(5)
    X, ch = _awgn_batch(c, 1.5, 512, rng)
    a64, i64 = c.decode_batch(ch, 50, "minsum")
    a32, i32 = c.decode_batch(ch, 50, "minsum", precision="f32")
    fe64 = np.any((a64 < 0) != X, axis=1)
    fe32 = np.any((a32 < 0) != X, axis=1)
    # same frames decode: at most a handful differ, iteration counts close
    assert np.sum(fe64 != fe32) <= 5
    assert abs(i64.mean() - i32.mean()) < 0.5


def test_scalar_shims_match_batched():
    """The reference-compatible C entry points (ctypes targets of ldpc.py:481-503)."""
    L = _native.lib()
    c = code("802.11n", "1/2", 27)
    rng = np.random.default_rng(2)
    X, ch = _awgn_batch(c, 1.5, 3, rng)
    v = c.vdeg.astype(np.int64); cd = c.cdeg.astype(np.int64); iv = c.intrlv.astype(np.int64)
    for row in ch:
        row = np.ascontiguousarray(row)
        for dt, fn in (("sumprod2", L.sumprod2), ("sumprod", L.sumprod)):
            app = np.zeros(c.N)
            it = fn(row.ctypes.data_as(_native.dp), v.ctypes.data_as(_native.lp),
                    cd.ctypes.data_as(_native.lp), iv.ctypes.data_as(_native.lp), c.Nv, c.Nc,
                    c.Nmsg, app.ctypes.data_as(_native.dp), 50)
            a2, i2 = c.decode(row, 50, dt)
            assert it == i2 and np.array_equal(app, a2, equal_nan=True)
        app = np.zeros(c.N)
        it = L.minsum(row.ctypes.data_as(_native.dp), v.ctypes.data_as(_native.lp),
                      cd.ctypes.data_as(_native.lp), iv.ctypes.data_as(_native.lp), c.Nv, c.Nc,
                      c.Nmsg, app.ctypes.data_as(_native.dp), 0.7, 50)
        oapp, oit = bp.decode("minsum", row, c.vdeg, c.cdeg, c.intrlv, 50, 0.7)
        assert it == oit and np.array_equal(app, oapp)


def test_lxor_lxfb_on_device():
    c = code()
    rng = np.random.default_rng(9)
    for _ in range(10):
        a, b = rng.standard_normal(2) * 4
        for corr in (0, 1):
            np.testing.assert_allclose(c.Lxor(a, b, corr), bp.lxor(a, b, corr), rtol=1e-12, atol=1e-14)
        L = rng.standard_normal(6) * 3
        agg, out = c.Lxfb(L, 1)
        oagg, oout = bp.lxfb(L, 1)
        np.testing.assert_allclose(agg, oagg, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(out, oout, rtol=1e-12, atol=1e-14)
        agg0, out0 = c.Lxfb(L, 0)
        oagg0, oout0 = bp.lxfb(L, 0)
        assert agg0 == oagg0 and np.array_equal(out0, oout0)


@pytest.mark.parametrize("B", [300, 5000])
def test_device_api_and_error_counter(B):
    """Device decode + error counters; B = 5000 is more codewords than the
    counter's 1024 wavefronts, so each loops over several."""
    c = code("802.11n", "1/2", 81)
    rng = np.random.default_rng(4)
    X, ch = _awgn_batch(c, 1.25, B, rng)
    L = _native.lib()
    g = c._device_graph()
    d_ch = _native.DeviceBuffer.from_array(ch.astype(np.float32))
    d_app = _native.DeviceBuffer(ch.size * 4)
    d_it = _native.DeviceBuffer(ch.shape[0] * 4)
    d_x = _native.DeviceBuffer.from_array(X.astype(np.uint8))
    d_cnt = _native.DeviceBuffer(4 * 8)
    d_cnt.zero()
    _native.check(L.sg_ldpc_decode_device(g, _native.SG_MINSUM, _native.SG_F32, d_ch.ptr,
                                          ch.shape[0], 50, 0.7, d_app.ptr, d_it.ptr, None))
    _native.check(L.sg_ldpc_count_errors_device(g, _native.SG_F32, d_app.ptr, d_x.ptr, d_it.ptr,
                                                ch.shape[0], c.K, d_cnt.ptr, None))
    _native.synchronize()
    app = d_app.download(np.zeros(ch.shape, np.float32))
    it = d_it.download(np.zeros(ch.shape[0], np.int32))
    cnt = d_cnt.download(np.zeros(4, np.int64))
    err = (app < 0) != X
    assert cnt[0] == err.sum()
    assert cnt[1] == np.any(err, axis=1).sum()
    assert cnt[2] == err[:, :c.K].sum()
    assert cnt[3] == it.sum()
    d_be = _native.DeviceBuffer(B * 4)
    _native.check(L.sg_ldpc_codeword_errors_device(g, _native.SG_F32, d_app.ptr, d_x.ptr, B, d_be.ptr, None))
    _native.synchronize()
    assert np.array_equal(d_be.download(np.zeros(B, np.int32)), err.sum(axis=1))


@pytest.mark.parametrize("std,rate,z", [("802.11n", "5/6", 81), ("802.16", "5/6", 96), ("802.11n", "3/4", 54)])
def test_high_degree_sumprod2_vs_oracle(std, rate, z):
    """High-rate codes (check degrees 14-22) through the register-lean check
    update (Lxfb backward values in LDS scratch, c_ldpc.c:294-314): f64 gives
    the oracle's iteration counts and hard decisions with app within 1e-9;
    f32 the same decisions on >= 98 % of the codewords."""
    c = code(std, rate, z)
    assert int(c.cdeg.max()) > 8
    rng = np.random.default_rng(17)
    X, ch = _awgn_batch(c, 4.0, 48, rng)
    for mi in (5, 50):
        app, it = c.decode_batch(ch, mi, "sumprod2")
        oapp, oit = bp.decode_batch("sumprod2", ch, c.vdeg, c.cdeg, c.intrlv, mi, 0.7)
        assert np.array_equal(it, oit)
        assert np.array_equal(app < 0, oapp < 0)
        np.testing.assert_allclose(app, oapp, rtol=1e-9, atol=1e-9)
        a32, i32 = c.decode_batch(ch, mi, "sumprod2", precision="f32")
        assert np.mean(np.all((a32 < 0) == (oapp < 0), axis=1)) >= 0.98
    for dt in ("minsum", "sumprod"):
        app, it = c.decode_batch(ch, 50, dt, 0.7)
        oapp, oit = bp.decode_batch(dt, ch, c.vdeg, c.cdeg, c.intrlv, 50, 0.7)
        assert np.array_equal(it, oit), dt
        assert np.array_equal(app < 0, oapp < 0), dt
        if dt == "minsum":
            assert np.array_equal(app, oapp)
