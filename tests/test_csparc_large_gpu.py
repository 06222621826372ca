"""GPU parity tests of the complex engine at transform sizes 2^17 to 2^20
(amp_cfft.hip's asymmetric split: P = 256, long-row pass B), with the bars of
tests/test_csparc_gpu.py:
  * design operators within 1e-12 of the NumPy restatement (tests/csparc_ref.py)
    and the encoder's x within 1e-12 of the golden x, relative to the output's
    max magnitude;
  * decode: t_final and every MAP location / symbol equal to the reference's
    on every case-seed of tests/golden/csparc_large_golden.npz, NMSE per
    iteration within 1e-9 absolute;
  * sparc_sim: the reference's error statistics reproduced exactly;
  * a batch decodes bit-identically to one of its codewords decoded alone;
  * the device-resident campaign path (encode, CSparcTrial) at w = 2^17 agrees
    with the host entry points, as in tests/test_csparc_campaign_gpu.py.
"""
import ctypes as ct
import functools

import numpy as np
import pytest

import csparc_ref
from csparc_large_cases import AWGN_VAR, CASES, K_of, all_seeds, golden, seed_of, transforms
from ldpc_sparc_amd import _native, montecarlo, sparc, sparc_sim

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


@functools.lru_cache(maxsize=None)
def _design(name, si):
    """(cp, W, n, operator) of a case-seed; the operator's plan is built once."""
    cp, W, n, Ab, Az = transforms(name, si)
    return cp, W, n, sparc.operator_of(Ab, Az)


def _true_indices(g, key, M, K):
    return sparc._msg_vector_indices(sparc.bin_arr_2_msg_vector(g[key + "_bits"], M, K), M, K)


@pytest.mark.parametrize("w_exp,Mr", [(17, 700), (18, 1500), (19, 2500), (20, 4000)])
def test_operator_sizes_large(w_exp, Mr):
    """The construction of test_csparc_gpu.test_operator_sizes at w = 2^17 ... 2^20."""
    w = 2 ** w_exp
    Mc = w // 2 + 3
    L, M = Mc, 1
    rng = np.random.RandomState(w_exp)
    idx0 = np.delete(np.arange(w, dtype=np.uint32), [0, w // 2]); rng.shuffle(idx0)
    idx1 = np.delete(np.arange(w, dtype=np.uint32), [0, w // 2]); rng.shuffle(idx1)
    o0, o1 = idx0[:Mr], idx1[:Mc]
    W = np.array(3.0)
    op = sparc.ComplexDesignOperator(W, L, M, Mr, o0, o1)
    assert op.w == w
    Ab, Az = csparc_ref.fft_operators(W, L, M, Mr, o0, o1)
    rng = np.random.default_rng(w_exp)
    X = rng.standard_normal((3, L * M)) + 1j * rng.standard_normal((3, L * M))
    Y = rng.standard_normal((3, Mr)) + 1j * rng.standard_normal((3, Mr))
    gx, gy = op.apply(X, False), op.apply(Y, True)
    for b in range(3):
        ex, ey = _rel(gx[b], Ab(X[b])), _rel(gy[b], Az(Y[b]))
        print("w 2^%d vector %d: A x rel err %.3g, A^H y rel err %.3g" % (w_exp, b, ex, ey))
        assert ex < 1e-12
        assert ey < 1e-12
    w_, nT, Mr_, Mc_, P, Q = (ct.c_int() for _ in range(6))
    _native.check(_native.lib().sg_camp_plan_info(op.plan(), *(ct.byref(v) for v in (w_, nT, Mr_, Mc_, P, Q))))
    assert (w_.value, nT.value, Mr_.value, Mc_.value) == (w, 1, Mr, Mc)
    assert P.value * Q.value == w and P.value == 256


def test_rejected_above_2_20():
    """log2 w = 21 stays unsupported."""
    L, M, Mr = 2 ** 20 + 1, 1, 8
    o0 = np.arange(1, Mr + 1, dtype=np.uint32)
    o1 = np.arange(1, L + 1, dtype=np.uint32)
    W = np.array([3.0])
    h = ct.c_void_p()
    p = _native.ptr
    rc = _native.lib().sg_camp_plan_create(0, p(W), 1, 1, L, M, Mr, p(o0), p(o1), ct.byref(h))
    assert rc == -6  # SG_ERR_UNSUPPORTED
    assert b"w=2^21" in _native.lib().sg_last_error()
    op = sparc.ComplexDesignOperator(np.array(3.0), L, M, Mr, o0, o1)
    assert op.w == 2 ** 21
    with pytest.raises(_native.NativeError, match="outside"):
        op.plan()


@pytest.mark.parametrize("name,cp,dp,si", list(all_seeds()))
def test_encode_x_matches_reference(name, cp, dp, si):
    g, key = golden(), f"{name}_s{si}"
    bits, beta0, x, Ab, Az = sparc.sparc_encode(dict(cp), AWGN_VAR, seed_of(si))
    assert np.array_equal(bits, g[key + "_bits"])
    assert x.dtype == np.complex128
    err = _rel(x, g[key + "_x"])
    print(key, "encode rel err", err)
    assert err < 1e-12, key


@pytest.mark.parametrize("name,cp,dp,si", list(all_seeds()))
def test_decode_matches_reference(name, cp, dp, si):
    g, key = golden(), f"{name}_s{si}"
    cp, W, n, op = _design(name, si)
    dp = dict(dp)
    sparc.check_decode_params(dp)
    K, L, M = K_of(cp), cp['L'], cp['M']
    assert op.w == 2 ** CASES[name][4]
    ti, ts = _true_indices(g, key, M, K)
    mi, ms, tf, nmse, psi = sparc.camp_decode_batch(g[key + "_y"][None], op, AWGN_VAR, dp['t_max'], dp['rtol'],
                                                    dp['phi_est_method'], K, ti[None], ts[None])
    ref_nmse = g[key + "_nmse"]
    print(key, "t_final", tf[0], int(g[key + "_t_final"]), "max nmse diff",
          np.abs(nmse[0].reshape(ref_nmse.shape) - ref_nmse).max())
    assert tf[0] == int(g[key + "_t_final"]), key
    assert np.array_equal(mi[0], g[key + "_map"]), key
    assert np.array_equal(ms[0], g[key + "_map_sym"]), key
    np.testing.assert_allclose(nmse[0].reshape(ref_nmse.shape), ref_nmse, rtol=0, atol=1e-9, err_msg=key)


@pytest.mark.parametrize("name,cp,dp,si", list(all_seeds(("cbig17", "cbig18sc"))))
def test_sparc_sim_dropin_matches_reference(name, cp, dp, si):
    """sparc_sim (the reference's call surface) end to end on the GPU."""
    g, key = golden(), f"{name}_s{si}"
    res = sparc_sim.sparc_sim(dict(cp), dict(dp), AWGN_VAR, seed_of(si))
    scalars = ['ber', 'ser', 't_final', 'detect']
    arrays = ['loc_of_sec_errs']
    if cp.get('modulated'):
        scalars += ['ler', 'ver', 'num_of_sec_errs', 'num_of_loc_errs', 'num_of_val_errs']
        arrays += ['loc_of_loc_errs', 'loc_of_val_errs']
    for k in scalars:
        assert res[k] == g[key + "_sim_" + k].item(), (key, k)
    for k in arrays:
        assert np.array_equal(res[k], g[key + "_sim_" + k]), (key, k)


def test_batch_equals_single():
    """Three noisy copies of cbig18sc's seed-0 codeword (8 transforms of 2^18
    points) at variances 0.3, 1.0 and 3.0: the batch is bit-identical, on all
    five outputs, to codeword 1 decoded alone."""
    g = golden()
    cp, W, n, op = _design("cbig18sc", 0)
    L, M = cp['L'], cp['M']
    x = g["cbig18sc_s0_x"]
    rng = np.random.RandomState(3)
    Y = np.stack([x + np.sqrt(v / 2) * (rng.randn(n) + 1j * rng.randn(n)) for v in (0.3, 1.0, 3.0)])
    ti, ts = _true_indices(g, "cbig18sc_s0", M, 1)
    TI, TS = np.tile(ti, (3, 1)), np.tile(ts, (3, 1))
    full = sparc.camp_decode_batch(Y, op, AWGN_VAR, 40, 1e-6, 1, 1, TI, TS)
    print("t_final of the batch", full[2])
    one = sparc.camp_decode_batch(Y[1:2], op, AWGN_VAR, 40, 1e-6, 1, 1, TI[1:2], TS[1:2])
    for a, o in zip(full, one):
        assert np.array_equal(a[1], o[0])


# ------------------------------------------------------------------ campaign path at w = 2^17
def _up(a, dtype):
    return _native.DeviceBuffer.from_array(np.ascontiguousarray(a, dtype=dtype))


def _down(buf, shape, dtype):
    _native.synchronize()
    return buf.download(np.zeros(shape, dtype=dtype))


def _msg(idx, sym, M, K):
    return sparc._msg_vector_from_indices(idx, sym, M, K)


def _host_counts(ti, ts, mi, ms, tf, L, M, K):
    """Per-codeword rows [1, bit, codeword, t_final, section, location, value errors]
    from calc_ler_ver and calc_ber over msg_vector_2_bin_arr."""
    rows = []
    for b in range(len(ti)):
        b0, b1 = _msg(ti[b], ts[b], M, K), _msg(mi[b], ms[b], M, K)
        _, _, (nloc, nval, nsec) = sparc_sim.calc_ler_ver(b0, b1, L, K)
        bits0, bits1 = sparc.msg_vector_2_bin_arr(b0, M, K), sparc.msg_vector_2_bin_arr(b1, M, K)
        nbit = int(round(sparc_sim.calc_ber(bits0, bits1) * bits0.size))
        rows.append([1, nbit, int(nbit > 0), int(tf[b]), nsec, nloc, nval])
    return np.array(rows, dtype=np.int64)


def test_encode_device_2_17():
    cp, W, n, op = _design("cbig17", 0)
    K, B = K_of(cp), 4
    rng = np.random.default_rng(17)
    idx = rng.integers(0, op.M, (B, op.L)).astype(np.int32)
    sym = rng.integers(0, K, (B, op.L)).astype(np.int32)
    ref = op.Ab(np.stack([_msg(idx[b], sym[b], op.M, K) for b in range(B)]))
    d_idx, d_sym = _up(idx, np.int32), _up(sym, np.int32)
    d_x = _native.DeviceBuffer(B * op.n * 16)
    c = sparc._interleaved(sparc.psk_constel(K))
    _native.check(_native.lib().sg_camp_encode_device(op.plan(), K, _native.ptr(c), d_idx.ptr, d_sym.ptr, B, d_x.ptr,
                                                      None))
    x = _down(d_x, (B, op.n), np.complex128)
    err = np.max(np.abs(x - ref)) / np.max(np.abs(ref))
    print("cbig17 encode_device rel err", err)
    assert err < 1e-12


def test_trial_2_17():
    """CSparcTrial on one block of B = 4: the seven counters equal those of its
    own generated batch decoded and counted through the host entry points."""
    cp, W, n, op = _design("cbig17", 0)
    K, t_max, block = K_of(cp), CASES["cbig17"][2]['t_max'], 4
    args = (op, K, [AWGN_VAR], t_max)
    trial = montecarlo.CSparcTrial(*args, seed=3)
    d_ti, d_ts, d_y = trial.generate(0, 0, 1, block)
    ti, ts = _down(d_ti, (block, op.L), np.int32), _down(d_ts, (block, op.L), np.int32)
    Y = _down(d_y, (block, op.n), np.complex128)
    mi, ms, tf, _, _ = sparc.camp_decode_batch(Y, op, AWGN_VAR, t_max, trial.rtol, trial.phi, K, ti, ts)
    rows = _host_counts(ti, ts, mi, ms, tf, op.L, op.M, K)
    print("cbig17 trial host counters", rows.sum(axis=0))
    tot = montecarlo.CSparcTrial(*args, seed=3)(0, 0, 1, block)
    assert tot.dtype == np.int64 and np.array_equal(tot, rows.sum(axis=0))
