"""Device-resident Monte-Carlo campaign of the complex / K-PSK engine
(camp_campaign.hip, capi_camp.cpp, montecarlo.CSparcTrial / csparc_ser_sweep)
against the package's own host functions, which tests/test_csparc_host.py and
tests/test_csparc_gpu.py pin to the reference.

Bars: everything discrete (section indices, MAP decisions, counters, rows,
t_final) and the decoder's nmse / psi are exactly equal -- the device decode
runs the same kernels in the same order as the host-fed one; the encoder's x
is within 1e-12 of op.Ab, relative to max |x| (the operator bar of
tests/test_csparc_gpu.py).
"""
import ctypes as ct
import functools

import numpy as np
import pytest

from csparc_cases import AWGN_VAR, CSPARC_CASES, code_params, design, golden
from ldpc_sparc_amd import _native, montecarlo, sparc, sparc_sim

pytestmark = pytest.mark.gpu

CASES = {c[0]: c for c in CSPARC_CASES}
NOISY_VAR = 4.0  # log2(1 + P / 4) = 2.25 bits, below the golden cases' rates: decoding errors are certain


@functools.lru_cache(maxsize=None)
def _op(name):
    """(operator, K, t_max) of a golden case's seed-0 design."""
    cp = code_params(CASES[name][1])
    W, L, M, n, o0, o1 = design(golden(), name, cp)
    K = cp['K'] if cp.get('modulated') else 1
    return sparc.ComplexDesignOperator(W, L, M, n, o0, o1), K, CASES[name][2]['t_max']


def _up(a, dtype):
    return _native.DeviceBuffer.from_array(np.ascontiguousarray(a, dtype=dtype))


def _down(buf, shape, dtype):
    _native.synchronize()
    return buf.download(np.zeros(shape, dtype=dtype))


def _constel(K):
    return sparc._interleaved(sparc.psk_constel(K)) if K != 1 else None


def _random_sections(rng, B, L, M, K):
    return rng.integers(0, M, (B, L)).astype(np.int32), rng.integers(0, K, (B, L)).astype(np.int32)


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


# ------------------------------------------------------------------ 1. bits -> (idx, sym)
@pytest.mark.parametrize("M,K", [(32, 1), (32, 2), (16, 4), (8, 16), (4, 64)])
def test_bits_to_psk_sections(M, K):
    B, L = 3, 16
    logM, logK = int(np.log2(M)), int(np.log2(K))
    bits = np.random.default_rng(M * 100 + K).integers(0, 2, (B, L * (logM + logK))).astype(np.uint8)
    ref = [sparc._msg_vector_indices(sparc.bin_arr_2_msg_vector(bits[b].astype(bool), M, K), M, K) for b in range(B)]
    d_bits = _up(bits, np.uint8)
    d_idx, d_sym = _native.DeviceBuffer(B * L * 4), _native.DeviceBuffer(B * L * 4)
    d_sym.upload(np.full((B, L), -1, np.int32))
    _native.check(_native.lib().sg_bits_to_psk_sections_device(d_bits.ptr, B, L, logM, logK, d_idx.ptr, d_sym.ptr, None))
    assert np.array_equal(_down(d_idx, (B, L), np.int32), np.stack([r[0] for r in ref]))
    assert np.array_equal(_down(d_sym, (B, L), np.int32), np.stack([r[1] for r in ref]))
    if K == 1:  # d_sym may be NULL
        d_idx.zero()
        _native.check(_native.lib().sg_bits_to_psk_sections_device(d_bits.ptr, B, L, logM, 0, d_idx.ptr, None, None))
        assert np.array_equal(_down(d_idx, (B, L), np.int32), np.stack([r[0] for r in ref]))


# ------------------------------------------------------------------ 2. encode
@pytest.mark.parametrize("name", ["creg", "cpsk4", "cpsk16", "cpa4", "csc4"])
def test_encode_device(name):
    op, K, _ = _op(name)
    B = 3
    idx, sym = _random_sections(np.random.default_rng(len(name) + K), B, op.L, op.M, K)
    ref = op.Ab(np.stack([_msg(idx[b], sym[b], op.M, K) for b in range(B)]))
    d_idx, d_sym = _up(idx, np.int32), _up(sym, np.int32)
    d_x = _native.DeviceBuffer(B * op.n * 16)
    _native.check(_native.lib().sg_camp_encode_device(op.plan(), K, _native.ptr(_constel(K)), d_idx.ptr,
                                                      d_sym.ptr if K != 1 else None, B, d_x.ptr, None))
    x = _down(d_x, (B, op.n), np.complex128)
    err = np.max(np.abs(x - ref)) / np.max(np.abs(ref))
    print(name, "encode rel err", err)
    assert err < 1e-12


# ------------------------------------------------------------------ 3. decode_device == host decode
@pytest.mark.parametrize("name", ["cpsk4", "creg", "csc4"])
def test_decode_device_equals_host_decode(name):
    op, K, t_max = _op(name)
    B, L, n, Lc = 5, op.L, op.n, op.Lc
    rng = np.random.RandomState(17)
    ti, ts = _random_sections(np.random.default_rng(5), B, L, op.M, K)
    X = op.Ab(np.stack([_msg(ti[b], ts[b], op.M, K) for b in range(B)]))
    Y = X + np.sqrt(AWGN_VAR / 2) * (rng.randn(B, n) + 1j * rng.randn(B, n))
    host = sparc.camp_decode_batch(Y, op, AWGN_VAR, t_max, 1e-6, 1, K, ti, ts)
    lib, c = _native.lib(), _constel(K)
    d_y, d_ti, d_ts = _up(Y, np.complex128), _up(ti, np.int32), _up(ts, np.int32)
    d_mi, d_ms, d_tf = (_native.DeviceBuffer(B * L * 4), _native.DeviceBuffer(B * L * 4), _native.DeviceBuffer(B * 4))
    d_nm, d_psi = _native.DeviceBuffer(B * t_max * Lc * 8), _native.DeviceBuffer(B * Lc * 8)
    _native.check(lib.sg_camp_decode_device(op.plan(), d_y.ptr, B, K, _native.ptr(c), d_ti.ptr, d_ts.ptr, AWGN_VAR,
                                            t_max, 1e-6, 1, d_mi.ptr, d_ms.ptr, d_tf.ptr, d_nm.ptr, d_psi.ptr, None))
    dev = (_down(d_mi, (B, L), np.int32), _down(d_ms, (B, L), np.int32), _down(d_tf, (B,), np.int32),
           _down(d_nm, (B, t_max, Lc), np.float64), _down(d_psi, (B, Lc), np.float64))
    for what, h, d in zip(("map_idx", "map_sym", "t_final", "nmse", "psi"), host, dev):
        assert np.array_equal(h, d), what
    assert np.array_equal(_down(d_y, (B, n), np.complex128), Y)  # the received words are only read
    # every optional output NULL except the MAP locations (and no true indices)
    d_mi.zero()
    _native.check(lib.sg_camp_decode_device(op.plan(), d_y.ptr, B, K, _native.ptr(c), None, None, AWGN_VAR, t_max,
                                            1e-6, 1, d_mi.ptr, None, None, None, None, None))
    assert np.array_equal(_down(d_mi, (B, L), np.int32), host[0])


# ------------------------------------------------------------------ 4. counters
def _count_case(logM, logK):
    """True and MAP sections of four codewords: no error; location-only errors;
    value-only errors (none possible for K = 1); both, one section carrying both."""
    B, L, M, K = 4, 16, 1 << logM, 1 << logK
    ti, ts = _random_sections(np.random.default_rng(logM * 10 + logK), B, L, M, K)
    mi, ms = ti.copy(), ts.copy()
    for l in (0, 5, 15):
        mi[1, l] = (ti[1, l] + 1 + l % 3) % M
    if K > 1:
        for l in (2, 3, 9, 14):
            ms[2, l] = (ts[2, l] + 1 + l % 3) % K
        ms[3, 7] = (ts[3, 7] + K // 2) % K
        ms[3, 11] = (ts[3, 11] + 1) % K
    mi[3, 7] = ti[3, 7] ^ (M - 1)
    mi[3, 1] = (ti[3, 1] + 3) % M
    tf = np.array([3, 25, 7, 11], dtype=np.int32)
    return B, L, M, K, ti, ts, mi, ms, tf


@pytest.mark.parametrize("logM,logK", [(5, 0), (5, 2), (3, 4)])
def test_count_errors_device(logM, logK):
    B, L, M, K, ti, ts, mi, ms, tf = _count_case(logM, logK)
    rows = _host_counts(ti, ts, mi, ms, tf, L, M, K)
    assert rows[0, 1] == 0 and rows[1, 5] == 3 and rows[1, 6] == 0 and rows[3, 4] >= 2  # the cases are what they claim
    if K > 1:
        assert rows[2, 5] == 0 and rows[2, 6] == 4 and rows[3, 4] == 3 and rows[3, 5] == 2 and rows[3, 6] == 2
    want = np.array([rows[:, 4].sum(), rows[:, 5].sum(), rows[:, 6].sum(), rows[:, 1].sum(), rows[:, 2].sum(),
                     rows[:, 3].sum()], dtype=np.int64)
    d = [_up(a, np.int32) for a in (mi, ms, ti, ts, tf)]
    sym_sets = [(d[1].ptr, d[3].ptr)] + ([(None, None)] if K == 1 else [])
    for p_ms, p_ts in sym_sets:
        d_cnt, d_rows = _native.DeviceBuffer(6 * 8), _native.DeviceBuffer(B * 4 * 4)
        d_cnt.zero()
        for rep in (1, 2):  # the counts accumulate
            d_rows.zero()
            _native.check(_native.lib().sg_camp_count_errors_device(d[0].ptr, p_ms, d[2].ptr, p_ts, d[4].ptr, B, L, logM,
                                                                    logK, d_cnt.ptr, d_rows.ptr, None))
            assert np.array_equal(_down(d_cnt, (6,), np.int64), rep * want)
            assert np.array_equal(_down(d_rows, (B, 4), np.int32), rows[:, [1, 4, 5, 6]])
        _native.check(_native.lib().sg_camp_count_errors_device(d[0].ptr, p_ms, d[2].ptr, p_ts, d[4].ptr, B, L, logM,
                                                                logK, d_cnt.ptr, None, None))  # d_rows may be NULL
        assert np.array_equal(_down(d_cnt, (6,), np.int64), 3 * want)


# ------------------------------------------------------------------ 5. trial end to end
def _host_trial(trial, point, first_block, n_blocks, block):
    """CSparcTrial's rows from its own generated batch, decoded and counted through the host entry points."""
    op, K = trial.op, trial.K
    B = n_blocks * block
    d_ti, d_ts, d_y = trial.generate(point, first_block, n_blocks, block)
    ti, ts = _down(d_ti, (B, op.L), np.int32), _down(d_ts, (B, op.L), np.int32)
    Y = _down(d_y, (B, op.n), np.complex128)
    mi, ms, tf, _, _ = sparc.camp_decode_batch(Y, op, trial.vars[point], trial.t_max, trial.rtol, trial.phi, K, ti, ts)
    return _host_counts(ti, ts, mi, ms, tf, op.L, op.M, K)


@pytest.mark.parametrize("name", ["cpsk4", "creg"])
def test_trial_end_to_end(name):
    op, K, t_max = _op(name)
    args = (op, K, [AWGN_VAR, NOISY_VAR], t_max)
    block, n_blocks = 8, 2
    for point in (0, 1):
        rows = _host_trial(montecarlo.CSparcTrial(*args, seed=3), point, 0, n_blocks, block)
        print(name, "point", point, "host counters", rows.sum(axis=0))
        tot = montecarlo.CSparcTrial(*args, seed=3)(point, 0, n_blocks, block)
        assert tot.dtype == np.int64 and np.array_equal(tot, rows.sum(axis=0))
        per = montecarlo.CSparcTrial(*args, seed=3, per_unit=True)(point, 0, n_blocks, block)
        assert per.dtype == np.int64 and np.array_equal(per, rows)
    # the noise is complex AWGN of the point's variance, drawn per (point, block)
    trial = montecarlo.CSparcTrial(*args, seed=3)
    d_ti, d_ts, d_y = trial.generate(0, 0, n_blocks, block)
    B = n_blocks * block
    ti, ts = _down(d_ti, (B, op.L), np.int32), _down(d_ts, (B, op.L), np.int32)
    noise = _down(d_y, (B, op.n), np.complex128) - op.Ab(np.stack([_msg(ti[b], ts[b], op.M, K) for b in range(B)]))
    assert abs(np.mean(np.abs(noise) ** 2) / AWGN_VAR - 1) < 0.1  # B n >= 2560 samples: 5 sigma is 0.1
    assert not np.array_equal(ti[:block], ti[block:])


# ------------------------------------------------------------------ 6. batching and rank independence
def test_batching_and_rank_independence():
    op, K, t_max = _op("cpsk4")
    args, block = (op, K, [NOISY_VAR], t_max), 8
    trial = montecarlo.CSparcTrial(*args, seed=1)
    per = montecarlo.CSparcTrial(*args, seed=1, per_unit=True)
    whole = trial(0, 0, 4, block)
    assert whole[0] == 4 * block and whole[1] > 0, whole  # errors to count at this noise level
    assert np.array_equal(whole, trial(0, 0, 1, block) + trial(0, 1, 2, block) + trial(0, 3, 1, block))
    rows = per(0, 0, 4, block)
    assert np.array_equal(rows, np.concatenate([per(0, 0, 1, block), per(0, 1, 2, block), per(0, 3, 1, block)]))
    assert np.array_equal(rows.sum(axis=0), whole)
    for t in (trial, per):
        run = functools.partial(montecarlo.run_point, t, 0, block=block, blocks_per_round=4, agg=montecarlo.Aggregator())
        one = run(rank=0, world=1)
        assert np.array_equal(one, whole)
        assert np.array_equal(run(rank=0, world=2) + run(rank=1, world=2), one)


# ------------------------------------------------------------------ 7. sweep
def test_ser_sweep_rates_and_resume(tmp_path):
    cp = code_params(CASES["cpsk4"][1])
    dp = {'t_max': 25}
    kw = dict(codewords=16, block=8, design_seed=4, seed=2)
    out = montecarlo.csparc_ser_sweep(cp, dp, [AWGN_VAR, NOISY_VAR], **kw)
    L, bits = cp['L'], cp['L'] * int(np.log2(cp['M'] * cp['K']))
    assert [o["awgn_var"] for o in out] == [AWGN_VAR, NOISY_VAR]
    for o in out:
        c = o["counts"]
        assert len(c) == 7 and c[0] == o["codewords"] == 16
        assert o["ber"] == c[1] / (16 * bits) and o["cer"] == c[2] / 16 and o["t_final_mean"] == c[3] / 16
        assert o["ser"] == c[4] / (16 * L) and o["ler"] == c[5] / (16 * L) and o["ver"] == c[6] / (16 * L)
        assert max(c[5], c[6]) <= c[4] <= c[5] + c[6]
    assert out[1]["counts"][1] > 0, out[1]
    part = montecarlo.csparc_ser_sweep(cp, dp, [AWGN_VAR, NOISY_VAR], checkpoint_dir=str(tmp_path), max_rounds=1, **kw)
    assert [o["codewords"] for o in part] == [8, 8]
    resumed = montecarlo.csparc_ser_sweep(cp, dp, [AWGN_VAR, NOISY_VAR], checkpoint_dir=str(tmp_path), **kw)
    assert resumed == out


def test_encode_and_decode_argument_checks():
    op, K, t_max = _op("cpsk4")
    lib = _native.lib()
    buf = _native.DeviceBuffer(1024)
    assert lib.sg_camp_encode_device(op.plan(), 128, _native.ptr(np.zeros(256)), buf.ptr, buf.ptr, 1, buf.ptr,
                                     None) == -6  # SG_ERR_UNSUPPORTED
    assert lib.sg_camp_encode_device(op.plan(), 4, None, buf.ptr, buf.ptr, 1, buf.ptr, None) == -2  # no constellation
    assert lib.sg_camp_decode_device(op.plan(), buf.ptr, 1, 1, None, None, None, 1.0, 1, 1e-6, 1, None, None, None, None,
                                     None, None) == -2  # t_max
    assert lib.sg_bits_to_psk_sections_device(buf.ptr, 1, 4, 3, 2, buf.ptr, None, None) == -2  # logK > 0 without d_sym
    h = ct.c_void_p()
    u = np.zeros((4, 8))
    _native.check(lib.sg_se_samples_create(_native.ptr(u), 4, 8, ct.byref(h)))
    E, tau = np.zeros(1), np.ones(1)
    assert lib.sg_se_expectation(h, 4, _native.ptr(tau), 1, _native.ptr(E)) == -2  # K = 4 on real samples
    lib.sg_se_samples_destroy(h)
