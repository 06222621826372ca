"""CPU tests of the host side of complex / K-PSK SPARCs: PSK helpers, message
vector formats, orderings, encoder bookkeeping, error statistics, and the
no-GPU behaviour of the complex entry points."""
import ctypes as ct

import numpy as np
import pytest

from csparc_cases import AWGN_VAR, CSPARC_CASES, PSK_K, all_seeds, code_params, design, golden, seed_of
from ldpc_sparc_amd import _native, sparc, sparc_sim


def _K(cp):
    return cp['K'] if cp.get('modulated') else 1


def test_gray_code():
    n = np.arange(64)
    g = sparc.bin2gray(n)
    assert np.array_equal(sparc.gray2bin(g), n)
    assert sparc.bin2gray(5) == 7 and sparc.gray2bin(7) == 5
    d = g[1:] ^ g[:-1]
    assert np.all((d & (d - 1)) == 0) and np.all(d > 0)  # neighbours differ in one bit


def test_psk_constellations():
    c2, c4 = sparc.psk_constel(2), sparc.psk_constel(4)
    assert not np.iscomplexobj(c2) and np.array_equal(c2, [1, -1])
    assert c4.dtype == np.complex128 and np.array_equal(c4, [1, 1j, -1, -1j])
    for K in (8, 16, 64):
        th = 2 * np.pi * np.arange(K) / K
        assert np.array_equal(sparc.psk_constel(K), np.cos(th) + 1j * np.sin(th))
    with pytest.raises(AssertionError):
        sparc.psk_constel(6)


@pytest.mark.parametrize("K", PSK_K)
def test_psk_mod_demod_golden(K):
    g = golden()
    bits = g[f"psk{K}_bits"]
    sym = sparc.psk_mod(bits, K)
    assert sym.dtype == g[f"psk{K}_sym"].dtype and np.array_equal(sym, g[f"psk{K}_sym"])
    dem = sparc.psk_demod(sym, K)
    assert dem.dtype == bool and np.array_equal(dem, g[f"psk{K}_demod"]) and np.array_equal(dem, bits)
    logK = int(np.log2(K))
    one = sparc.psk_mod(bits[:logK], K)  # a single symbol, as bin_arr_2_msg_vector uses it
    assert np.ndim(one) == 0 and one == sym[0]
    assert np.array_equal(sparc.psk_demod(np.asarray(one), K), bits[:logK])


@pytest.mark.parametrize("K", PSK_K)
def test_rnd_msg_vector_golden(K):
    ref = golden()[f"rnd{K}_msg"]
    mv = sparc.rnd_msg_vector(12, 8, [K, 3], K)
    assert mv.dtype == ref.dtype and np.array_equal(mv, ref)
    assert mv.dtype == (np.float64 if K == 2 else np.complex128)


@pytest.mark.parametrize("K,M", [(1, 8), (2, 4), (4, 32), (8, 16), (16, 2), (64, 8)])
def test_bits_msg_vector_round_trip(K, M):
    L = 10
    logM, logK = int(np.log2(M)), int(np.log2(K))
    bits = sparc.rnd_bin_arr(L * (logM + logK), [K, M])
    mv = sparc.bin_arr_2_msg_vector(bits, M, K)
    assert mv.size == L * M
    assert mv.dtype == (np.float64 if K <= 2 else np.complex128)
    sec = bits.reshape(L, logM + logK)  # location bits first
    loc = sec[:, :logM].astype(int) @ (1 << np.arange(logM)[::-1])
    assert np.array_equal(np.nonzero(mv.reshape(L, M))[1], loc)
    if K > 1:
        assert np.array_equal(mv.reshape(L, M)[np.arange(L), loc], sparc.psk_mod(sec[:, logM:].ravel(), K))
    assert np.array_equal(sparc.msg_vector_2_bin_arr(mv, M, K), bits)


def test_generate_ordering_csparc_golden():
    g = golden()
    W = sparc.sc_basic(np.array(15.0), 2, 4)
    o0, o1 = sparc.generate_ordering(W, 9, 8 * 16 // 4, [4, 44], csparc=True)
    assert o0.dtype == np.uint32 and o0.shape == W.shape + (9,) and o1.shape == W.shape + (32,)
    nz = [(r, c) for r in range(W.shape[0]) for c in range(W.shape[1]) if W[r, c] != 0]
    assert np.array_equal(np.stack([o0[b] for b in nz]), g["ord2d_order0"])
    assert np.array_equal(np.stack([o1[b] for b in nz]), g["ord2d_order1"])
    w = 64  # max(9 + 2, 32 + 2) -> 64; bins 0 and w/2 are never drawn
    assert sparc.transform_size(9, 32, True) == w
    assert not np.isin([0, w // 2], np.concatenate([o0[nz[0]], o1[nz[0]]])).any()
    assert sparc.transform_size(30, 62, True) == 64 and sparc.transform_size(30, 63, True) == 128
    assert sparc.transform_size(30, 63) == 64


@pytest.mark.parametrize("name,cp", [(c[0], code_params(c[1])) for c in CSPARC_CASES])
def test_orders_of_golden_designs(name, cp):
    g = golden()
    W, L, M, n, o0, o1 = design(g, name, cp)
    Lr = W.shape[0] if W.ndim == 2 else 1
    Lc = W.shape[-1] if W.ndim >= 1 else 1
    m0, m1 = sparc.generate_ordering(W, n // Lr, L * M // Lc, seed_of(0), csparc=True)
    assert np.array_equal(m0, o0) and np.array_equal(m1, o1)


@pytest.mark.parametrize("name,cp,dp,si", list(all_seeds()))
def test_encode_bits_and_n(name, cp, dp, si, monkeypatch):
    """sparc_encode's host side (bits, message vector, n, R_actual) on the golden
    seeds; the GPU operator is replaced by a recorder."""
    g, key = golden(), f"{name}_s{si}"
    seen = {}

    def fake_transforms(W, L, M, n, rand_seed, csparc=False):
        seen.update(n=n, csparc=csparc, seed=rand_seed)
        return (lambda x: np.zeros(n, dtype=complex)), (lambda y: np.zeros(L * M, dtype=complex))
    monkeypatch.setattr(sparc, "sparc_transforms", fake_transforms)
    cp = dict(cp)
    bits, beta0, x, Ab, Az = sparc.sparc_encode(cp, AWGN_VAR, seed_of(si))
    assert np.array_equal(bits, g[key + "_bits"])
    assert cp['n'] == int(g[key + "_n"]) == seen['n'] and seen['csparc'] is True
    assert cp['R_actual'] == bits.size / cp['n']
    K = _K(cp)
    assert beta0.dtype == (np.float64 if K <= 2 else np.complex128)
    assert np.array_equal(sparc.msg_vector_2_bin_arr(beta0, cp['M'], K), bits)


def test_calc_ler_ver():
    c = sparc.psk_constel(4)
    L, M = 4, 4
    b0 = np.zeros((L, M), dtype=complex)
    b = np.zeros((L, M), dtype=complex)
    b0[0, 1], b[0, 1] = c[1], c[1]   # correct
    b0[1, 2], b[1, 3] = c[0], c[0]   # location error only
    b0[2, 0], b[2, 0] = c[2], c[3]   # value error only
    b0[3, 3], b[3, 0] = c[1], c[2]   # both
    rates, locs, nums = sparc_sim.calc_ler_ver(b0.ravel(), b.ravel(), L, 4)
    assert rates == (0.5, 0.5, 0.75) and nums == (2, 2, 3)
    assert [a.tolist() for a in locs] == [[1, 3], [2, 3], [1, 2, 3]]
    with pytest.raises(AssertionError):
        sparc_sim.calc_ler_ver(b0.ravel(), b.ravel().real, L, 4)


def test_scope_limits():
    with pytest.raises(NotImplementedError, match="real K=2"):
        sparc.sparc_encode({'P': 15.0, 'R': 1.0, 'L': 8, 'M': 8, 'modulated': True, 'K': 2}, 1.0, [1, 2])
    with pytest.raises(NotImplementedError, match="K > 64"):
        sparc.sparc_encode({'P': 15.0, 'R': 1.0, 'L': 8, 'M': 8, 'complex': True, 'modulated': True, 'K': 128},
                           1.0, [1, 2])
    W, L, M, n, o0, o1 = design(golden(), "creg", code_params(CSPARC_CASES[0][1]))
    op = sparc.ComplexDesignOperator(W, L, M, n, o0, o1)
    assert sparc.operator_of(op.Ab, op.Az) is op and op.w == 8192
    cp = code_params(CSPARC_CASES[0][1])
    sparc.check_code_params(cp)
    cp['n'] = n
    with pytest.raises(NotImplementedError, match="double precision"):
        sparc.sparc_amp(np.zeros(n, dtype=complex), cp, {'t_max': 5, 'rtol': 1e-6, 'phi_est_method': 1,
                                                         'precision': 'f32'}, 1.0, [1, 2], None, op.Ab, op.Az)


def test_complex_entry_points_need_a_gpu():
    if _native.device_count() > 0:
        pytest.skip("GPU present")
    lib = _native.lib()
    h = ct.c_void_p()
    W = np.array([15.0])
    o = np.arange(1, 9, dtype=np.uint32)
    buf = np.zeros(64)
    i32 = np.zeros(16, dtype=np.int32)
    p = _native.ptr
    assert lib.sg_camp_plan_create(0, p(W), 1, 1, 2, 4, 8, p(o), p(o), ct.byref(h)) == -3  # SG_ERR_NO_DEVICE
    assert b"no GPU" in lib.sg_last_error()
    assert lib.sg_camp_apply(None, 0, p(buf), 1, p(buf)) == -3
    assert lib.sg_camp_decode(None, p(buf), 1, 1, None, None, None, 1.0, 5, 1e-6, 1, p(i32), p(i32), p(i32),
                              p(buf), p(buf)) == -3
    assert lib.sg_section_mmse_psk(p(buf), 2, 4, 1, None, 0, p(np.zeros(16))) == -3
    assert lib.sg_section_map_psk(p(buf), 2, 4, 1, None, 0, p(i32), p(i32)) == -3
    with pytest.raises(_native.NativeError, match="no GPU"):
        sparc.msg_vector_mmse_estimator(np.zeros(8, dtype=complex), 1.0, 4, 4)
    with pytest.raises(_native.NativeError, match="no GPU"):
        sparc_sim.sparc_sim(code_params({'R': 2.0, 'L': 8, 'M': 8, 'modulated': True, 'K': 4}), {'t_max': 5}, 1.0,
                            [1, 2])
