"""CPU tests of the real K = 2 (BPSK) modulated SPARC path: the restatement
tests/amp_bpsk_ref.py against the reference's fixture
(tests/golden/bpsk_golden.npz, written by tests/golden/make_golden_bpsk.py),
the section-word packing, the opt-in switch of the drop-in functions, and the
library's three entry points."""
import ctypes as ct

import numpy as np
import pytest

import amp_bpsk_ref as br
from bpsk_cases import AWGN_VAR, BPSK_CASES, IDS, all_seeds, code_params, design, golden, seed_of, true_words, words
from ldpc_sparc_amd import _native, sparc


def _design_of_seed(cp, n, seed):
    """(W, order0, order1) as sparc_transforms draws them for a seed (host only)."""
    tmp = dict(cp)
    tmp.update({'awgn_var': AWGN_VAR})
    W = sparc.create_base_matrix(**tmp)
    L, M = cp['L'], cp['M']
    Mr = n // W.shape[0] if W.ndim == 2 else n
    Mc = L * M // (W.shape[-1] if W.ndim else 1)
    o0, o1 = sparc.generate_ordering(W, Mr, Mc, seed)
    return W, o0, o1


@pytest.mark.parametrize("name,cp", [(c[0], code_params(c[1])) for c in BPSK_CASES])
def test_orders_of_seed_0_are_the_reference_s(name, cp):
    g = golden()
    W, L, M, n, o0, o1 = design(g, name, cp)
    cp = dict(cp)
    sparc.check_code_params(cp)
    W2, p0, p1 = _design_of_seed(cp, n, seed_of(0))
    assert np.array_equal(W, W2) and np.array_equal(o0, p0) and np.array_equal(o1, p1)


@pytest.mark.parametrize("name,cp,dp,si", list(all_seeds()), ids=IDS)
def test_restatement_matches_the_reference(name, cp, dp, si):
    g, key = golden(), f"{name}_s{si}"
    cp, dp = dict(cp), dict(dp)
    sparc.check_code_params(cp)
    sparc.check_decode_params(dp)
    L, M, n = cp['L'], cp['M'], int(g[key + "_n"])
    W, o0, o1 = _design_of_seed(cp, n, seed_of(si))
    Ab, Az = br.operators(W, L, M, n, o0, o1)
    tw = true_words(g[key + "_bits"], M)
    beta0 = br.beta_of_words(tw, M)
    assert np.array_equal(beta0, sparc.bin_arr_2_msg_vector(g[key + "_bits"], M, 2))
    np.testing.assert_allclose(Ab(beta0), g[key + "_x"], rtol=0, atol=1e-9)
    mw, tf, nmse, psi = br.amp_bpsk(g[key + "_y"], W, L, M, n, AWGN_VAR, dp['t_max'], Ab, Az, beta0, dp['rtol'],
                                    dp['phi_est_method'])
    print(key, "t_final", tf, "max |nmse - ref|", np.abs(nmse - g[key + "_nmse"]).max())
    assert tf == int(g[key + "_t_final"])
    assert np.array_equal(mw, words(g[key + "_map"], g[key + "_map_sym"]))
    np.testing.assert_allclose(nmse, g[key + "_nmse"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(psi, g[key + "_psi"], rtol=0, atol=1e-9)


def test_fixture_holds_wrong_decisions_and_sign_errors():
    g = golden()
    assert g["bhard_s0_sim_ver"] > 0 and g["bM2048_s2_sim_ser"] == 1.0 and int(g["bhard_s0_t_final"]) == 24
    mw = words(g["bhard_s0_map"], g["bhard_s0_map_sym"])
    assert np.any(mw != true_words(g["bhard_s0_bits"], 32))


@pytest.mark.parametrize("M", [2, 32, 2048])
def test_word_digits_are_the_section_bits(M):
    """The MSB-first digits of a word are the section's log2 M + 1 bits, both ways."""
    logM, L = int(np.log2(M)), 24
    bits = sparc.rnd_bin_arr(L * (logM + 1), [M, 4])
    beta0 = sparc.bin_arr_2_msg_vector(bits, M, 2)
    loc, sym = sparc._msg_vector_indices(beta0, M, 2)
    w = sparc.bpsk_words(loc, sym)
    assert w.dtype == np.int32 and np.array_equal(w, true_words(bits, M)) and np.all((w >= 0) & (w < 2 * M))
    assert np.array_equal(sparc._indices_to_bits(w, logM + 1), bits)
    back = sparc._msg_vector_from_indices(w >> 1, w & 1, M, 2)
    assert np.array_equal(back, beta0) and np.array_equal(back, br.beta_of_words(w, M))
    assert np.array_equal(sparc.msg_vector_2_bin_arr(back, M, 2), bits)
    assert set(np.unique(beta0)) == {-1.0, 0.0, 1.0}


def test_enable_real_psk_switch():
    cp = {'P': 15.0, 'R': 1.0, 'L': 8, 'M': 8, 'modulated': True, 'K': 2}
    assert sparc._real_psk is False  # off by default
    with pytest.raises(NotImplementedError, match="real K=2") as e:
        sparc.sparc_encode(dict(cp), 1.0, [1, 2])
    assert "enable_real_psk" in str(e.value)
    try:
        assert sparc.enable_real_psk() is False
        assert sparc.enable_real_psk() is True and sparc.enable_real_psk(True) is True  # idempotent
        sparc._check_family(2, False)
        assert sparc.enable_real_psk(False) is True
        with pytest.raises(NotImplementedError, match="real K=2"):
            sparc._check_family(2, False)
        assert sparc.enable_real_psk(False) is False
    finally:
        sparc.enable_real_psk(False)
    with pytest.raises(NotImplementedError, match="real K=2"):
        sparc.sparc_encode(dict(cp), 1.0, [1, 2])


def test_native_declares_the_entry_points():
    lib = _native.lib()
    names = {s[0] for s in _native.SIGNATURES}
    for name in ("sg_amp_decode_bpsk", "sg_amp_decode_bpsk_device", "sg_amp_encode_bpsk_device"):
        assert name in names and getattr(lib, name).restype is ct.c_int


def test_entry_points_need_a_gpu():
    if _native.device_count() > 0:
        pytest.skip("GPU present")
    lib, p = _native.lib(), _native.ptr
    buf, i32 = np.zeros(64), np.zeros(16, dtype=np.int32)
    assert lib.sg_amp_decode_bpsk(None, p(buf), 1, None, 1.0, 5, 1e-6, 1, p(i32), p(i32), p(buf), p(buf)) == -3
    assert b"no GPU" in lib.sg_last_error()
    assert lib.sg_amp_decode_bpsk_device(None, None, 1, None, 1.0, 5, 1e-6, 1, None, None, None, None, None) == -3
    assert lib.sg_amp_encode_bpsk_device(None, None, 1, None, None) == -3


def test_operator_refusals_need_no_gpu():
    W, L, M, n = np.array(15.0), 4, 8, 12
    o0, o1 = sparc.generate_ordering(W, n, L * M, 1, True)
    cop = sparc.ComplexDesignOperator(W, L, M, n, o0, o1)
    with pytest.raises(ValueError, match="real DesignOperator"):
        sparc.amp_decode_bpsk_batch(np.zeros((1, n)), cop, 1.0, 5)
    with pytest.raises(ValueError, match="K must be 1"):
        from ldpc_sparc_amd import montecarlo
        montecarlo.SparcTrial(cop, [1.0], K=4)
