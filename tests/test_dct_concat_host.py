"""CPU tests of the DCT-design concatenated decoder's boundary: the new C-ABI
symbols, their refusal without a GPU, the sweep's `design` switch, and the
oracle composition (tests/dct_concat_ref.py) that the GPU tests measure
against."""
import inspect
import os
import re

import numpy as np
import pytest

import dct_concat_ref as ref
from ldpc_sparc_amd import _native, montecarlo, sparc_new

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ldpc_sparc_amd.h")


def _header_arity(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,arity", [("sg_amp_llr_device", 8), ("sg_amp_llr", 6)])
def test_symbols_declared_bound_and_exported(name, arity):
    assert _header_arity(name) == arity
    bound = {n: (r, a) for n, r, a in _native.SIGNATURES}
    assert name in bound and len(bound[name][1]) == arity
    assert hasattr(_native.lib(), name)


def test_bad_arg_is_the_invalid_code():
    src = open(HEADER).read()
    assert re.search(r"SG_ERR_BAD_ARG\s*=\s*SG_ERR_INVALID", src)
    assert _native.SG_ERR_BAD_ARG == _native.SG_ERR_INVALID == -2
    assert _native.SG_ERR_NO_DEVICE == -3 and _native.SG_ERR_UNSUPPORTED == -6


def test_llr_without_a_device():
    if _native.device_count() > 0:
        pytest.skip("GPU present")
    lib = _native.lib()
    out = np.zeros(8)
    assert lib.sg_amp_llr_device(None, 1, 0, 1, 8, 0, _native.ptr(out), None) == _native.SG_ERR_NO_DEVICE
    assert b"no GPU" in lib.sg_last_error()
    assert lib.sg_amp_llr(None, 1, 0, 1, 0, _native.ptr(out)) == _native.SG_ERR_NO_DEVICE
    assert np.all(out == 0)


def test_sweep_rejects_an_unknown_design():
    with pytest.raises(ValueError, match="design"):
        montecarlo.concat_ber_sweep(112, 64, 672, 15.0, 4, 1, [2.0], codewords=16, block=16,
                                    ldpc=("802.11n", "1/2", 27), design="nonsense")


def test_sweep_design_default_and_tags():
    sig = inspect.signature(montecarlo.concat_ber_sweep)
    assert sig.parameters["design"].default == "dense"
    assert montecarlo.concat_checkpoint_tag(1024, 512, 9216) == "concat_L1024_M512_n9216"
    assert montecarlo.concat_checkpoint_tag(1024, 512, 9216, "dct") == "concat_dct_L1024_M512_n9216"


def test_dct_sweep_checkpoints_apart_from_dense(tmp_path):
    """A DCT sweep (rehearsed with a CPU trial) writes concat_dct_* checkpoints
    with "design": "dct"; under the dense tag they do not resume."""
    import json
    calls = []

    def trial(point, first, nb, block):
        calls.append((point, first, nb))
        return np.array([nb * block, 3, 1, 1, 2], dtype=np.int64)
    kw = dict(codewords=32, block=16, ldpc=("802.11n", "1/2", 27), checkpoint_dir=str(tmp_path), trial=trial)
    out = montecarlo.concat_ber_sweep(112, 64, 672, 15.0, 4, 1, [2.0], design="dct", **kw)
    assert out[0]["codewords"] == 32 and calls
    path = tmp_path / "concat_dct_L112_M64_n672_pt0.json"
    assert json.load(open(path))["params"]["design"] == "dct"
    os.rename(path, tmp_path / "concat_L112_M64_n672_pt0.json")
    with pytest.raises(ValueError, match="parameters"):
        montecarlo.concat_ber_sweep(112, 64, 672, 15.0, 4, 1, [2.0], **kw)
    # and a dense checkpoint keeps the parameters it always had (no "design" key)
    os.remove(tmp_path / "concat_L112_M64_n672_pt0.json")
    montecarlo.concat_ber_sweep(112, 64, 672, 15.0, 4, 1, [2.0], **kw)
    assert "design" not in json.load(open(tmp_path / "concat_L112_M64_n672_pt0.json"))["params"]


def _bp_probs_loops(beta, L, M, snp):
    """beta_estimate_to_bp_probs as the reference defines it (sparc_new.py
    :1118-1138): per section and bit k, the sum of beta / sqrt(n P_l) over the
    indices whose k-th MSB-first bit is 0 (S_k_mapping, :1140-1160)."""
    S = sparc_new.S_k_mapping(M)
    b = np.asarray(beta).reshape(L, M)
    return np.array([[sum(b[l][j] / snp for j in S[k]) for k in range(len(S))] for l in range(L)]).reshape(-1)


def test_oracle_composition_reproduces_the_glue():
    M, L = 16, 3
    beta = np.zeros((L, M))
    beta[0, 11] = 1.0                      # one-hot: 11 = 1011b -> P(bit = 0) = (0, 1, 0, 0)
    rng = np.random.default_rng(0)
    soft = rng.random(M) ** 4
    beta[1] = soft / soft.sum()            # a soft section
    beta[2] = 1.0 / M                      # uniform: every bit 1/2
    got = ref.bit_probs(beta.reshape(-1), L, M)
    np.testing.assert_allclose(got, _bp_probs_loops(beta, L, M, 1.0), rtol=0, atol=1e-15)
    assert got[:4].tolist() == [0.0, 1.0, 0.0, 0.0]
    np.testing.assert_allclose(got[8:], 0.5, atol=1e-15)
    assert np.all((got[4:8] > 0) & (got[4:8] < 1))
    # a section range, and the clip / log of ldpc_bp (sparc_new.py:1167-1169)
    assert np.array_equal(ref.bit_probs(beta.reshape(-1), L, M, 1, 2), got[4:])
    llr = ref.llr_of_probs(got)
    hi = 1 - 1e-15  # (not 1 - 1e-15 exactly in double: the two clipped LLRs are not each other's negative)
    assert llr[0] == np.log(1e-15) - np.log(1 - 1e-15) and llr[1] == np.log(hi) - np.log(1 - hi)
    assert 34.4 < llr[1] < 34.7 and -34.6 < llr[0] < -34.5
    np.testing.assert_allclose(llr[4:8], np.log(got[4:8]) - np.log(1 - got[4:8]), rtol=1e-15)
    # the message-vector scale of the dense design divides out
    np.testing.assert_allclose(_bp_probs_loops(7.0 * beta, L, M, 7.0), got, rtol=0, atol=1e-15)


def test_oracle_composition_decodes_a_clean_codeword(oracle_built):
    """End to end on the CPU at the small geometry: AMP soft output -> LLR ->
    sumprod2 returns the drawn user bits at awgn_var = 1."""
    from ldpc_sparc_amd.ldpc import code
    from oracle import sparc_ref
    g = ref.SMALL
    L, M, n, Lu = g["L"], g["M"], g["n"], g["L_unp"]
    c = code(*g["ldpc"])
    rng = np.random.default_rng(5)
    unp, info = rng.integers(0, 2, Lu * 6), rng.integers(0, 2, (1, c.K))
    bits = np.concatenate([unp, c.encode_batch(info)[0]]).reshape(L, 6)
    idx = bits @ (1 << np.arange(6)[::-1])
    W, o0, o1 = ref.flat_design(L, M, n, g["P"], 2)
    Ab, Az = sparc_ref.dct_operators(W, L, M, n, o0, o1)
    beta0 = np.zeros(L * M)
    beta0[np.arange(L) * M + idx] = 1
    y = Ab(beta0) + rng.standard_normal(n)
    beta, mp, tf = ref.amp_soft(y, W, L, M, n, 1.0, 25, Ab, Az, beta0)
    assert 2 <= tf < 24
    got = ref.decode_user_bits(beta, mp, L, M, Lu, c)
    assert np.array_equal(got, ref.user_bits_truth(idx, info[0], Lu, 6))
