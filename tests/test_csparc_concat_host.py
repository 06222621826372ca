"""CPU tests around the complex engine's soft output: the yardstick
(tests/csparc_concat_ref.py) is consistent with the restatements it extends,
the section word is the bit string of sparc.msg_vector_2_bin_arr, the new
C-ABI entry points are declared, bound, exported and refuse without a GPU, and
the pipeline's constructor and the sweep's `design="fft"` check their
arguments."""
import os
import re

import numpy as np
import pytest

import csparc_concat_ref as ref
import csparc_ref
from ldpc_sparc_amd import _native, montecarlo, sparc
from oracle import sparc_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ldpc_sparc_amd.h")


def _x(L, M, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    return scale * (rng.standard_normal(L * M) + 1j * rng.standard_normal(L * M))


# ---------------------------------------------------------------- the yardstick

def test_k1_equals_the_real_glue_of_its_own_beta():
    L, M = 5, 32
    x = _x(L, M, 0)
    beta = ref.joint_posterior(x, M, 1)[:, :, 0]
    np.testing.assert_allclose(beta.reshape(-1), csparc_ref.mmse(x, 2.0, M, 1), rtol=0, atol=1e-15)
    want = sparc_ref.beta_to_bit_probs(beta.reshape(-1), L, M, 1.0).reshape(L, -1)
    np.testing.assert_allclose(ref.bit_probs(x, M, 1), want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("K", [2, 4, 8, 16])
def test_conditional_mean_of_the_posterior_is_the_mmse_estimate(K):
    L, M = 4, 16
    s = _x(L, M, K)
    if K == 2:
        s = s.real.astype(complex)
    p = ref.joint_posterior(ref.x_of(s, 2.0), M, K)
    mean = (p * ref.constel(K)[None, None, :]).sum(axis=2).reshape(-1)
    np.testing.assert_allclose(mean, csparc_ref.mmse(s, 2.0, M, K), rtol=0, atol=1e-14)
    np.testing.assert_allclose(p.sum(axis=(1, 2)), 1.0, rtol=0, atol=1e-14)


def test_marginals_agree_with_a_direct_enumeration():
    """For every bit string of a section (M = 4, K = 4: 16 strings) its
    posterior is p(j, k) of the (j, k) that bin_arr_2_msg_vector maps it to."""
    M, K = 4, 4
    x = _x(1, M, 7, 1.0)
    p = ref.joint_posterior(x, M, K)[0]
    got = ref.bit_probs(x, M, K)[0]
    want = np.zeros(4)
    c = sparc.psk_constel(K)
    for word in range(16):
        bits = np.array([(word >> (3 - i)) & 1 for i in range(4)], dtype=bool)
        beta0 = sparc.bin_arr_2_msg_vector(bits, M, K)
        j = int(np.nonzero(beta0)[0][0])
        k = int(np.argmin(np.abs(c - beta0[j])))
        want[~bits] += p[j, k]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    # an observation on (j, k) = (2, 3) puts every bit on that pair's string
    x = np.zeros(M, dtype=complex)
    x[2] = 60 * c[3]
    bits = sparc.msg_vector_2_bin_arr(sparc._msg_vector_from_indices([2], [3], M, K), M, K)
    np.testing.assert_allclose(ref.bit_probs(x, M, K)[0], 1.0 - bits, rtol=0, atol=1e-12)


@pytest.mark.parametrize("M,K", [(8, 1), (16, 2), (16, 4), (4, 16), (2, 64)])
def test_section_word_is_the_bit_string_of_msg_vector_2_bin_arr(M, K):
    rng = np.random.default_rng(M * K)
    L = 9
    idx, sym = rng.integers(0, M, L), rng.integers(0, K, L)
    per = sum(ref.bits_of(M, K))
    want = sparc.msg_vector_2_bin_arr(sparc._msg_vector_from_indices(idx, sym, M, K), M, K)
    assert np.array_equal(ref.word_bits(ref.section_words(idx, sym, K), per), want.astype(np.int64))


def test_counters():
    truth = np.zeros((3, 10), dtype=int)
    got = truth.copy()
    got[1, 2] = got[1, 7] = got[2, 9] = 1
    assert ref.counters(got, truth, 4).tolist() == [3, 3, 2, 1, 2]


# ---------------------------------------------------------------- ABI

def _header_arity(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    return len([a for a in m.group(1).split(",") if a.strip()])


NEW = [("sg_camp_soft_output", 2), ("sg_camp_llr_device", 10), ("sg_camp_llr", 8), ("sg_section_llr_psk", 8),
       ("sg_bits_to_psk_sections_strided_device", 10), ("sg_psk_pack_sections_device", 7)]


@pytest.mark.parametrize("name,arity", NEW)
def test_symbols_declared_bound_and_exported(name, arity):
    assert _header_arity(name) == arity
    bound = {n: (r, a) for n, r, a in _native.SIGNATURES}
    assert name in bound and len(bound[name][1]) == arity
    assert hasattr(_native.lib(), name)


def test_new_entry_points_without_a_device():
    if _native.device_count() > 0:
        pytest.skip("GPU present")
    lib = _native.lib()
    out = np.zeros(8)
    calls = [lambda: lib.sg_camp_soft_output(None, 1),
             lambda: lib.sg_camp_llr_device(None, 1, 1, None, 0, 1, 8, 0, _native.ptr(out), None),
             lambda: lib.sg_camp_llr(None, 1, 1, None, 0, 1, 0, _native.ptr(out)),
             lambda: lib.sg_section_llr_psk(_native.ptr(out), 1, 4, 1, None, 0, 0, _native.ptr(out)),
             lambda: lib.sg_bits_to_psk_sections_strided_device(None, 0, 1, 1, 1, 0, None, None, 1, None),
             lambda: lib.sg_psk_pack_sections_device(None, None, 1, 1, 0, None, None)]
    for call in calls:
        assert call() == _native.SG_ERR_NO_DEVICE
        assert b"no GPU" in lib.sg_last_error()
    assert np.all(out == 0)
    with pytest.raises(_native.NativeError, match="no GPU"):
        sparc.section_llr_psk(np.zeros(8, dtype=complex), 1.0, 4, 4)


# ---------------------------------------------------------------- Python surface

def test_pipeline_constructor_checks():
    from ldpc_sparc_amd.pipeline import CsparcConcatPipeline
    ldpc = ("802.11n", "1/2", 27)
    with pytest.raises(NotImplementedError, match="double precision"):
        CsparcConcatPipeline(112, 16, 4, 336, 15.0, 4, 1, ldpc=ldpc, precision="f32")
    with pytest.raises(AssertionError, match="protected sections"):
        CsparcConcatPipeline(112, 16, 4, 336, 15.0, 5, 1, ldpc=ldpc)   # 107 x 6 bits != 648
    with pytest.raises(AssertionError, match="protected sections"):
        CsparcConcatPipeline(112, 16, 1, 336, 15.0, 4, 1, ldpc=ldpc)   # K = 1: 4 bits per section
    with pytest.raises(NotImplementedError):
        CsparcConcatPipeline(112, 16, 128, 336, 15.0, 4, 1, ldpc=ldpc)  # K > 64
    W = np.array(15.0)
    o0, o1 = sparc.generate_ordering(W, 336, 112 * 16, 0)
    with pytest.raises(ValueError, match="ComplexDesignOperator"):
        CsparcConcatPipeline(112, 16, 4, 336, 15.0, 4, 1, ldpc=ldpc, op=sparc.DesignOperator(W, 112, 16, 336, o0, o1))


def test_real_soft_output_still_refuses_a_complex_operator():
    W = np.array(15.0)
    o0, o1 = sparc.generate_ordering(W, 64, 16 * 8, 0, csparc=True)
    op = sparc.ComplexDesignOperator(W, 16, 8, 64, o0, o1)
    with pytest.raises(NotImplementedError, match="real"):
        sparc.amp_llr(op, 1, 0, 16)


def test_fft_sweep_noise_tags_and_checkpoints(tmp_path):
    import json
    assert montecarlo.concat_checkpoint_tag(112, 16, 336, "fft", 4) == "concat_fft_L112_M16_K4_n336"
    assert montecarlo.concat_checkpoint_tag(112, 16, 336, "fft") == "concat_fft_L112_M16_K1_n336"
    with pytest.raises(ValueError, match="fft"):
        montecarlo.concat_ber_sweep(112, 64, 672, 15.0, 4, 1, [2.0], codewords=16, block=16,
                                    ldpc=("802.11n", "1/2", 27), design="dct", K=4)
    calls = []

    def trial(point, first, nb, block):
        calls.append((point, first, nb))
        return np.array([nb * block, 3, 1, 1, 2], dtype=np.int64)
    kw = dict(codewords=32, block=16, ldpc=("802.11n", "1/2", 27), checkpoint_dir=str(tmp_path), trial=trial)
    out = montecarlo.concat_ber_sweep(112, 16, 336, 15.0, 4, 1, [3.0], design="fft", K=4, **kw)
    ub = 4 * 6 + 324
    # complex noise: N0 = awgn_var, Eb/N0 = P / (R_overall awgn_var)
    assert out[0]["R_overall"] == ub / 336
    assert abs(out[0]["awgn_var"] - 15.0 / ((ub / 336) * 10 ** 0.3)) < 1e-12
    assert out[0]["ber"] == 6 / (32 * ub)
    st = json.load(open(tmp_path / "concat_fft_L112_M16_K4_n336_pt0.json"))
    assert st["params"]["design"] == "fft" and st["params"]["K"] == 4
    # the real sweeps keep their factor 2 and their tags
    real = montecarlo.concat_ber_sweep(112, 64, 672, 15.0, 4, 1, [3.0], design="dct", **kw)
    assert abs(real[0]["awgn_var"] - 15.0 / (2 * ((4 * 6 + 324) / 672) * 10 ** 0.3)) < 1e-12
    assert (tmp_path / "concat_dct_L112_M64_n672_pt0.json").exists()


class _FakePipe:
    """Counts what ConcatTrial asks of a pipeline."""
    L_unp, logM, mults = 4, 4, 1
    bits_per_section = 6

    class c:
        K = 324

    def __init__(self):
        self.batches = []

    def make_batch_device(self, B, var, seed, sid):
        self.batches.append((B, sid))

    def reset_counts(self):
        pass

    def decode(self):
        pass

    def counts(self):
        B, sid = self.batches[-1]
        return np.array([B, sid & 0xffff, 1, 0, 0], dtype=np.int64)


def test_trial_granule_keys_draws_independently_of_the_block():
    a, b, c = _FakePipe(), _FakePipe(), _FakePipe()
    ta = montecarlo.ConcatTrial(a, [1.0, 1.0], granule=32)
    assert ta.user_bits == 4 * 6 + 324
    ra = ta(1, 0, 2, 32)
    rb = montecarlo.ConcatTrial(b, [1.0, 1.0], granule=32)(1, 0, 1, 64)
    assert a.batches == b.batches == [(32, (1 << 32) | 0), (32, (1 << 32) | 1)]
    assert np.array_equal(ra, rb)
    montecarlo.ConcatTrial(c, [1.0, 1.0])(1, 3, 1, 64)  # no granule: the block is the batch, keyed by its index
    assert c.batches == [(64, (1 << 32) | 3)]
    with pytest.raises(ValueError, match="granule"):
        montecarlo.ConcatTrial(c, [1.0], granule=48)(0, 0, 1, 64)
