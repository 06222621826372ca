"""CPU tests around the K = 2 decoder's soft output: the yardstick
(tests/bpsk_concat_ref.py) is tied to the reference's K = 2 denoiser, the new
C-ABI entry points are declared, bound, exported and refuse without a GPU,
concat_ber_sweep(design="dct", K=2) names, parametrises and refuses as it
should, and the shapes and operating points that tests/test_bpsk_concat_gpu.py
decodes are what it needs them to be -- on the restatement alone."""
import json
import os
import re

import numpy as np
import pytest

import amp_bpsk_ref as br
import bpsk_concat_ref as ref
from bpsk_cases import AWGN_VAR, BPSK_CASES, code_params, design, golden
from ldpc_sparc_amd import _native, montecarlo, sparc
from ldpc_sparc_amd.ldpc import code

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ldpc_sparc_amd.h")


def soft_count(p):
    return int(np.count_nonzero((p > 0.01) & (p < 0.99)))


# ---------------------------------------------------------------- the yardstick

@pytest.mark.parametrize("name,cp,dp,ns", BPSK_CASES, ids=[c[0] for c in BPSK_CASES])
def test_posterior_mean_is_the_reference_denoiser(name, cp, dp, ns):
    """sum_c c p(j, c) = mmse_bpsk on every golden design, at observations of
    the design's own scale: what ties the soft output to the reference."""
    W, L, M, n, o0, o1 = design(golden(), name, code_params(cp))
    rng = np.random.default_rng(len(name))
    for scale in (0.3, 1.0, 4.0):
        s = scale * rng.standard_normal(L * M)
        s[::M] += 1.0
        tau = np.full(L * M, 0.37 * scale)
        got = ref.posterior_mean(s / tau, M)
        want = br.mmse_bpsk(s, tau, M)
        print(name, scale, "max |mean - mmse_bpsk|", np.abs(got - want).max())
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
        p = ref.bit_probs(s / tau, M)
        assert p.shape == (L, int(np.log2(M)) + 1) and np.all(p >= 0) and np.all(p <= 1 + 1e-15)


def test_bit_order_is_the_words():
    """An observation on (location 5, sign -) puts every bit on the digits of the word (5 << 1) | 1."""
    M = 8
    x = np.zeros(M)
    x[5] = -60.0
    want = 1.0 - ref.word_bits([(5 << 1) | 1], 4)
    np.testing.assert_allclose(ref.bit_probs(x, M)[0], want, rtol=0, atol=1e-12)
    x[5] = 60.0
    np.testing.assert_allclose(ref.bit_probs(x, M)[0], 1.0 - ref.word_bits([5 << 1], 4), rtol=0, atol=1e-12)


# ---------------------------------------------------------------- ABI

def _header_arity(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    return len([a for a in m.group(1).split(",") if a.strip()])


NEW = [("sg_amp_bpsk_soft_output", 2), ("sg_amp_bpsk_llr_device", 8), ("sg_amp_bpsk_llr", 6)]


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
    calls = [lambda: lib.sg_amp_bpsk_soft_output(None, 1),
             lambda: lib.sg_amp_bpsk_llr_device(None, 1, 0, 1, 8, 0, _native.ptr(out), None),
             lambda: lib.sg_amp_bpsk_llr(None, 1, 0, 1, 0, _native.ptr(out))]
    for call in calls:
        assert call() == _native.SG_ERR_NO_DEVICE
        assert b"no GPU" in lib.sg_last_error()
    assert np.all(out == 0)


def test_python_surface_refuses_a_complex_operator():
    W = np.array(15.0)
    o0, o1 = sparc.generate_ordering(W, 64, 16 * 8, 0, csparc=True)
    op = sparc.ComplexDesignOperator(W, 16, 8, 64, o0, o1)
    with pytest.raises(ValueError, match="camp_llr"):
        sparc.amp_llr_bpsk(op, 1, 0, 16)


# ---------------------------------------------------------------- sweep

def test_k2_sweep_noise_tags_and_refusals(tmp_path):
    assert montecarlo.concat_checkpoint_tag(144, 32, 864, "dct_k2", 2) == "concat_dct_k2_L144_M32_n864"

    def trial(point, first, nb, block):
        return np.array([nb * block, 3, 1, 1, 2], dtype=np.int64)
    kw = dict(codewords=32, block=16, ldpc=ref.LDPC, checkpoint_dir=str(tmp_path), trial=trial)
    out = montecarlo.concat_ber_sweep(144, 32, 864, 15.0, 36, 1, [3.0], design="dct", K=2, **kw)
    ub = 36 * 6 + 324  # log2 M + 1 bits per section
    assert out[0]["R_overall"] == ub / 864
    assert abs(out[0]["awgn_var"] - 15.0 / (2 * (ub / 864) * 10 ** 0.3)) < 1e-12  # real noise: the factor 2
    assert out[0]["ber"] == 6 / (32 * ub)
    st = json.load(open(tmp_path / "concat_dct_k2_L144_M32_n864_pt0.json"))
    assert st["params"]["design"] == "dct_k2" and st["params"]["K"] == 2
    with pytest.raises(ValueError, match="fft"):
        montecarlo.concat_ber_sweep(144, 32, 864, 15.0, 36, 1, [3.0], design="dct", K=4, **kw)
    with pytest.raises(ValueError, match="fft"):
        montecarlo.concat_ber_sweep(144, 32, 864, 15.0, 36, 1, [3.0], design="dense", K=2, **kw)
    with pytest.raises(ValueError, match="known sections for K = 2 are not built"):
        montecarlo.concat_ber_sweep(144, 32, 864, 15.0, 36, 1, [3.0], design="dct", K=2, final_amp=True, **kw)
    # a plain DCT sweep keeps its tag and parameters
    plain = montecarlo.concat_ber_sweep(112, 64, 672, 15.0, 4, 1, [3.0], design="dct", **kw)
    assert abs(plain[0]["awgn_var"] - 15.0 / (2 * ((4 * 6 + 324) / 672) * 10 ** 0.3)) < 1e-12
    st = json.load(open(tmp_path / "concat_dct_L112_M64_n672_pt0.json"))
    assert st["params"]["design"] == "dct" and "K" not in st["params"]


# ---------------------------------------------------------------- the GPU tests' cases, on the restatement alone

BAR = 1e-9


def _moves(Y, W, L, M, n, var, t_max, ops, dp, want):
    """How far the restatement's probabilities of each codeword move when every received value moves by one ulp."""
    out = []
    for b in range(len(Y)):
        st = ref.amp_bpsk_soft(np.nextafter(Y[b], np.inf), W, L, M, n, var, t_max, *ops, **dp)
        out.append(np.abs(ref.soft_probs(st, M) - want[b]).max())
    return np.array(out)


@pytest.mark.parametrize("name,cp,dp,ns", BPSK_CASES, ids=[c[0] for c in BPSK_CASES])
def test_golden_designs_are_soft_and_stable(name, cp, dp, ns):
    """Every golden design, three seeds as one batch: soft probabilities at
    t_max = 3, and at most one codeword that the one-ulp rule leaves out at
    either t_max."""
    g = golden()
    W, L, M, n, o0, o1 = design(g, name, code_params(cp))
    ops = br.operators(W, L, M, n, o0, o1)
    Y, _ = ref.golden_batch(g, name, cp, ops)
    kw = dict(rtol=1e-6, phi_method=dp.get('phi_est_method', 1))
    for t_max in (3, dp['t_max']):
        sts = [ref.amp_bpsk_soft(y, W, L, M, n, AWGN_VAR, t_max, *ops, **kw) for y in Y]
        want = [ref.soft_probs(st, M) for st in sts]
        soft = sum(soft_count(p) for p in want)
        mv = _moves(Y, W, L, M, n, AWGN_VAR, t_max, ops, kw, want)
        print(name, "t_max", t_max, "soft", soft, "t_final", [st["t_final"] for st in sts], "moves", mv)
        if t_max == 3:
            assert soft >= 20
        if name == "bhard":
            assert soft >= 20  # stays soft to the end
        assert np.count_nonzero(mv > BAR) <= 1


@pytest.mark.parametrize("name", list(ref.SIZES) + ["pa256"])
def test_section_size_cases_are_soft(name):
    W, L, M, n, o0, o1, words, Y, ops = ref.size_case(name)
    want = np.stack([ref.soft_probs(ref.amp_bpsk_soft(y, W, L, M, n, 1.0, ref.SIZE_TMAX, *ops), M) for y in Y])
    soft = (want > 0.01) & (want < 0.99)
    logM = int(np.log2(M))
    high = int(np.count_nonzero(soft[:, :, :max(logM - 6, 0)]))  # location bits >= 6 come first (MSB first)
    print(name, "soft", int(soft.sum()), "in bits >= 6", high)
    assert soft.sum() >= 20
    if M >= 128:
        assert high >= 5
    if name == "pa256":
        assert np.asarray(W).shape == (4,)


@pytest.fixture(scope="module")
def point_results():
    from oracle import sparc_ref
    out = {}

    def get(name):
        if name not in out:
            L, M, Lu, mults, n, var = ref.POINTS[name]
            W, o0, o1 = ref.flat_design(L, M, n, ref.P, 0)
            ops = sparc_ref.dct_operators(W, L, M, n, o0, o1)
            words, info, noise = ref.point_batch(name)
            Y = np.stack([ops[0](br.beta_of_words(w, M)) for w in words]) + noise
            c = code(*ref.LDPC)
            per = int(np.log2(M)) + 1
            sts = [ref.amp_bpsk_soft(y, W, L, M, n, var, 25, *ops) for y in Y]
            probs = [ref.soft_probs(st, M) for st in sts]
            dec = [ref.decode_user_bits(st, L, M, Lu, c) for st in sts]
            truth = np.stack([ref.user_bits_truth(words[b], info.reshape(ref.PIPE_B, -1)[b], Lu, per)
                              for b in range(ref.PIPE_B)])
            mv = _moves(Y, W, L, M, n, var, 25, ops, {}, probs)
            out[name] = dict(words=words, sts=sts, probs=probs, dec=dec, truth=truth, moves=mv, Lu=Lu, per=per, c=c)
        return out[name]
    return get


@pytest.mark.parametrize("name", ["A", "B"])
def test_operating_points(point_results, name):
    """At A every LDPC block converges and hundreds of protected probabilities
    are soft; at B some blocks converge and some do not; at both the one-ulp
    rule leaves out at most 2 of 8 codewords."""
    r = point_results(name)
    Lu, c = r["Lu"], r["c"]
    wrong = sum(int(np.count_nonzero(st["words"] != r["words"][b])) for b, st in enumerate(r["sts"]))
    soft = sum(soft_count(p[Lu:]) for p in r["probs"])
    conv = [all(it < 200 for it in d[1]) for d in r["dec"]]
    cnt = ref.counters(np.stack([d[0] for d in r["dec"]]), r["truth"], Lu * r["per"])
    print(name, "AMP wrong sections", wrong, "soft protected", soft, "BP converged", sum(conv), "of", len(conv),
          "counters", cnt.tolist(), "moves", r["moves"])
    if name == "A":
        assert all(conv) and soft >= 500
    else:
        assert any(conv) and not all(conv)
    assert np.count_nonzero(r["moves"] > BAR) <= 2
