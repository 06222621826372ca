"""GPU tests of the complex engine's soft output (sg_camp_soft_output,
sg_camp_llr*, sg_section_llr_psk, camp_llr.hip) and of the concatenated K-PSK
SPARC + LDPC decoder built on it (pipeline.CsparcConcatPipeline,
concat_ber_sweep(design="fft")).

The yardstick is tests/csparc_concat_ref.py: the joint posterior over
(location, symbol) by brute force, its bit marginals, the AMP loop of
tests/csparc_ref.py keeping its last s and tau, the clip / log of ldpc_bp and
oracle.bp.decode.

Bars.  Stand-alone kernel: probabilities atol 1e-12 at |x| <= 100 (the
exponent's argument carries an absolute error of about 1e-14 there and the sums
have at most 2^17 positive terms); 1e-9, the after-decode bar, at |x| ~ 1e4.
After a decode: atol 1e-9 (the f64 parity bar of test_amp_gpu.py).  LLR against
the clip / log of the same call's probabilities: rtol 1e-12.  Pipeline LLRs
against the yardstick's: rtol 1e-6, atol 1e-9.

Every seed and operating point below was chosen on the CPU with the yardstick
alone (the assertions on `margin`, on the stopping iterations and on the BP
iteration counts repeat that choice's conditions at test time):
 * after a decode, DECODE_SEEDS (the first seed of each design with the
   property): at every stopping test of every codeword the yardstick's
   |psi - psi_prev| is a factor >= 2.5 away from its threshold (asserted:
   >= 2), so a 1e-13 transform difference cannot move t_final; cpa4 also
   stops by itself before iteration 22 of 30;
 * stopped codewords, seed 13, noise standard deviations MIXED_SIGMAS at
   rtol = 1e-2: stopping iterations [7, 7, 8, 14, 7, 24], the same factor;
 * pipeline, L = 112, M = 16, K = 4, n = PIPE_N, awgn_var = PIPE_VAR, batch seed
   PIPE_SEED: the yardstick decodes all 8 codewords and every BP run stops
   before its cap (n = 336 is R = 2 bits per channel use; this short code's
   waterfall is steep: at n <= 240 the yardstick's AMP fails on some of the 8
   codewords and BP with it).  There and at twice the variance every posterior
   is hard; test_pipeline_soft_llrs adds the batch with soft LLRs."""
import ctypes as ct
import functools

import numpy as np
import pytest

import csparc_cases as cc
import csparc_concat_ref as ref
import csparc_ref
from dct_concat_ref import llr_of_probs
from ldpc_sparc_amd import _native, montecarlo, sparc
from ldpc_sparc_amd.pipeline import CsparcConcatPipeline

pytestmark = pytest.mark.gpu

LO = np.log(1e-15) - np.log(1 - 1e-15)  # the LLR of a probability clipped from below


def _c(K):
    return sparc._interleaved(sparc.psk_constel(K)) if K != 1 else None


# ---------------------------------------------------------------- 1: the stand-alone kernel

STANDALONE = [(2, 1), (2, 4), (16, 8), (8, 64), (64, 2), (128, 4), (512, 16), (2048, 1), (2048, 4)]
SCALES = (0.1, 1.0, 30.0, 100.0)


def standalone_x(M, K, real=False):
    """8 sections of complex Gaussian x at the four scales, section 4 with all
    entries equal, and a ninth section with |x| ~ 1e4."""
    rng = np.random.default_rng(1000 * M + K)
    x = (rng.standard_normal((9, M)) + 1j * rng.standard_normal((9, M))) / np.sqrt(2)
    for l in range(8):
        x[l] *= SCALES[l % 4]
    x[4] = 0.7 - 0.3j
    x[8] *= 1e4
    if real:
        x = x.real * np.sqrt(2)
    return x.reshape(-1)


def _section_llr(x, M, K, probs_only):
    # tau = 2 (complex) / 1 (real) makes x = s exactly
    return sparc.section_llr_psk(x, 2.0 if np.iscomplexobj(x) else 1.0, M, K, probs_only=probs_only)


@pytest.mark.parametrize("M,K", STANDALONE)
def test_standalone_kernel_matches_enumeration(M, K):
    x = standalone_x(M, K)
    per = sum(ref.bits_of(M, K))
    want = ref.bit_probs(x if K > 2 else x.real.astype(complex), M, K)
    got = _section_llr(x, M, K, True).reshape(9, per)
    assert np.all(np.isfinite(got))
    print(f"M={M} K={K}: max |p - enumeration| = {np.max(np.abs(got[:8] - want[:8])):.3e}, "
          f"|x| ~ 1e4: {np.max(np.abs(got[8] - want[8])):.3e}")
    np.testing.assert_allclose(got[:8], want[:8], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[8], want[8], rtol=0, atol=1e-9)
    logM = ref.bits_of(M, K)[0]
    np.testing.assert_allclose(got[4, :logM], 0.5, rtol=0, atol=1e-12)  # all entries equal: location bits are coins
    # LLR = ldpc_bp's clip / log of the same call's probabilities
    llr = _section_llr(x, M, K, False).reshape(9, per)
    assert np.all(np.isfinite(llr))
    np.testing.assert_allclose(llr, llr_of_probs(got), rtol=1e-12, atol=0)
    # clipped values are exactly those of the clip: log(1e-15) - log(1 - 1e-15) below and, since 1 - 1e-15 is not
    # a double, the clip / log of 1.0 above (34.5396, not the negative of the lower 34.5388)
    assert np.all(llr[got <= 1e-15] == LO)
    assert np.all(llr[got >= 1 - 1e-15] == llr_of_probs(1.0))
    assert np.any((got <= 1e-15) | (got >= 1 - 1e-15))


@pytest.mark.parametrize("M,K", [(64, 2), (128, 1)])
def test_standalone_kernel_real_x(M, K):
    x = standalone_x(M, K, real=True)
    per = sum(ref.bits_of(M, K))
    want = ref.bit_probs(x.astype(complex), M, K)
    got = _section_llr(x, M, K, True).reshape(9, per)
    np.testing.assert_allclose(got[:8], want[:8], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[8], want[8], rtol=0, atol=1e-9)


def test_standalone_kernel_refuses_m4096():
    lib = _native.lib()
    x = np.zeros(2 * 4096)
    out = np.full(14, -777.0)
    rc = lib.sg_section_llr_psk(_native.ptr(x), 1, 4096, 4, _native.ptr(_c(4)), 1, 1, _native.ptr(out))
    assert rc == _native.SG_ERR_UNSUPPORTED
    assert b"4096" in lib.sg_last_error()
    assert np.all(out == -777.0)


# ---------------------------------------------------------------- 2: after a decode

B = 4
DECODE_SEEDS = {"creg": 1, "cpsk4": 1, "cpsk8": 1, "cpsk2m2": 1, "cpa4": 64, "csc4": 1}
DECODE_CASES = list(DECODE_SEEDS)


class Case:
    """B codewords of a golden design through the NumPy operators, and the yardstick's decode of each."""

    def __init__(self, name, seed=None, sigmas=None, rtol=1e-6, nb=B):
        seed = DECODE_SEEDS[name] if seed is None else seed
        _, cp, dp, _ = next(c for c in cc.CSPARC_CASES if c[0] == name)
        cp = cc.code_params(cp)
        self.K = cp['K'] if cp.get('modulated') else 1
        self.W, self.L, self.M, self.n, self.o0, self.o1 = cc.design(cc.golden(), name, cp)
        self.t_max, self.phi = dp['t_max'], dp.get('phi_est_method', 1)
        self.rtol, self.nb = rtol, nb
        self.Ab, self.Az = csparc_ref.fft_operators(self.W, self.L, self.M, self.n, self.o0, self.o1)
        rng = np.random.RandomState(seed)
        L, M, K, n = self.L, self.M, self.K, self.n
        self.idx = rng.randint(0, M, (nb, L))
        self.sym = rng.randint(0, K, (nb, L))
        beta0 = np.zeros((nb, L * M), dtype=complex)
        beta0[np.arange(nb)[:, None], np.arange(L) * M + self.idx] = ref.constel(K)[self.sym]
        sig = np.broadcast_to(np.sqrt(cc.AWGN_VAR) if sigmas is None else np.asarray(sigmas), (nb,))
        noise = (rng.randn(nb, n) + 1j * rng.randn(nb, n)) / np.sqrt(2)
        self.Y = np.stack([self.Ab(beta0[b]) for b in range(nb)]) + sig[:, None] * noise
        self.per = sum(ref.bits_of(M, K))
        self.op = None

    @functools.lru_cache(maxsize=None)
    def oracle(self):
        return [ref.amp_soft(self.Y[b], self.W, self.L, self.M, self.n, self.K, self.Ab, self.Az, cc.AWGN_VAR,
                             self.t_max, self.rtol, self.phi) for b in range(self.nb)]

    def decode(self, rows=slice(None), soft=True):
        if self.op is None:
            self.op = sparc.ComplexDesignOperator(self.W, self.L, self.M, self.n, self.o0, self.o1)
        self.op.soft_output(soft)
        return sparc.camp_decode_batch(self.Y[rows], self.op, cc.AWGN_VAR, self.t_max, self.rtol, self.phi, self.K)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@pytest.mark.parametrize("name", DECODE_CASES)
def test_soft_output_after_a_decode(name):
    c = case(name)
    orc = c.oracle()
    assert min(o["margin"] for o in orc) >= 2.0, [o["margin"] for o in orc]
    mi, ms, tf, _, _ = c.decode()
    assert np.array_equal(tf, [o["t_final"] for o in orc])
    assert np.array_equal(mi, np.stack([o["idx"] for o in orc]))
    assert np.array_equal(ms, np.stack([o["sym"] for o in orc]))
    want = np.stack([ref.soft_probs(o, c.M, c.K).reshape(-1) for o in orc])
    got = sparc.camp_llr(c.op, B, c.K, 0, c.L, probs_only=True)
    print(f"{name}: t_final {tf.tolist()}, max |p - yardstick| = {np.max(np.abs(got - want)):.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    # a sub-range with l0 > 0 and a row stride longer than needed
    l0, nl = 3, c.L - 5
    ld = nl * c.per + 7
    buf = _native.DeviceBuffer.from_array(np.full((B, ld), -777.0))
    _native.check(_native.lib().sg_camp_llr_device(c.op.plan(), B, c.K, _native.ptr(_c(c.K)), l0, nl, ld, 1, buf.ptr,
                                                   None))
    _native.synchronize()
    out = buf.download(np.empty((B, ld)))
    assert np.all(out[:, nl * c.per:] == -777.0)
    assert np.array_equal(out[:, :nl * c.per], got[:, l0 * c.per:(l0 + nl) * c.per])
    np.testing.assert_allclose(out[:, :nl * c.per], want[:, l0 * c.per:(l0 + nl) * c.per], rtol=0, atol=1e-9)
    # the LLRs are the clip / log of these probabilities, and the same bits on every run
    llr = sparc.camp_llr(c.op, B, c.K, 0, c.L)
    np.testing.assert_allclose(llr, llr_of_probs(got), rtol=1e-12, atol=0)
    assert np.array_equal(llr, sparc.camp_llr(c.op, B, c.K, 0, c.L))


# ---------------------------------------------------------------- 3: stopped codewords keep their state

MIXED_SEED = 13
MIXED_SIGMAS = (0.01, 0.6, 1.0, 1.4, 1.8, 6.0)  # clean ... hopeless


@functools.lru_cache(maxsize=None)
def mixed_case():
    return Case("cpsk4", seed=MIXED_SEED, sigmas=MIXED_SIGMAS, rtol=1e-2, nb=len(MIXED_SIGMAS))


def test_stopped_codewords_keep_their_state():
    """Codewords that stop at different iterations: each one's soft output is
    that of decoding it alone.  Later iterations of the others touching a
    stopped codeword's s or tau would move every probability that is not hard."""
    c = mixed_case()
    orc = c.oracle()
    tf_ref = [o["t_final"] for o in orc]
    assert len(set(tf_ref)) >= 3, tf_ref
    assert min(o["margin"] for o in orc) >= 2.0, [o["margin"] for o in orc]
    nb = c.nb
    _, _, tf, _, _ = c.decode()
    assert np.array_equal(tf, tf_ref)
    got = sparc.camp_llr(c.op, nb, c.K, 0, c.L, probs_only=True)
    soft = np.count_nonzero((got > 0.01) & (got < 0.99), axis=1)
    assert np.count_nonzero(soft >= 10) >= 2, soft
    for b in range(nb):
        _, _, t1, _, _ = c.decode(slice(b, b + 1))
        assert t1[0] == tf[b]
        one = sparc.camp_llr(c.op, 1, c.K, 0, c.L, probs_only=True)
        np.testing.assert_allclose(got[b], one[0], rtol=0, atol=1e-9)


# ---------------------------------------------------------------- 4: contract

def test_contract():
    c = case("cpsk4")
    lib = _native.lib()
    L, per, K = c.L, c.per, c.K
    cs = _native.ptr(_c(K))
    buf = _native.DeviceBuffer.from_array(np.full((B, L * per), -777.0))

    def llr(plan, *args):
        return lib.sg_camp_llr_device(plan, *args, 1, buf.ptr, None)

    fresh = sparc.ComplexDesignOperator(c.W, c.L, c.M, c.n, c.o0, c.o1)
    plan = fresh.plan()
    ok = (B, K, cs, 0, L, L * per)
    # off by default, also after a decode
    assert llr(plan, *ok) == _native.SG_ERR_BAD_ARG and b"soft output is off" in lib.sg_last_error()
    off = sparc.camp_decode_batch(c.Y, fresh, cc.AWGN_VAR, c.t_max, c.rtol, c.phi, K)
    assert llr(plan, *ok) == _native.SG_ERR_BAD_ARG and b"soft output is off" in lib.sg_last_error()
    # on, but no decode yet
    fresh.soft_output(True)
    assert llr(plan, *ok) == _native.SG_ERR_BAD_ARG and b"no decode" in lib.sg_last_error()
    on = sparc.camp_decode_batch(c.Y, fresh, cc.AWGN_VAR, c.t_max, c.rtol, c.phi, K)
    # the same batch with soft output off and on: bit-identical decoder outputs
    for a, b in zip(off, on):
        assert np.array_equal(a, b)
    for args in ((B - 1, K, cs, 0, L, L * per),          # another batch size than the decode's
                 (B + 1, K, cs, 0, L, L * per),
                 (B, 8, _native.ptr(_c(8)), 0, L, L * (per + 1)),  # another K
                 (B, 1, None, 0, L, L * per),
                 (B, K, cs, 1, L, L * per),              # nl past L
                 (B, K, cs, 0, L + 1, (L + 1) * per),
                 (B, K, cs, -1, 2, L * per),
                 (B, K, cs, 0, L, L * per - 1)):         # short llr_ld
        assert llr(plan, *args) == _native.SG_ERR_BAD_ARG, args
        assert lib.sg_last_error()
    _native.synchronize()
    assert np.all(buf.download(np.empty((B, L * per))) == -777.0)  # nothing was launched
    assert llr(plan, *ok) == _native.SG_OK
    _native.synchronize()
    first = buf.download(np.empty((B, L * per)))
    assert np.all((first >= 0) & (first <= 1))
    # sg_camp_apply clears the state
    fresh.apply(np.zeros((B, c.L * c.M), dtype=complex), False)
    assert llr(plan, *ok) == _native.SG_ERR_BAD_ARG and b"no decode" in lib.sg_last_error()
    # ... so does sg_camp_encode_device
    sparc.camp_decode_batch(c.Y, fresh, cc.AWGN_VAR, c.t_max, c.rtol, c.phi, K)
    assert llr(plan, *ok) == _native.SG_OK
    d_idx = _native.DeviceBuffer.from_array(c.idx.astype(np.int32))
    d_sym = _native.DeviceBuffer.from_array(c.sym.astype(np.int32))
    d_x = _native.DeviceBuffer(B * c.n * 16)
    _native.check(lib.sg_camp_encode_device(plan, K, cs, d_idx.ptr, d_sym.ptr, B, d_x.ptr, None))
    assert llr(plan, *ok) == _native.SG_ERR_BAD_ARG and b"no decode" in lib.sg_last_error()
    # ... a B = 0 decode and a failed one
    sparc.camp_decode_batch(c.Y, fresh, cc.AWGN_VAR, c.t_max, c.rtol, c.phi, K)
    assert lib.sg_camp_decode_device(plan, None, 0, K, cs, None, None, 1.0, 25, 1e-6, 1, None, None, None, None, None,
                                     None) == _native.SG_OK
    assert llr(plan, *ok) == _native.SG_ERR_BAD_ARG
    sparc.camp_decode_batch(c.Y, fresh, cc.AWGN_VAR, c.t_max, c.rtol, c.phi, K)
    assert lib.sg_camp_decode_device(plan, None, B, K, cs, None, None, 1.0, 25, 1e-6, 1, None, None, None, None, None,
                                     None) == _native.SG_ERR_BAD_ARG
    assert llr(plan, *ok) == _native.SG_ERR_BAD_ARG
    # switching off refuses again; the host variant raises
    sparc.camp_decode_batch(c.Y, fresh, cc.AWGN_VAR, c.t_max, c.rtol, c.phi, K)
    fresh.soft_output(False)
    with pytest.raises(_native.NativeError, match="soft output is off"):
        sparc.camp_llr(fresh, B, K, 0, L)
    with pytest.raises(NotImplementedError):  # the real entry stays as it is
        sparc.amp_llr(fresh, B, 0, L)


# ---------------------------------------------------------------- 5: pipeline, small geometry

PIPE = dict(L=112, M=16, K=4, L_unp=4, mults=1, ldpc=("802.11n", "1/2", 27), P=15.0)
PIPE_N, PIPE_VAR, PIPE_SEED, PIPE_SEED2, PIPE_DESIGN_SEED, PIPE_B = 336, 0.5, 1, 1, 2, 8
SOFT_VAR, SOFT_SEED = 2.0, 13


def pipe_design():
    g = PIPE
    W = np.array(g["P"])
    o0, o1 = sparc.generate_ordering(W, PIPE_N, g["L"] * g["M"], PIPE_DESIGN_SEED, csparc=True)
    assert sparc.transform_size(PIPE_N, g["L"] * g["M"], True) == 2048
    return W, o0, o1


def pipe_oracle(Y, var, W, o0, o1, c, bp_its=200):
    """Per codeword: (amp_soft state, LLRs of the protected sections, user bits, BP iteration counts)."""
    g = PIPE
    L, M, K = g["L"], g["M"], g["K"]
    Ab, Az = csparc_ref.fft_operators(W, L, M, PIPE_N, o0, o1)
    out = []
    for y in Y:
        st = ref.amp_soft(y, W, L, M, PIPE_N, K, Ab, Az, var, 25)
        llr = llr_of_probs(ref.soft_probs(st, M, K)[g["L_unp"]:].reshape(-1))
        bits, its = ref.decode_user_bits(st, L, M, K, g["L_unp"], c, bp_its)
        out.append((st, llr, bits, its))
    return out


def _make_pipe(**kw):
    g = PIPE
    return CsparcConcatPipeline(g["L"], g["M"], g["K"], PIPE_N, g["P"], g["L_unp"], g["mults"], ldpc=g["ldpc"],
                                design_seed=PIPE_DESIGN_SEED, **kw)


def test_pipeline_equals_the_yardstick(oracle_built):
    g = PIPE
    L, K, Lu, per = g["L"], g["K"], g["L_unp"], 6
    pipe = _make_pipe()
    W, o0, o1 = pipe_design()
    assert np.array_equal(pipe.op.order0[0], o0) and np.array_equal(pipe.op.order1[0], o1)
    c = pipe.c
    idx, sym, info = pipe.make_batch(PIPE_B, PIPE_VAR, np.random.default_rng(PIPE_SEED))
    pipe.reset_counts()
    pipe.decode()
    cnt = pipe.counts()
    Y = pipe.d_y.download(np.empty((PIPE_B, PIPE_N), np.complex128))
    orc = pipe_oracle(Y, PIPE_VAR, W, o0, o1, c)
    truth = np.stack([np.concatenate([ref.word_bits(ref.section_words(idx[b, :Lu], sym[b, :Lu], K), per),
                                      info.reshape(PIPE_B, -1)[b]]) for b in range(PIPE_B)])
    bits = np.stack([o[2] for o in orc])
    assert np.array_equal(bits, truth)                      # the yardstick alone decodes all 8 codewords
    assert max(max(o[3]) for o in orc) < 200                # ... with BP stopping before its cap
    want = ref.counters(bits, truth, Lu * per)
    llr = pipe.d_llr.download(np.empty((PIPE_B, c.N)))
    wl = np.stack([o[1] for o in orc])
    print(f"counters {cnt.tolist()}, yardstick {want.tolist()}, max |llr - yardstick| = {np.max(np.abs(llr - wl)):.3e}")
    np.testing.assert_allclose(llr, wl, rtol=1e-6, atol=1e-9)
    # user bits of every codeword: unprotected words and the systematic BP decisions
    words = pipe.d_idx.download(np.empty((PIPE_B, L), np.int32))
    app = pipe.d_app.download(np.empty((PIPE_B, c.N)))
    got = np.stack([np.concatenate([ref.word_bits(words[b, :Lu], per), (app[b, :c.K] < 0).astype(np.int64)])
                    for b in range(PIPE_B)])
    assert np.array_equal(got, bits)
    assert np.array_equal(cnt, want)
    # a second batch at twice the noise variance: LLRs only
    pipe.make_batch(PIPE_B, 2 * PIPE_VAR, np.random.default_rng(PIPE_SEED2))
    pipe.reset_counts()
    pipe.decode()
    assert pipe.counts()[0] == PIPE_B
    Y = pipe.d_y.download(np.empty((PIPE_B, PIPE_N), np.complex128))
    llr = pipe.d_llr.download(np.empty((PIPE_B, c.N)))
    Ab, Az = csparc_ref.fft_operators(W, L, g["M"], PIPE_N, o0, o1)
    st = [ref.amp_soft(y, W, L, g["M"], PIPE_N, K, Ab, Az, 2 * PIPE_VAR, 25) for y in Y]
    assert min(o["margin"] for o in st) >= 2.0
    wl = np.stack([llr_of_probs(ref.soft_probs(o, g["M"], K)[Lu:].reshape(-1)) for o in st])
    print(f"awgn_var {2 * PIPE_VAR}: max |llr - yardstick| = {np.max(np.abs(llr - wl)):.3e}")
    np.testing.assert_allclose(llr, wl, rtol=1e-6, atol=1e-9)


def test_pipeline_soft_llrs(oracle_built):
    """A third batch, at awgn_var = 2 (seed SOFT_SEED, the first with the
    stopping margin), where 300 to 400 of a codeword's 648 LLRs are soft.

    log p - log(1 - p) of a p rounded to double is ill-conditioned where p is
    near 1: 1 - p is then a few units of 1.1e-16 and one unit's difference in p
    -- another order of the same sum -- moves the LLR by up to ln 2.  Measured
    on the MI355X at this batch: every probability within 1e-13 of the
    yardstick's, yet 723 of 5184 LLRs outside rtol 1e-6, the largest
    difference 0.28768 = ln(4 / 3) (1 - p of 4 units against 3).  The
    yardstick's own LLR has that error, so the pipeline bar (rtol 1e-6, atol
    1e-9) is asked where it means something, 1 - p >= 1e-9 (an LLR error of at
    most 1.1e-7 from p's rounding; P(bit = 0) near 0 is well-conditioned),
    and every bit is compared as a probability at the after-decode bar."""
    g = PIPE
    L, M, K, Lu, per = g["L"], g["M"], g["K"], g["L_unp"], 6
    pipe = _make_pipe()
    W, o0, o1 = pipe_design()
    c = pipe.c
    pipe.make_batch(PIPE_B, SOFT_VAR, np.random.default_rng(SOFT_SEED))
    pipe.reset_counts()
    pipe.decode()
    Y = pipe.d_y.download(np.empty((PIPE_B, PIPE_N), np.complex128))
    llr = pipe.d_llr.download(np.empty((PIPE_B, c.N)))
    probs = sparc.camp_llr(pipe.op, PIPE_B, K, Lu, L - Lu, probs_only=True)
    Ab, Az = csparc_ref.fft_operators(W, L, M, PIPE_N, o0, o1)
    st = [ref.amp_soft(y, W, L, M, PIPE_N, K, Ab, Az, SOFT_VAR, 25) for y in Y]
    assert min(o["margin"] for o in st) >= 2.0
    wp = np.stack([ref.soft_probs(o, M, K)[Lu:].reshape(-1) for o in st])
    wl = llr_of_probs(wp)
    well = 1 - wp >= 1e-9
    soft = np.abs(wl) < 34
    assert np.count_nonzero(soft) >= 8 * 100 and np.count_nonzero(soft & well) >= 8 * 50
    print(f"max |p - yardstick| = {np.max(np.abs(probs - wp)):.3e}; LLR: max difference {np.max(np.abs(llr - wl)):.3e}, "
          f"where 1 - p >= 1e-9 {np.max(np.abs(llr - wl)[well]):.3e}")
    np.testing.assert_allclose(probs, wp, rtol=0, atol=1e-9)
    np.testing.assert_allclose(llr[well], wl[well], rtol=1e-6, atol=1e-9)
    assert np.array_equal(llr < 0, wl < 0)
    np.testing.assert_allclose(llr, llr_of_probs(probs), rtol=1e-12, atol=0)


# ---------------------------------------------------------------- 6: make_batch_device

def test_make_batch_device():
    g = PIPE
    L, M, K, Lu, per = g["L"], g["M"], g["K"], g["L_unp"], 6
    pipe = _make_pipe()
    c = pipe.c
    Bd = 16

    def state():
        return (pipe.d_tidx.download(np.zeros((Bd, L), np.int32)), pipe.d_tsym.download(np.zeros((Bd, L), np.int32)),
                pipe.d_info.download(np.zeros((Bd, c.K), np.uint8)), pipe.d_unp.download(np.zeros((Bd, Lu * per), np.uint8)),
                pipe.d_x.download(np.zeros((Bd, PIPE_N), np.complex128)),
                pipe.d_y.download(np.zeros((Bd, PIPE_N), np.complex128)), pipe.d_true.download(np.zeros((Bd, L), np.int32)))

    pipe.make_batch_device(Bd, 1e-6, 7, (3 << 32) | 5)
    idx, sym, info, unp, x, y, words = state()
    # the true (idx, sym) are the PSK bit mapping of the bits: unprotected sections, then LDPC codewords
    bits = np.concatenate([unp, c.encode_batch(info.astype(np.int64))], axis=1).astype(bool)
    for b in range(Bd):
        beta0 = sparc.bin_arr_2_msg_vector(bits[b], M, K)
        ti, ts = sparc._msg_vector_indices(beta0, M, K)
        assert np.array_equal(idx[b], ti) and np.array_equal(sym[b], ts)
        assert np.array_equal(ref.word_bits(words[b], per), bits[b].astype(np.int64))
    beta0 = np.zeros((Bd, L * M), dtype=complex)
    beta0[np.arange(Bd)[:, None], np.arange(L) * M + idx] = ref.constel(K)[sym]
    assert np.max(np.abs(x - pipe.op.apply(beta0, False))) < 1e-9
    d = y - x
    assert abs(np.mean(np.abs(d) ** 2) - 1e-6) < 0.05e-6
    assert abs(d.real.var() - d.imag.var()) < 0.1e-6
    pipe.reset_counts()
    pipe.decode()
    cnt = pipe.counts()
    assert cnt[0] == Bd and not cnt[1:].any(), cnt
    # the same (seed, stream_id): identical buffers; another stream: another draw
    pipe.make_batch_device(Bd, 1e-6, 7, (3 << 32) | 5)
    for a, b in zip(state(), (idx, sym, info, unp, x, y, words)):
        assert np.array_equal(a, b)
    pipe.make_batch_device(Bd, 1e-6, 7, (3 << 32) | 6)
    assert not np.array_equal(state()[0], idx)


# ---------------------------------------------------------------- 7: sweep

def test_fft_sweep_does_not_depend_on_the_block_size(tmp_path):
    """2 points x 64 codewords, once in blocks of 32 and once in blocks of 64
    at the same seeds.  With the draws keyed in granules of 32 codewords
    (ConcatTrial's `granule`) each codeword's draw depends only on (seed,
    stream, index), so the counters are equal."""
    g = PIPE
    ebn0 = [1.0, 6.0]
    kw = dict(codewords=64, design_seed=PIPE_DESIGN_SEED, seed=4, t_max=15, bp_its=50, ldpc=g["ldpc"],
              precision="f64", design="fft", K=g["K"], granule=32)
    args = (g["L"], g["M"], PIPE_N, g["P"], g["L_unp"], g["mults"], ebn0)
    a = montecarlo.concat_ber_sweep(*args, block=32, checkpoint_dir=str(tmp_path), **kw)
    b = montecarlo.concat_ber_sweep(*args, block=64, **kw)
    ub = g["L_unp"] * 6 + 324
    for p in range(2):
        assert a[p]["codewords"] == b[p]["codewords"] == 64
        for k in ("ber", "fer", "unprotected_bit_errors", "protected_bit_errors", "awgn_var"):
            assert a[p][k] == b[p][k], (p, k)
        # complex noise: N0 = awgn_var, no factor 2
        assert abs(a[p]["awgn_var"] - g["P"] / ((ub / PIPE_N) * 10 ** (ebn0[p] / 10))) < 1e-12
    print([(o["ebn0_db"], o["ber"], o["fer"]) for o in a])
    assert a[0]["ber"] > 0 and a[1]["ber"] <= a[0]["ber"]  # (the noisy point has errors to compare)
    import os
    tag = montecarlo.concat_checkpoint_tag(g["L"], g["M"], PIPE_N, "fft", g["K"])
    assert tag == f"concat_fft_L112_M16_K4_n{PIPE_N}"
    assert sorted(os.listdir(tmp_path)) == [f"{tag}_pt0.json", f"{tag}_pt1.json"]
    with pytest.raises(NotImplementedError):
        montecarlo.concat_ber_sweep(*args, block=32, **dict(kw, precision="f32"))
