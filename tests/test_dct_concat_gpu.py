"""GPU tests of the soft output of the DCT-design AMP engines (sg_amp_llr_device,
amp_llr.hip) and of the concatenated SPARC + LDPC decoder built on it
(pipeline.DctConcatPipeline, concat_ber_sweep(design="dct")).

The yardstick is tests/dct_concat_ref.py: oracle.sparc_ref.amp (last beta and
MAP) -> beta_to_bit_probs -> clip / log -> oracle.bp.decode, per codeword.

Bars: bit probabilities against the oracle atol 1e-9 in double (the f64 parity
bar of test_amp_gpu.py) and 1e-3 in single precision at t_max = 4 (its f32 bar
for the first iterations); LLR against the clip / log of the same call's
probabilities rtol 1e-12 (f64) and 1e-5 (f32).

Operating points (chosen on the CPU with the oracle alone): awgn_var = 1 at
every small geometry decodes every section by t_max = 25 (all bit
probabilities hard) and leaves hundreds of them inside (0.01, 0.99) at
t_max = 4; the pipeline runs at awgn_var = 4, where the oracle composition has
error-free codewords and codewords with a few bit errors."""

import numpy as np
import pytest

import dct_concat_ref as ref
from ldpc_sparc_amd import _native, montecarlo, sparc
from ldpc_sparc_amd.pipeline import DctConcatPipeline
from oracle import sparc_ref
from sparc_cases import SPARC_CASES, design

pytestmark = pytest.mark.gpu

B = 6
VAR = 1.0
F64, F32 = _native.SG_F64, _native.SG_F32
ATOL = {F64: 1e-9, F32: 1e-3}
LLR_RTOL = {F64: 1e-12, F32: 1e-5}
# mixed stopping (chosen on the CPU): at rtol = 0.01 the oracle stops the flat design's codewords after 6, 6, 8,
# 22, 9 and 24 iterations, the noisy ones at stalled states with more than a hundred soft bit probabilities
MIXED_SIGMAS = [0.3, 1.0, 2.0, 2.4, 2.8, 3.2]


class Case:
    """One small geometry: its design, a batch of B received words, the GPU
    operator and the oracle's soft output per t_max (each computed once)."""

    def __init__(self, W, L, M, n, o0, o1, seed, sigmas=1.0, rtol=1e-6):
        self.W, self.L, self.M, self.n, self.o0, self.o1, self.rtol = W, L, M, n, o0, o1, rtol
        self.logM = int(np.log2(M))
        self.Ab, self.Az = sparc_ref.dct_operators(W, L, M, n, o0, o1)
        self.true, self.beta0, self.Y = ref.batch(self.Ab, L, M, n, B, sigmas, seed)
        self.op = sparc.DesignOperator(W, L, M, n, o0, o1)
        self._ref = {}

    def oracle(self, t_max):
        """(P(bit = 0) of every section [B, L log2 M], t_final [B])."""
        if t_max not in self._ref:
            res = [ref.amp_soft(self.Y[b], self.W, self.L, self.M, self.n, VAR, t_max, self.Ab, self.Az,
                                self.beta0[b], rtol=self.rtol) for b in range(B)]
            self._ref[t_max] = (np.stack([ref.bit_probs(r[0], self.L, self.M) for r in res]),
                                np.array([r[2] for r in res]))
        return self._ref[t_max]

    def oracle_moves(self, t_max):
        """The oracle's own conditioning: how far its probabilities of each
        codeword move when every received value moves by one ulp [B]."""
        want, _ = self.oracle(t_max)
        out = []
        for b in range(B):
            beta, _, _ = ref.amp_soft(np.nextafter(self.Y[b], np.inf), self.W, self.L, self.M, self.n, VAR, t_max,
                                      self.Ab, self.Az, self.beta0[b], rtol=self.rtol)
            out.append(np.max(np.abs(ref.bit_probs(beta, self.L, self.M) - want[b])))
        return np.array(out)

    def decode(self, t_max, prec, rows=slice(None)):
        Y = self.Y[rows]
        return sparc.amp_decode_batch(Y, self.op, VAR, t_max, rtol=self.rtol, true_idx=self.true[rows],
                                      precision=prec)


@pytest.fixture(scope="module")
def cases(sparc_golden):
    g = ref.SMALL
    L, M, n, P = g["L"], g["M"], g["n"], g["P"]
    made = {}

    def get(name):
        if name not in made:
            if name == "flat":
                made[name] = Case(np.array(P), L, M, n, *ref.flat_design(L, M, n, P, 3)[1:], seed=11)
            elif name == "pa":  # four column blocks of 28 sections, each with its own tau
                W, o0, o1 = ref.pa_design(L, M, n, P, 3)
                made[name] = Case(W, L, M, n, o0, o1, seed=11)
            elif name == "m16":  # lanes 16 .. 63 of every wavefront idle
                made[name] = Case(np.array(15.0), 32, 16, 128, *ref.flat_design(32, 16, 128, 15.0, 5)[1:], seed=13)
            elif name == "sc":  # omega = 2, Lambda = 4 of the golden set: the general four-step engine
                _, cp, _, var, _ = [c for c in SPARC_CASES if c[0] == "sc"][0]
                made[name] = Case(*design(sparc_golden, "sc", 0, cp, var), seed=14)
            elif name == "mixed":  # noise levels from clean to hopeless, all decoded at awgn_var = 1, rtol = 0.01
                made[name] = Case(np.array(P), L, M, n, *ref.flat_design(L, M, n, P, 3)[1:], seed=12,
                                  sigmas=MIXED_SIGMAS, rtol=1e-2)
            elif name == "mixed_pa":
                W, o0, o1 = ref.pa_design(L, M, n, P, 3)
                made[name] = Case(W, L, M, n, o0, o1, seed=12, sigmas=MIXED_SIGMAS, rtol=1e-2)
        return made[name]
    return get


def _engine(c, prec):
    return _native.lib().sg_amp_plan_engine(c.op.plan(prec), B)


# ---------------------------------------------------------------- 1, 2: probabilities against the oracle

@pytest.mark.parametrize("t_max", [25, 4])
@pytest.mark.parametrize("name", ["flat", "pa", "m16", "sc"])
def test_probs_f64_vs_oracle(cases, name, t_max):
    c = cases(name)
    want, tf_ref = c.oracle(t_max)
    if t_max == 4:  # the soft point is soft on the oracle's side
        assert np.count_nonzero((want > 0.01) & (want < 0.99)) >= 10
    _, tf, _, _ = c.decode(t_max, F64)
    assert _engine(c, F64) == (0 if name == "sc" else 1)
    got = sparc.amp_llr(c.op, B, 0, c.L, probs_only=True)
    assert np.array_equal(tf, tf_ref)
    print(f"{name} t_max={t_max} f64: max |p - oracle| = {np.max(np.abs(got - want)):.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL[F64])


@pytest.mark.parametrize("name", ["flat", "pa", "m16"])
def test_probs_f32_vs_oracle_soft_point(cases, name):
    c = cases(name)
    want, _ = c.oracle(4)
    assert np.count_nonzero((want > 0.01) & (want < 0.99)) >= 10
    c.decode(4, F32)
    got = sparc.amp_llr(c.op, B, 0, c.L, probs_only=True, precision=F32)
    print(f"{name} t_max=4 f32: max |p - oracle| = {np.max(np.abs(got - want)):.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL[F32])


# ---------------------------------------------------------------- 4: LLR = clip / log of the same probabilities

@pytest.mark.parametrize("t_max", [25, 4])
@pytest.mark.parametrize("name,prec", [("flat", F64), ("pa", F64), ("m16", F64), ("sc", F64),
                                       ("flat", F32), ("pa", F32), ("m16", F32)])
def test_llr_is_clip_log_of_probs(cases, name, t_max, prec):
    c = cases(name)
    c.decode(t_max, prec)
    p = sparc.amp_llr(c.op, B, 0, c.L, probs_only=True, precision=prec)
    llr = sparc.amp_llr(c.op, B, 0, c.L, precision=prec)
    want = ref.llr_of_probs(p)
    assert np.all(np.isfinite(llr))
    np.testing.assert_allclose(llr, want, rtol=LLR_RTOL[prec], atol=0)


# ---------------------------------------------------------------- 5: mixed stopping

@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", ["mixed", "mixed_pa"])
def test_mixed_stopping_reads_each_codewords_own_state(cases, name, prec):
    """Codewords that stop at different iterations: each one's soft output is
    that of its own single-codeword decode (the tau of another iteration, or
    later iterations of the others touching a stopped codeword's s or tau,
    would move every probability that is not hard), and in double precision
    the oracle's.

    The oracle is a 1e-9 yardstick only where AMP contracts.  At the stalled
    states of the hopeless codewords it does not: one ulp on the received
    values moves the oracle's own probabilities by 2e-8 to 6e-7 after 22 to 24
    iterations (the GPU's measured distance there is 2e-8 to 5e-7, its NMSE
    trajectory leaving the oracle's by a factor of about two per iteration from
    1e-16).  So the comparison with the oracle takes the codewords whose oracle
    output moves by less than 1e-10 under that one-ulp change -- at the flat
    design they include the two that stopped by themselves after 8 and 9
    iterations with more than 150 soft probabilities each; every codeword is
    compared with its own single-codeword decode."""
    c = cases(name)
    want, tf_ref = c.oracle(25)
    assert len(set(tf_ref.tolist())) >= 2, tf_ref
    soft = np.count_nonzero((want > 0.01) & (want < 0.99), axis=1)
    if name == "mixed":  # codewords that stopped early, by themselves, with soft probabilities
        assert np.count_nonzero((tf_ref < tf_ref.max()) & (soft >= 10)) >= 2, (tf_ref, soft)
    stable = c.oracle_moves(25) < 1e-10
    if name == "mixed":
        assert np.count_nonzero(stable & (tf_ref < tf_ref.max()) & (soft >= 10)) >= 2, (stable, tf_ref, soft)
    assert np.count_nonzero(stable) >= 2
    _, tf, _, _ = c.decode(25, prec)
    assert len(set(tf.tolist())) >= 2, tf
    got = sparc.amp_llr(c.op, B, 0, c.L, probs_only=True, precision=prec)
    for b in range(B):
        _, t1, _, _ = c.decode(25, prec, slice(b, b + 1))
        assert t1[0] == tf[b]
        one = sparc.amp_llr(c.op, 1, 0, c.L, probs_only=True, precision=prec)
        np.testing.assert_allclose(got[b], one[0], rtol=0, atol=ATOL[prec])
    if prec == F64:
        assert np.array_equal(tf, tf_ref)
        print(f"{name}: t_final {tf.tolist()}, max |p - oracle| per codeword = {np.max(np.abs(got - want), axis=1)}")
        np.testing.assert_allclose(got[stable], want[stable], rtol=0, atol=ATOL[F64])


# ---------------------------------------------------------------- 6, 7: ranges, stride, determinism

def _llr_device(c, prec, l0, nl, ld, probs_only=0, sentinel=None):
    dt = np.float64 if prec == F64 else np.float32
    host = np.full((B, ld), -777.0 if sentinel is None else sentinel, dt)
    buf = _native.DeviceBuffer.from_array(host)
    _native.check(_native.lib().sg_amp_llr_device(c.op.plan(prec), B, l0, nl, ld, probs_only, buf.ptr, None))
    _native.synchronize()
    return buf.download(host)


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", ["pa", "sc"])
def test_section_range_and_stride(cases, name, prec):
    c = cases(name)
    c.decode(4, prec)
    logM, L = c.logM, c.L
    l0, nl = 3, L - 5  # (pa: the range starts inside block 0 and ends inside block 3)
    whole = sparc.amp_llr(c.op, B, 0, L, precision=prec)
    ld = nl * logM + 7
    out = _llr_device(c, prec, l0, nl, ld)
    assert np.all(out[:, nl * logM:] == -777.0)  # the padding is untouched
    assert np.array_equal(out[:, :nl * logM].astype(np.float64), whole[:, l0 * logM:(l0 + nl) * logM])
    # two calls over disjoint ranges = one call over the union
    dt = out.dtype
    buf = _native.DeviceBuffer.from_array(np.full((B, ld), -777.0, dt))
    n1 = nl // 3
    lib, plan = _native.lib(), c.op.plan(prec)
    _native.check(lib.sg_amp_llr_device(plan, B, l0, n1, ld, 0, buf.ptr, None))
    _native.check(lib.sg_amp_llr_device(plan, B, l0 + n1, nl - n1, ld, 0,
                                        _native.offset(buf.ptr, n1 * logM * dt.itemsize), None))
    _native.synchronize()
    two = buf.download(np.empty((B, ld), dt))
    assert np.array_equal(two, out)
    # an empty range writes nothing
    assert np.all(_llr_device(c, prec, L, 0, 4) == -777.0)


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", ["flat", "sc"])
def test_bitwise_deterministic(cases, name, prec):
    c = cases(name)
    runs = []
    for _ in range(2):
        c.decode(4, prec)
        runs.append(sparc.amp_llr(c.op, B, 0, c.L, precision=prec))
    assert np.array_equal(runs[0], runs[1])


# ---------------------------------------------------------------- 8: bad arguments

def test_bad_arguments(cases):
    c = cases("flat")
    lib = _native.lib()
    logM, L = c.logM, c.L
    buf = _native.DeviceBuffer.from_array(np.full((B, L * logM), -777.0))
    fresh = sparc.DesignOperator(c.W, c.L, c.M, c.n, c.o0, c.o1)
    assert lib.sg_amp_llr_device(fresh.plan(F64), B, 0, L, L * logM, 0, buf.ptr, None) == _native.SG_ERR_BAD_ARG
    assert b"no decode" in lib.sg_last_error()
    c.decode(4, F64)
    plan = c.op.plan(F64)
    for args in ((B - 1, 0, L, L * logM),      # another batch size than the decode's
                 (B + 1, 0, L, L * logM),
                 (B, 1, L, L * logM),          # nl past L
                 (B, 0, L + 1, (L + 1) * logM),
                 (B, -1, 2, L * logM),
                 (B, 0, L, L * logM - 1)):     # short llr_ld
        assert lib.sg_amp_llr_device(plan, *args, 0, buf.ptr, None) == _native.SG_ERR_BAD_ARG, args
    _native.synchronize()
    assert np.all(buf.download(np.empty((B, L * logM))) == -777.0)  # nothing was launched
    assert lib.sg_amp_llr_device(plan, B, 0, L, L * logM, 0, buf.ptr, None) == _native.SG_OK
    # a decode of another batch size, or an operator application, invalidates the state
    c.decode(4, F64, slice(0, 2))
    assert lib.sg_amp_llr_device(plan, B, 0, L, L * logM, 0, buf.ptr, None) == _native.SG_ERR_BAD_ARG
    c.op.apply(c.beta0[:2], False)
    assert lib.sg_amp_llr_device(plan, 2, 0, L, L * logM, 0, buf.ptr, None) == _native.SG_ERR_BAD_ARG
    with pytest.raises(_native.NativeError):
        sparc.amp_llr(c.op, 2, 0, L)


def test_block_engine_plan_is_unsupported():
    """An f32 spatially coupled plan at w = 2^15 (the C4 geometry) runs the
    block engine, which keeps no soft output: SG_ERR_UNSUPPORTED, naming it."""
    M, P, omega, Lam, L = 512, 15.0, 6, 32, 1024
    W = sparc.sc_basic(np.array(P), omega, Lam)
    Lr, Lc = W.shape
    Mr = int(round(int(round(L * 9 / 1.5)) / Lr))
    o0, o1 = sparc.generate_ordering(W, Mr, L * M // Lc, 5)
    op = sparc.DesignOperator(W, L, M, Mr * Lr, o0, o1)
    lib = _native.lib()
    assert lib.sg_amp_plan_engine(op.plan(F32), 1) == 3
    buf = _native.DeviceBuffer(L * 9 * 4)
    assert lib.sg_amp_llr_device(op.plan(F32), 1, 0, L, L * 9, 0, buf.ptr, None) == _native.SG_ERR_UNSUPPORTED
    assert b"amp_block" in lib.sg_last_error()


# ---------------------------------------------------------------- 9: split engines (C2 geometry)

@pytest.mark.parametrize("prec", [F32, F64])
def test_split_engines_full_size(monkeypatch, prec):
    """L = 1024, M = 512, R = 1.3 (the only geometry with the split per-codeword
    engines): soft output after the split engine equals that after the staged
    engine on the same received words -- the same hard decisions of the
    protected bits, probabilities within the precision's bar -- and a decode
    without an override, which a batch of 2 runs on the companion plan (f32),
    is answered from the plan that ran."""
    L, M, R, Bc = 1024, 512, 1.3, 2
    Lu, nl = 160, 864
    n = int(round(L * 9 / R))
    W = np.array(15.0)
    o0, o1 = sparc.generate_ordering(W, n, L * M, 21)
    rng = np.random.default_rng(9)
    true = rng.integers(0, M, (Bc, L))
    beta0 = np.zeros((Bc, L * M))
    beta0[np.arange(Bc)[:, None], np.arange(L) * M + true] = 1
    out = {}
    Y = None
    for eng in ("cw", "staged", None):
        if eng:
            monkeypatch.setenv("SG_AMP_ENGINE", eng)
        else:
            monkeypatch.delenv("SG_AMP_ENGINE", raising=False)
        op = sparc.DesignOperator(W, L, M, n, o0, o1)
        if Y is None:
            Y = op.apply(beta0, False) + rng.standard_normal((Bc, n))
        mi, tf, _, _ = sparc.amp_decode_batch(Y, op, 1.0, 25, true_idx=true, precision=prec)
        last = _native.amp_last_decode(op.plan(prec))
        assert last["engine"] == (2 if eng == "cw" else 1), (eng, last)
        if eng is None:
            assert last["companion"] == (prec == F32)
        out[eng] = (sparc.amp_llr(op, Bc, Lu, nl, probs_only=True, precision=prec),
                    sparc.amp_llr(op, Bc, Lu, nl, precision=prec), mi)
    for eng in ("cw", None):
        assert np.array_equal(out[eng][1] < 0, out["staged"][1] < 0), eng
        print(f"{eng} vs staged prec={prec}: max |dp| = {np.max(np.abs(out[eng][0] - out['staged'][0])):.3e}")
        np.testing.assert_allclose(out[eng][0], out["staged"][0], rtol=0, atol=ATOL[prec])


# ---------------------------------------------------------------- 10: pipeline

def _pipe(precision, **kw):
    g = ref.SMALL
    return DctConcatPipeline(g["L"], g["M"], g["n"], g["P"], g["L_unp"], g["mults"], ldpc=g["ldpc"], design_seed=2,
                             precision=precision, **kw)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_pipeline_equals_per_codeword_composition(precision):
    g = ref.SMALL
    L, M, n, Lu, logM = g["L"], g["M"], g["n"], g["L_unp"], 6
    var = 4.0
    pipe = _pipe(precision)
    idx, info = pipe.make_batch(B, var, np.random.default_rng(1))
    pipe.reset_counts()
    pipe.decode()
    cnt = pipe.counts()
    Y = pipe.d_y.download(np.empty((B, n), pipe.dt)).astype(np.float64)
    op, c = pipe.op, pipe.c
    errs = cw_err = 0
    if precision == "f64":
        W = np.array(g["P"])
        o0, o1 = sparc.generate_ordering(W, n, L * M, 2)
        Ab, Az = sparc_ref.dct_operators(W, L, M, n, o0, o1)
    for b in range(B):
        if precision == "f64":  # the oracle's composition
            beta0 = np.zeros(L * M)
            beta0[np.arange(L) * M + idx[b]] = 1
            beta, mp, _ = ref.amp_soft(Y[b], W, L, M, n, var, 25, Ab, Az, beta0)
            bits = ref.decode_user_bits(beta, mp, L, M, Lu, c)
        else:  # the package's own steps, one codeword at a time
            mi, _, _, _ = sparc.amp_decode_batch(Y[b:b + 1], op, var, 25, precision=F32)
            llr = sparc.amp_llr(op, 1, Lu, L - Lu, precision=F32)
            app, _ = c.decode_batch(llr.reshape(-1, c.N), 200, "sumprod2", precision="f32")
            unp = ((mi[0, :Lu, None] >> np.arange(logM)[::-1]) & 1).reshape(-1)
            bits = np.concatenate([unp, (app[:, :c.K] < 0).astype(np.int64).reshape(-1)])
        e = int(np.sum(bits != ref.user_bits_truth(idx[b], info.reshape(B, -1)[b], Lu, logM)))
        errs += e
        cw_err += e > 0
    print(f"{precision}: counters {cnt.tolist()}, composition {errs} bit / {cw_err} codeword errors")
    assert cnt[0] == B
    assert cnt[1] == errs and cnt[2] == cw_err
    assert cnt[3] + cnt[4] == cnt[1]


def test_pipeline_device_batch():
    """make_batch_device on the DCT design: the draw depends only on (seed,
    stream_id), and the protected sections carry valid LDPC codewords of the
    drawn information words (as the dense pipeline's test checks)."""
    g = ref.SMALL
    L, n, Lu = g["L"], g["n"], g["L_unp"]
    pipe = _pipe("f32")
    c = pipe.c
    Bd, var = 32, 0.7
    pipe.make_batch_device(Bd, var, 7, (3 << 32) | 5)
    idx = pipe.d_true.download(np.zeros((Bd, L), np.int32))
    info = pipe.d_info.download(np.zeros((Bd, c.K), np.uint8))
    unp = pipe.d_unp.download(np.zeros((Bd, Lu * 6), np.uint8))
    bits = ((idx[:, :, None] >> np.arange(6)[::-1]) & 1).reshape(Bd, L * 6)
    assert np.array_equal(bits[:, :Lu * 6], unp)
    assert np.array_equal(bits[:, Lu * 6:], c.encode_batch(info.astype(np.int64)))
    x = pipe.d_x.download(np.zeros((Bd, n), np.float32)).astype(np.float64)
    y = pipe.d_y.download(np.zeros((Bd, n), np.float32)).astype(np.float64)
    beta0 = np.zeros((Bd, L * g["M"]))
    beta0[np.arange(Bd)[:, None], np.arange(L) * g["M"] + idx] = 1
    assert np.max(np.abs(x - pipe.op.apply(beta0, False))) < 1e-4  # x = A beta0 of the DCT design
    d = y - x
    assert abs(d.var() - var) < 0.05 * var and abs(d.mean()) < 0.02
    pipe.make_batch_device(Bd, var, 7, (3 << 32) | 5)
    assert np.array_equal(pipe.d_y.download(np.zeros((Bd, n), np.float32)), y.astype(np.float32))
    pipe.make_batch_device(Bd, var, 7, (3 << 32) | 6)
    assert not np.array_equal(pipe.d_true.download(np.zeros((Bd, L), np.int32)), idx)
    pipe.reset_counts()
    pipe.decode()
    assert pipe.counts()[0] == Bd


# ---------------------------------------------------------------- 11: sweep

def test_dct_sweep_rank_invariant(tmp_path):
    g = ref.SMALL
    L, M, n, P, Lu = g["L"], g["M"], g["n"], g["P"], g["L_unp"]
    ebn0 = [2.0, 8.0]
    kw = dict(codewords=32, block=16, design_seed=3, seed=4, t_max=10, bp_its=50, ldpc=g["ldpc"])
    ck = str(tmp_path)
    one = montecarlo.concat_ber_sweep(L, M, n, P, Lu, 1, ebn0, design="dct", checkpoint_dir=ck, **kw)
    # the same blocks dealt to two ranks, summed by hand
    pipe = DctConcatPipeline(L, M, n, P, Lu, 1, ldpc=g["ldpc"], design_seed=3, t_max=10, bp_its=50)
    ub = Lu * 6 + pipe.c.K
    for p, e in enumerate(ebn0):
        var = P / (2 * (ub / n) * 10 ** (e / 10))
        tr = montecarlo.ConcatTrial(pipe, [var] * 2, seed=4)
        shards = [montecarlo.shard_range(2, r, 2) for r in range(2)]
        a = sum(tr(p, lo, hi - lo, 16) for lo, hi in shards)
        assert int(a[0]) == one[p]["codewords"] == 32
        assert abs(float(a[1]) / (32 * ub) - one[p]["ber"]) < 1e-12
        assert int(a[2]) == round(one[p]["fer"] * 32)
    assert one[1]["ber"] <= one[0]["ber"]
    # its checkpoints carry their own tag and parameters: a dense sweep of the same geometry neither finds
    # nor resumes them
    import json
    import os
    tag = montecarlo.concat_checkpoint_tag(L, M, n, "dct")
    assert tag.startswith("concat_dct_L") and tag != montecarlo.concat_checkpoint_tag(L, M, n)
    names = sorted(os.listdir(ck))
    assert names == [f"{tag}_pt0.json", f"{tag}_pt1.json"]
    with open(os.path.join(ck, names[0])) as f:
        assert json.load(f)["params"]["design"] == "dct"
    os.rename(os.path.join(ck, names[0]), os.path.join(ck, montecarlo.concat_checkpoint_tag(L, M, n) + "_pt0.json"))
    with pytest.raises(ValueError, match="parameters"):
        montecarlo.concat_ber_sweep(L, M, n, P, Lu, 1, ebn0[:1], checkpoint_dir=ck, trial=lambda *a: None, **kw)
