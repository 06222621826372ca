"""GPU tests of the soft output of the real K = 2 (BPSK) AMP decoder
(sg_amp_bpsk_soft_output, sg_amp_bpsk_llr*, amp_bpsk_llr.hip) and of the
concatenated K = 2 SPARC + LDPC decoder built on it
(pipeline.DctBpskConcatPipeline, concat_ber_sweep(design="dct", K=2)).

The yardstick is tests/bpsk_concat_ref.py: the restated K = 2 AMP loop (last s
and tau) -> the joint posterior over (location, sign) by enumeration -> clip /
log -> oracle.bp.decode, per codeword.  tests/test_bpsk_concat_host.py holds
it against the reference's denoiser and asserts, on the restatement alone,
that the cases below are soft and stable.

Bars (those of sg_amp_llr, test_dct_concat_gpu.py): in double precision words
and t_final equal, bit probabilities atol 1e-9, LLR against the clip / log of
the same call's probabilities rtol 1e-12; in single precision at t_max = 4
probabilities atol 1e-3 and LLR rtol 1e-5.  A codeword whose restatement
output moves by more than the bar when every received value moves by one ulp
is left out of the comparison with the restatement (at most one per case, two
of eight at the pipeline's operating points)."""
import numpy as np
import pytest

import amp_bpsk_ref as br
import bpsk_concat_ref as ref
import section_size_cases as ssc
from bpsk_cases import AWGN_VAR, BPSK_CASES, code_params, design, golden
from ldpc_sparc_amd import _native, montecarlo, sparc
from ldpc_sparc_amd.pipeline import DctBpskConcatPipeline

pytestmark = pytest.mark.gpu

F64, F32 = _native.SG_F64, _native.SG_F32
ATOL = {F64: 1e-9, F32: 1e-3}
LLR_RTOL = {F64: 1e-12, F32: 1e-5}


class Case:
    """One design with a batch of received words: the GPU operator, the CPU
    operators and the restatement's soft output per t_max (each computed once)."""

    def __init__(self, W, L, M, n, o0, o1, Y, words, ops, var=1.0, rtol=1e-6, phi_method=1):
        self.W, self.L, self.M, self.n, self.Y, self.words, self.ops = W, L, M, n, Y, words, ops
        self.var, self.rtol, self.phi_method = var, rtol, phi_method
        self.B, self.per = len(Y), int(np.log2(M)) + 1
        self.op = sparc.DesignOperator(W, L, M, n, o0, o1)
        self._ref = {}

    def _soft(self, y, t_max):
        return ref.amp_bpsk_soft(y, self.W, self.L, self.M, self.n, self.var, t_max, *self.ops, rtol=self.rtol,
                                 phi_method=self.phi_method)

    def restated(self, t_max, prec=F64):
        """(P(bit = 0) [B, L per], words [B, L], t_final [B], stable [B]): stable where the restatement's own
        probabilities move by no more than the precision's bar under a one-ulp change of y."""
        if t_max not in self._ref:
            sts = [self._soft(y, t_max) for y in self.Y]
            p = np.stack([ref.soft_probs(st, self.M).reshape(-1) for st in sts])
            moved = np.array([np.abs(ref.soft_probs(self._soft(np.nextafter(y, np.inf), t_max), self.M).reshape(-1)
                                     - p[b]).max() for b, y in enumerate(self.Y)])
            self._ref[t_max] = (p, np.stack([st["words"] for st in sts]), np.array([st["t_final"] for st in sts]),
                                moved)
        p, w, tf, moved = self._ref[t_max]
        return p, w, tf, moved <= ATOL[prec]

    def decode(self, t_max, prec, rows=slice(None), soft=True):
        self.op.soft_output(soft, prec)
        return sparc.amp_decode_bpsk_batch(self.Y[rows], self.op, self.var, t_max, self.rtol, self.phi_method,
                                           self.words[rows], prec)

    def probs(self, prec, B=None, l0=0, nl=None):
        return sparc.amp_llr_bpsk(self.op, self.B if B is None else B, l0, self.L if nl is None else nl,
                                  probs_only=True, precision=prec)

    def llr(self, prec, B=None):
        return sparc.amp_llr_bpsk(self.op, self.B if B is None else B, 0, self.L, precision=prec)


_cases = {}


def golden_case(name):
    if name not in _cases:
        _, cp, dp, _ = [c for c in BPSK_CASES if c[0] == name][0]
        g = golden()
        W, L, M, n, o0, o1 = design(g, name, code_params(cp))
        ops = br.operators(W, L, M, n, o0, o1)
        Y, tw = ref.golden_batch(g, name, cp, ops)
        _cases[name] = Case(W, L, M, n, o0, o1, Y, tw, ops, AWGN_VAR, 1e-6, dp.get('phi_est_method', 1))
        _cases[name].t_max = dp['t_max']
    return _cases[name]


def size_case(name):
    if name not in _cases:
        W, L, M, n, o0, o1, words, Y, ops = ref.size_case(name)
        _cases[name] = Case(W, L, M, n, o0, o1, Y, words, ops)
    return _cases[name]


def _check_soft_output(c, t_max, prec, label):
    want, w_ref, tf_ref, stable = c.restated(t_max, prec)
    assert np.count_nonzero(~stable) <= 1, stable
    mw, tf, _, _ = c.decode(t_max, prec)
    p, llr = c.probs(prec), c.llr(prec)
    print(f"{label} t_max={t_max} prec={prec}: max |p - restatement| = {np.abs(p - want)[stable].max():.3e}, "
          f"t_final {tf.tolist()}, left out {np.count_nonzero(~stable)}")
    if prec == F64:
        assert np.array_equal(tf[stable], tf_ref[stable]) and np.array_equal(mw[stable], w_ref[stable])
    np.testing.assert_allclose(p[stable], want[stable], rtol=0, atol=ATOL[prec])
    assert np.all(np.isfinite(llr))
    np.testing.assert_allclose(llr, ref.llr_of_probs(p), rtol=LLR_RTOL[prec], atol=0)


# ---------------------------------------------------------------- soft output after a decode

NAMES = [c[0] for c in BPSK_CASES]


@pytest.mark.parametrize("own", [False, True], ids=["t3", "own"])
@pytest.mark.parametrize("name", NAMES)
def test_f64_golden_designs(name, own):
    c = golden_case(name)
    _check_soft_output(c, c.t_max if own else 3, F64, name)


@pytest.mark.parametrize("name", NAMES)
def test_f32_golden_designs(name):
    _check_soft_output(golden_case(name), 4, F32, name)


# ---------------------------------------------------------------- section sizes

@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", list(ref.SIZES) + ["pa256"])
def test_section_sizes(name, prec):
    _check_soft_output(size_case(name), ref.SIZE_TMAX if prec == F64 else 4, prec, name)


# ---------------------------------------------------------------- contract

def _llr_device(c, prec, B, l0, nl, ld, probs_only=0):
    dt = np.float64 if prec == F64 else np.float32
    host = np.full((B, ld), -777.0, dt)
    buf = _native.DeviceBuffer.from_array(host)
    rc = _native.lib().sg_amp_bpsk_llr_device(c.op.plan(prec), B, l0, nl, ld, probs_only, buf.ptr, None)
    _native.synchronize()
    return rc, buf.download(host)


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", ["pa256", "bsc"])
def test_section_range_and_stride(name, prec):
    c = size_case(name) if name == "pa256" else golden_case(name)
    c.decode(3, prec)
    per, L = c.per, c.L
    whole = c.llr(prec)
    l0, nl = 1, L - 2
    rc, out = _llr_device(c, prec, c.B, l0, nl, nl * per + 3)
    assert rc == _native.SG_OK
    assert np.all(out[:, nl * per:] == -777.0)  # nothing else is written
    assert np.array_equal(out[:, :nl * per].astype(np.float64), whole[:, l0 * per:(l0 + nl) * per])
    rc, out = _llr_device(c, prec, c.B, L, 0, 4)  # an empty range writes nothing
    assert rc == _native.SG_OK and np.all(out == -777.0)


@pytest.mark.parametrize("prec", [F64, F32])
def test_codeword_alone_and_two_runs_are_bit_identical(prec):
    c = size_case("m128")
    runs = []
    for _ in range(2):
        c.decode(3, prec)
        runs.append((c.probs(prec), c.llr(prec)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    c.decode(3, prec, slice(1, 2))
    assert np.array_equal(c.probs(prec, B=1)[0], runs[0][0][1])
    assert np.array_equal(c.llr(prec, B=1)[0], runs[0][1][1])


SIGMAS = [0.5, 1.0, 2.5, 1.0, 2.0, 1.5, 2.2, 0.8]
_mixed = {}


def mixed_case():
    """breg's design with eight codewords at noise sigma 0.5 to 2.5, decoded at awgn_var = 1 and rtol = 0.05
    (chosen on the CPU): the restatement stops them after 5, 8, 7, 7, 12, 9, 23 and 6 iterations, codewords 2 and 4
    at stalled states with 170 and 110 soft probabilities, where the tau of another iteration, or a later iteration
    of the others touching their s, would show."""
    if not _mixed:
        c0 = golden_case("breg")
        rng = np.random.RandomState(41)
        tw = rng.randint(0, 2 * c0.M, (8, c0.L)).astype(np.int32)
        X = np.stack([c0.ops[0](br.beta_of_words(w, c0.M)) for w in tw])
        Y = X + np.array(SIGMAS)[:, None] * rng.randn(8, c0.n)
        op = c0.op
        _mixed["c"] = Case(c0.W, c0.L, c0.M, c0.n, op.order0[0], op.order1[0], Y, tw, c0.ops, rtol=0.05)
    return _mixed["c"]


def test_early_stops_keep_each_codewords_own_state():
    c = mixed_case()
    want, _, tf_ref, stable = c.restated(25)
    soft = np.count_nonzero((want > 0.01) & (want < 0.99), axis=1)
    assert len(set(tf_ref.tolist())) >= 3
    assert np.count_nonzero(stable & (tf_ref < tf_ref.max()) & (soft >= 10)) >= 2 and np.count_nonzero(stable) >= 6
    _, tf, _, _ = c.decode(25, F64)
    p = c.probs(F64)
    print("t_final", tf.tolist(), "stable", stable.tolist(), "max |p - restatement| per codeword",
          np.abs(p - want).max(axis=1))
    assert np.array_equal(tf[stable], tf_ref[stable])
    np.testing.assert_allclose(p[stable], want[stable], rtol=0, atol=ATOL[F64])
    for b in (2, 6):  # an early and a late stop at soft states: each its own single-codeword decode, bit for bit
        _, t1, _, _ = c.decode(25, F64, slice(b, b + 1))
        assert t1[0] == tf[b] and np.array_equal(c.probs(F64, B=1)[0], p[b])


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", ["m2048", "bsc"])
def test_decode_outputs_do_not_depend_on_the_switch(name, prec):
    c = size_case(name) if name == "m2048" else golden_case(name)
    off = c.decode(5, prec, soft=False)
    on = c.decode(5, prec, soft=True)
    for a, b in zip(off, on):
        assert a.tobytes() == b.tobytes()


def test_refusals():
    c = size_case("m64")
    lib, B, L, per = _native.lib(), c.B, c.L, c.per
    BAD = _native.SG_ERR_BAD_ARG
    fresh = sparc.DesignOperator(c.W, c.L, c.M, c.n, c.op.order0[0], c.op.order1[0])
    buf = _native.DeviceBuffer.from_array(np.full((B, L * per), -777.0))

    def call(op, *args):
        return lib.sg_amp_bpsk_llr_device(op.plan(F64), *args, 0, buf.ptr, None)
    assert call(fresh, B, 0, L, L * per) == BAD and b"soft output is off" in lib.sg_last_error()
    fresh.soft_output(True)
    assert call(fresh, B, 0, L, L * per) == BAD and b"no K = 2 decode" in lib.sg_last_error()
    c.decode(3, F64, soft=False)  # soft output off: nothing on record
    assert call(c.op, B, 0, L, L * per) == BAD
    c.decode(3, F64)
    out = np.zeros((B, L * (per - 1)))
    assert lib.sg_amp_llr(c.op.plan(F64), B, 0, L, 0, _native.ptr(out)) == BAD  # sg_amp_llr* keeps refusing
    for args in ((B - 1, 0, L, L * per), (B + 1, 0, L, L * per), (B, 1, L, L * per), (B, 0, L + 1, (L + 1) * per),
                 (B, -1, 2, L * per), (B, 0, L, L * per - 1)):
        assert call(c.op, *args) == BAD, args
    _native.synchronize()
    assert np.all(buf.download(np.empty((B, L * per))) == -777.0)  # nothing was launched
    assert call(c.op, B, 0, L, L * per) == _native.SG_OK
    # an unmodulated decode, an operator application or switching off clears the record
    sparc.amp_decode_batch(c.Y, c.op, 1.0, 3)
    assert call(c.op, B, 0, L, L * per) == BAD
    c.decode(3, F64)
    c.op.apply(np.zeros((1, c.L * c.M)), False)
    assert call(c.op, B, 0, L, L * per) == BAD
    c.decode(3, F64)
    c.op.soft_output(False)
    assert call(c.op, B, 0, L, L * per) == BAD
    with pytest.raises(_native.NativeError):
        sparc.amp_llr_bpsk(c.op, B, 0, L)
    s = ssc.case("m4096")
    big = sparc.DesignOperator(s.W, s.L, s.M, s.n, s.o0, s.o1)
    assert lib.sg_amp_bpsk_llr_device(big.plan(F64), 1, 0, 1, 13, 0, buf.ptr, None) == _native.SG_ERR_UNSUPPORTED
    assert b"4096" in lib.sg_last_error()


# ---------------------------------------------------------------- pipeline

def _pipe(name, precision, **kw):
    L, M, Lu, mults, n, var = ref.POINTS[name]
    return DctBpskConcatPipeline(L, M, n, ref.P, Lu, mults, ldpc=ref.LDPC, design_seed=0, precision=precision, **kw)


_point_ref = {}


def point_restated(name, Y, words, info):
    """Per codeword of the batch the pipeline drew: (user bits, protected LLRs, stable), and the truth."""
    if name not in _point_ref:
        from oracle import sparc_ref
        L, M, Lu, mults, n, var = ref.POINTS[name]
        W, o0, o1 = ref.flat_design(L, M, n, ref.P, 0)
        ops = sparc_ref.dct_operators(W, L, M, n, o0, o1)
        c = Case(W, L, M, n, o0, o1, Y, words, ops, var)
        _, _, _, stable = c.restated(25)
        from ldpc_sparc_amd.ldpc import code
        lc = code(*ref.LDPC)
        dec = [ref.decode_user_bits(c._soft(y, 25), L, M, Lu, lc) for y in Y]
        truth = np.stack([ref.user_bits_truth(words[b], info.reshape(len(Y), -1)[b], Lu, c.per) for b in range(len(Y))])
        _point_ref[name] = (np.stack([d[0] for d in dec]), np.stack([d[2] for d in dec]), stable, truth)
    return _point_ref[name]


@pytest.mark.parametrize("name", ["A", "B"])
def test_pipeline_f64_equals_the_restatement(name):
    L, M, Lu, mults, n, var = ref.POINTS[name]
    B = ref.PIPE_B
    pipe = _pipe(name, "f64")
    words, info = pipe.make_batch(B, var, np.random.default_rng(1))
    assert np.array_equal(words, ref.point_batch(name)[0])
    Y = pipe.d_y.download(np.empty((B, n)))
    bits, llr_ref, stable, truth = point_restated(name, Y, words, info)
    assert np.count_nonzero(~stable) <= 2
    keep = np.nonzero(stable)[0]
    # the kept codewords as the pipeline's batch
    pipe.d_y.upload(Y[keep])
    pipe.d_true.upload(words[keep])
    pipe.d_info.upload(info.reshape(B, -1)[keep].astype(np.uint8))
    pipe.B = len(keep)
    pipe.reset_counts()
    pipe.decode()
    cnt = pipe.counts()
    want = ref.counters(bits[keep], truth[keep], Lu * pipe.bits_per_section)
    llr = pipe.d_llr.download(np.empty((len(keep), mults * pipe.c.N)))
    dp = np.abs(1 / (1 + np.exp(-llr)) - 1 / (1 + np.exp(-llr_ref[keep]))).max()
    print(f"point {name} f64: counters {cnt.tolist()}, restatement {want.tolist()}, kept {len(keep)} of {B}, "
          f"max |p - restatement| of the protected bits {dp:.3e}")
    assert np.array_equal(cnt, want)
    assert dp <= ATOL[F64]


@pytest.mark.parametrize("name", ["A", "B"])
def test_pipeline_f32_runs(name):
    L, M, Lu, mults, n, var = ref.POINTS[name]
    pipe = _pipe(name, "f32")
    pipe.make_batch(ref.PIPE_B, var, np.random.default_rng(1))
    pipe.reset_counts()
    pipe.decode()
    cnt = pipe.counts()
    print(f"point {name} f32: counters {cnt.tolist()}")
    assert cnt[0] == ref.PIPE_B and cnt[3] + cnt[4] == cnt[1]


def test_pipeline_device_batch():
    """make_batch_device: words of log2 M + 1 bits, valid LDPC codewords in
    the protected sections, the draw of codeword b a function of (seed,
    stream_id, b) alone -- the same at another batch size."""
    L, M, Lu, mults, n, var = ref.POINTS["A"]
    pipe = _pipe("A", "f64")
    c, per = pipe.c, pipe.bits_per_section
    got = {}
    for Bd in (8, 4, 8):
        pipe.make_batch_device(Bd, var, 7, (3 << 32) | 5)
        _native.synchronize()
        rows = (pipe.d_true.download(np.zeros((Bd, L), np.int32)), pipe.d_info.download(np.zeros((Bd, c.K), np.uint8)),
                pipe.d_y.download(np.zeros((Bd, n))))
        if Bd in got:
            assert all(np.array_equal(a, b) for a, b in zip(rows, got[Bd]))
        got[Bd] = rows
    assert all(np.array_equal(a[:4], b) for a, b in zip(got[8], got[4]))
    words, info, y = got[8]
    assert words.max() < 2 * M and words.max() >= M and words.min() >= 0
    bits = ref.word_bits(words, per).reshape(8, L * per)
    assert np.array_equal(bits[:, Lu * per:], c.encode_batch(info.astype(np.int64)))
    x = np.stack([br.operators(*_flat("A"))[0](br.beta_of_words(w, M)) for w in words[:2]])
    d = y[:2] - x
    assert abs(d.var() - var) < 0.15 * var
    pipe.reset_counts()
    pipe.decode()
    assert pipe.counts()[0] == 8


def _flat(name):
    L, M, Lu, mults, n, var = ref.POINTS[name]
    W, o0, o1 = ref.flat_design(L, M, n, ref.P, 0)
    return W, L, M, n, o0, o1


def test_k2_sweep_does_not_depend_on_the_block(tmp_path):
    L, M, Lu, mults, n, var = ref.POINTS["A"]
    kw = dict(codewords=16, design_seed=0, seed=4, t_max=10, bp_its=50, ldpc=ref.LDPC, precision="f64", design="dct",
              K=2, granule=8)
    a = montecarlo.concat_ber_sweep(L, M, n, ref.P, Lu, mults, [5.0], block=8, **kw)  # (no checkpoints)
    b = montecarlo.concat_ber_sweep(L, M, n, ref.P, Lu, mults, [5.0], block=16, checkpoint_dir=str(tmp_path), **kw)
    print("K = 2 sweep:", a[0])
    assert a[0]["codewords"] == b[0]["codewords"] == 16
    for k in ("ber", "fer", "unprotected_bit_errors", "protected_bit_errors", "awgn_var"):
        assert a[0][k] == b[0][k], k
    assert (tmp_path / f"concat_dct_k2_L{L}_M{M}_n{n}_pt0.json").exists()


def test_spatially_coupled_design_through_the_pipeline():
    """bsc's base matrix (omega = 2, Lambda = 4) at L = 128, M = 32: 108 protected sections of 6 bits."""
    L, M, Lu, n = 128, 32, 20, 700
    W = sparc.sc_basic(np.array(ref.P), 2, 4)
    Lr, Lc = W.shape
    o0, o1 = sparc.generate_ordering(W, n // Lr, L * M // Lc, 5)
    op = sparc.DesignOperator(W, L, M, n, o0, o1)
    pipe = DctBpskConcatPipeline(L, M, n, ref.P, Lu, 1, ldpc=ref.LDPC, precision="f64", op=op)
    pipe.make_batch(4, 1.0, np.random.default_rng(2))
    pipe.reset_counts()
    pipe.decode()
    cnt = pipe.counts()
    print("spatially coupled K = 2 pipeline: counters", cnt.tolist())
    assert cnt[0] == 4 and cnt[3] + cnt[4] == cnt[1]
