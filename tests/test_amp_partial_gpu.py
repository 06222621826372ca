"""GPU tests of the AMP decode with known sections (sg_amp_decode_partial*,
amp_oploop.hip), the BP -> known-sections glue
(sg_concat_known_sections_device) and the three-stage concatenated decoder
built on them (pipeline.DctConcat3Pipeline).

The yardstick is tests/amp_partial_ref.py: sparc_ref.amp with known sections,
per codeword, and its composition with dct_concat_ref's AMP -> LLR -> BP.

Bars: in double precision map_idx and t_final equal and nmse / psi at atol 1e-9
(the f64 parity bar of test_amp_gpu.py) on every codeword whose restatement
moves by less than 1e-10 when the received values move by one ulp (the
oracle_moves device of test_dct_concat_gpu.py; at most one codeword of a batch
falls outside); in single precision map_idx on the codewords the restatement
decodes without a section error, and nmse at 1e-3 at t_max = 4 (the existing
f32 bar for the first iterations).

Inputs (chosen on the CPU with the restatement alone): the geometry of
amp_partial_ref.GEOM, a flat and a four-block power-allocated design, eight
codewords at noise sigma 1 to 2.2 decoded at awgn_var = 1, and per codeword
its own known set (amp_partial_ref.mixed_known): none, every protected
section, the same with one wrong index, and random subsets of all sections."""
import numpy as np
import pytest

import amp_partial_ref as pr
import dct_concat_ref as ref
import section_size_cases as ssc
from ldpc_sparc_amd import _native, montecarlo, sparc
from ldpc_sparc_amd.pipeline import DctConcat3Pipeline, DctConcatPipeline
from oracle import sparc_ref
from sparc_cases import SPARC_CASES, design

pytestmark = pytest.mark.gpu

B = 8
VAR = 1.0
SIGMAS = [1.0, 1.0, 1.5, 1.0, 1.7, 1.2, 2.2, 1.0]
F64, F32 = _native.SG_F64, _native.SG_F32
ATOL = {F64: 1e-9, F32: 1e-3}
G = pr.GEOM


class Case:
    """A design, a batch of B received words with a known set per codeword, the
    GPU operator and the restatement per t_max (each computed once)."""

    def __init__(self, W, L, M, n, o0, o1, seed, L_unp, sigmas=SIGMAS, nb=B):
        self.W, self.L, self.M, self.n = W, L, M, n
        self.Ab, self.Az = sparc_ref.dct_operators(W, L, M, n, o0, o1)
        self.true, self.beta0, self.Y = ref.batch(self.Ab, L, M, n, nb, sigmas, seed)
        self.known = pr.mixed_known(self.true, L_unp, M, seed + 1)
        self.none = np.full_like(self.known, -1)
        self.op = sparc.DesignOperator(W, L, M, n, o0, o1)
        self.nb = nb
        self._ref = {}

    def _run(self, Y, t_max, phi_method):
        res = [pr.amp_partial(Y[b], self.W, self.L, self.M, self.n, VAR, t_max, self.Ab, self.Az, self.beta0[b],
                              self.known[b], 1e-6, phi_method) for b in range(self.nb)]
        return (np.stack([r[0] for r in res]), np.array([r[1] for r in res]),
                np.stack([np.asarray(r[2]).reshape(t_max, -1) for r in res]),
                np.stack([np.atleast_1d(r[3]) for r in res]))

    def restatement(self, t_max, phi_method=1):
        """(map [B, L], t_final [B], nmse [B, t_max, Lc], psi [B, Lc])."""
        key = (t_max, phi_method)
        if key not in self._ref:
            self._ref[key] = self._run(self.Y, t_max, phi_method)
        return self._ref[key]

    def moves(self, t_max, phi_method=1):
        """How far the restatement's nmse and psi of each codeword move when
        every received value moves by one ulp [B]."""
        _, _, nm, ps = self.restatement(t_max, phi_method)
        _, _, nm1, ps1 = self._run(np.nextafter(self.Y, np.inf), t_max, phi_method)
        return np.maximum(np.max(np.abs(nm1 - nm), axis=(1, 2)), np.max(np.abs(ps1 - ps), axis=1))

    def decode(self, t_max, prec, known=None, rows=slice(None), phi_method=1):
        known = self.known if known is None else known
        return sparc.amp_decode_partial_batch(self.Y[rows], self.op, known[rows], VAR, t_max, true_idx=self.true[rows],
                                              phi_est_method=phi_method, precision=prec)


def make_case(name):
    L, M, n, P, Lu = G["L"], G["M"], G["n"], G["P"], G["L_unp"]
    if name == "flat":
        return Case(np.array(P), L, M, n, *ref.flat_design(L, M, n, P, 3)[1:], seed=21, L_unp=Lu)
    if name == "pa":  # four column blocks of 36 sections, each with its own tau and psi
        W, o0, o1 = ref.pa_design(L, M, n, P, 3)
        return Case(W, L, M, n, o0, o1, seed=21, L_unp=Lu)
    if name == "m16":  # lanes 16 .. 63 of every wavefront idle
        return Case(np.array(15.0), 32, 16, 128, *ref.flat_design(32, 16, 128, 15.0, 5)[1:], seed=13, L_unp=8,
                    sigmas=1.0)
    raise KeyError(name)


_made = {}


def case(name):
    if name not in _made:
        _made[name] = make_case(name)
    return _made[name]


# ---------------------------------------------------------------- against the restatement

@pytest.mark.parametrize("phi_method", [1, 2])
@pytest.mark.parametrize("name", ["flat", "pa"])
def test_f64_vs_restatement(name, phi_method):
    c = case(name)
    mp_r, tf_r, nm_r, ps_r = c.restatement(25, phi_method)
    stable = c.moves(25, phi_method) < 1e-10
    assert np.count_nonzero(~stable) <= 1, stable
    assert len(set(tf_r.tolist())) >= 3, tf_r  # codewords stop at different iterations
    mp, tf, nm, ps = c.decode(25, F64, phi_method=phi_method)
    err = np.maximum(np.max(np.abs(nm - nm_r), axis=(1, 2)), np.max(np.abs(ps - ps_r), axis=1))
    print(f"{name} phi {phi_method}: t_final {tf.tolist()}, stable {stable.tolist()}, max |nmse, psi - ref| {err}")
    assert np.array_equal(tf, tf_r)
    assert np.array_equal(mp, mp_r)
    np.testing.assert_allclose(nm[stable], nm_r[stable], rtol=0, atol=ATOL[F64])
    np.testing.assert_allclose(ps[stable], ps_r[stable], rtol=0, atol=ATOL[F64])
    # the known sections come back as given, the wrong one included
    kn = c.known >= 0
    assert np.array_equal(mp[kn], c.known[kn]) and mp[2, G["L_unp"] + 3] != c.true[2, G["L_unp"] + 3]


@pytest.mark.parametrize("name", ["flat", "pa"])
def test_f32_vs_restatement(name):
    c = case(name)
    mp_r, _, _, _ = c.restatement(25)
    clean = np.all((mp_r == c.true) | (c.known >= 0), axis=1)  # no section error outside the given (wrong) index
    assert np.count_nonzero(clean) >= 5, clean
    mp, _, _, _ = c.decode(25, F32)
    assert np.array_equal(mp[clean], mp_r[clean])
    _, _, nm_r, _ = c.restatement(4)
    _, _, nm, _ = c.decode(4, F32)
    print(f"{name} f32 t_max=4: max |nmse - ref| = {np.max(np.abs(nm - nm_r)):.3e}")
    np.testing.assert_allclose(nm, nm_r, rtol=0, atol=ATOL[F32])


# ---------------------------------------------------------------- all unknown = the plain decode

@pytest.mark.parametrize("name", ["flat", "pa", "m16"])
def test_all_unknown_is_the_plain_decode(name):
    c = case(name)
    # (without the hopeless codeword: two decoders pin its stalled state no better than the restatement does)
    rows = np.array(SIGMAS) < 2.0
    mi0, tf0, nm0, ps0 = sparc.amp_decode_batch(c.Y[rows], c.op, VAR, 25, true_idx=c.true[rows], precision=F64)
    mi, tf, nm, ps = c.decode(25, F64, known=c.none, rows=rows)
    assert len(set(tf0.tolist())) >= 2
    assert np.array_equal(mi, mi0) and np.array_equal(tf, tf0)
    print(f"{name}: max |psi - decode| = {np.max(np.abs(ps - ps0)):.3e}")
    np.testing.assert_allclose(ps, ps0, rtol=0, atol=1e-9)


# ---------------------------------------------------------------- section sizes

@pytest.mark.parametrize("name,t_max", [("m2", 3), ("m2048", 3), ("m2048", 25)])
def test_section_size_bounds(name, t_max):
    """M = 2 (62 idle lanes) and M = 2048 (32 entries per lane) at the
    section-size sweep's geometries, a known set per codeword, against the
    restatement in double precision."""
    s = ssc.case(name)
    known = pr.mixed_known(np.concatenate([s.true, s.true[2:]]), s.L // 2, s.M, 5)[[0, 1, 3]]
    op = sparc.DesignOperator(s.W, s.L, s.M, s.n, s.o0, s.o1)
    res = [pr.amp_partial(s.Y[b], s.W, s.L, s.M, s.n, ssc.VAR, t_max, s.Ab, s.Az, s.beta0[b], known[b])
           for b in range(ssc.B)]
    mp, tf, nm, ps = sparc.amp_decode_partial_batch(s.Y, op, known, ssc.VAR, t_max, true_idx=s.true, precision=F64)
    assert np.array_equal(tf, [r[1] for r in res])
    assert np.array_equal(mp, np.stack([r[0] for r in res]))
    np.testing.assert_allclose(nm[:, :, 0], np.stack([r[2] for r in res]), rtol=0, atol=ATOL[F64])
    mp32, _, _, _ = sparc.amp_decode_partial_batch(s.Y, op, known, ssc.VAR, t_max, precision=F32)
    assert np.array_equal(mp32[known >= 0], known[known >= 0])


def test_m4096_is_refused_before_any_launch():
    s = ssc.case("m4096")
    op = sparc.DesignOperator(s.W, s.L, s.M, s.n, s.o0, s.o1)
    lib, p = _native.lib(), _native.ptr
    known = np.full((ssc.B, s.L), -1, np.int32)
    mp, tf = np.full((ssc.B, s.L), -7, np.int32), np.full(ssc.B, -7, np.int32)
    nm, ps = np.full((ssc.B, 25, 1), -7.0), np.full((ssc.B, 1), -7.0)
    for prec in (F64, F32):
        rc = lib.sg_amp_decode_partial(op.plan(prec), p(s.Y), ssc.B, p(known), None, 1.0, 25, 1e-6, 1, p(mp), p(tf),
                                       p(nm), p(ps))
        assert rc == _native.SG_ERR_UNSUPPORTED and b"2048" in lib.sg_last_error()
    assert np.all(mp == -7) and np.all(tf == -7) and np.all(nm == -7) and np.all(ps == -7)


# ---------------------------------------------------------------- batch independence

@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", ["flat", "pa"])
def test_codeword_does_not_depend_on_its_batch(name, prec):
    c = case(name)
    whole = c.decode(25, prec)
    assert len(set(whole[1].tolist())) >= 3
    for b in (0, 2, 4, 7):
        one = c.decode(25, prec, rows=slice(b, b + 1))
        for w, o in zip(whole, one):
            assert np.array_equal(w[b], o[0]), (name, prec, b)


# ---------------------------------------------------------------- refusals and the plan's state

def test_spatially_coupled_plan_is_unsupported(sparc_golden):
    _, cp, _, var, _ = [c for c in SPARC_CASES if c[0] == "sc"][0]
    W, L, M, n, o0, o1 = design(sparc_golden, "sc", 0, cp, var)
    op = sparc.DesignOperator(W, L, M, n, o0, o1)
    with pytest.raises(_native.NativeError, match="spatially coupled"):
        sparc.amp_decode_partial_batch(np.zeros((2, n)), op, np.full((2, L), -1), 1.0, 5)
    lib = _native.lib()
    known = np.full((2, L), -1, np.int32)
    buf = _native.DeviceBuffer.from_array(np.zeros((2, n)))
    dk = _native.DeviceBuffer.from_array(known)
    assert lib.sg_amp_decode_partial_device(op.plan(F64), buf.ptr, 2, dk.ptr, None, 1.0, 5, 1e-6, 1, None, None, None,
                                            None, None) == _native.SG_ERR_UNSUPPORTED


def test_bad_arguments_and_plan_state():
    c = case("flat")
    lib, p = _native.lib(), _native.ptr
    before = sparc.amp_decode_batch(c.Y, c.op, VAR, 25, true_idx=c.true, precision=F64)
    llr = sparc.amp_llr(c.op, B, 0, c.L)
    # a known index outside [-1, M) is refused by the host variant, which scans the array
    for bad in (-2, c.M):
        known = c.known.copy()
        known[3, 7] = bad
        with pytest.raises(_native.NativeError, match="known_idx"):
            sparc.amp_decode_partial_batch(c.Y, c.op, known, VAR, 25)
    # ... and the refusal cleared the last-decode state, as every call of the entry point does
    with pytest.raises(_native.NativeError):
        sparc.amp_llr(c.op, B, 0, c.L)
    # B = 0 does nothing
    e = np.zeros(0)
    assert lib.sg_amp_decode_partial(c.op.plan(F64), p(e), 0, None, None, VAR, 25, 1e-6, 1, None, None, None,
                                     None) == _native.SG_OK
    # the device variant treats an index out of range as unknown
    known = c.known.copy()
    known[0, :] = c.M + 5
    known[3, 7] = -9
    want = c.known.copy()
    want[3, 7] = -1
    dt = np.float64
    d_y = _native.DeviceBuffer.from_array(c.Y.astype(dt))
    d_k = _native.DeviceBuffer.from_array(known)
    d_m = _native.DeviceBuffer(B * c.L * 4)
    _native.check(lib.sg_amp_decode_partial_device(c.op.plan(F64), d_y.ptr, B, d_k.ptr, None, VAR, 25, 1e-6, 1,
                                                   d_m.ptr, None, None, None, None))
    _native.synchronize()
    got = d_m.download(np.empty((B, c.L), np.int32))
    assert np.array_equal(got, c.decode(25, F64, known=want)[0])
    # soft output after a partial decode: no decode state
    assert lib.sg_amp_llr(c.op.plan(F64), B, 0, c.L, 0, p(np.empty_like(llr))) == _native.SG_ERR_BAD_ARG
    assert b"no decode" in lib.sg_last_error()
    # the plan is fit for a plain decode, which gives what it gave before
    after = sparc.amp_decode_batch(c.Y, c.op, VAR, 25, true_idx=c.true, precision=F64)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(sparc.amp_llr(c.op, B, 0, c.L), llr)


# ---------------------------------------------------------------- glue

def _known_device(prec, app, it, max_it, nb, mults, N, L, L_unp, logM):
    dt = np.float64 if prec == F64 else np.float32
    d_app = _native.DeviceBuffer.from_array(np.ascontiguousarray(app, dtype=dt))
    d_it = _native.DeviceBuffer.from_array(np.ascontiguousarray(it, dtype=np.int32))
    d_k = _native.DeviceBuffer.from_array(np.full((nb, L), -5, np.int32))
    _native.check(_native.lib().sg_concat_known_sections_device(prec, d_app.ptr, d_it.ptr, max_it, nb, mults, N, L,
                                                                L_unp, logM, d_k.ptr, None))
    _native.synchronize()
    return d_k.download(np.empty((nb, L), np.int32))


@pytest.mark.parametrize("prec", [F64, F32])
def test_known_sections_kernel(prec):
    rng = np.random.default_rng(8)
    # straddling: N = 20, logM = 8, two blocks per codeword, 5 protected sections in 40 bits, one unprotected
    N, logM, L_unp, L, mults, nb, max_it = 20, 8, 1, 6, 2, 3, 50
    app = rng.standard_normal((nb * mults, N))
    it = np.array([4, max_it, 7, max_it - 1, max_it, 0], dtype=np.int32)
    want = pr.known_sections(app, it, max_it, nb, mults, L, L_unp, logM)
    assert want[0].tolist()[3:] == [-1, -1, -1] and want[0, 1] >= 0 and np.all(want[1, 1:] >= 0)
    assert np.array_equal(_known_device(prec, app, it, max_it, nb, mults, N, L, L_unp, logM), want)
    # the real block: 648 bits = 108 sections of 6 bits behind 36 unprotected ones; codeword 1 unconverged
    N, logM, L_unp, L, mults, nb, max_it = 648, 6, G["L_unp"], G["L"], 1, 3, 200
    app = rng.standard_normal((nb, N))
    it = np.array([3, max_it, 199], dtype=np.int32)
    want = pr.known_sections(app, it, max_it, nb, mults, L, L_unp, logM)
    assert np.all(want[1] == -1) and np.all(want[0, L_unp:] >= 0) and np.all(want[:, :L_unp] == -1)
    assert np.array_equal(_known_device(prec, app, it, max_it, nb, mults, N, L, L_unp, logM), want)
    # sections that do not fit the blocks are refused
    lib = _native.lib()
    d = _native.DeviceBuffer(64)
    assert lib.sg_concat_known_sections_device(prec, d.ptr, d.ptr, 10, 1, 1, 20, 6, 1, 8, d.ptr,
                                               None) == _native.SG_ERR_BAD_ARG


# ---------------------------------------------------------------- pipeline

def _pipe(cls, precision, **kw):
    return cls(G["L"], G["M"], G["n"], G["P"], G["L_unp"], G["mults"], ldpc=G["ldpc"], design_seed=pr.DESIGN_SEED,
               precision=precision, **kw)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_pipeline_at_the_operating_point(precision):
    """The operating point of tests/test_amp_partial_host.py with host-made
    batches: in double precision the five counters are the restatement's on
    the received words the pipeline holds; in either precision the
    unprotected-bit counter is strictly below the two-stage pipeline's on the
    same batch."""
    L, M, n, Lu, logM = G["L"], G["M"], G["n"], G["L_unp"], 6
    nb = pr.B_POINT
    cnt = {}
    for cls in (DctConcatPipeline, DctConcat3Pipeline):
        pipe = _pipe(cls, precision)
        idx, info = pipe.make_batch(nb, pr.VAR, np.random.default_rng(pr.BATCH_SEED))
        pipe.reset_counts()
        pipe.decode()
        cnt[cls] = pipe.counts()
    two, three = cnt[DctConcatPipeline], cnt[DctConcat3Pipeline]
    print(f"{precision}: two-stage {two.tolist()}, three-stage {three.tolist()}")
    assert np.array_equal(idx, pr.point()["idx"])  # the host test's batch
    assert three[0] == nb and three[3] + three[4] == three[1]
    assert three[4] == two[4]  # the same BP output counts the protected bits
    assert three[3] < two[3]
    if precision == "f64":
        Y = pipe.d_y.download(np.empty((nb, n), pipe.dt))
        pt = pr.point()
        want2, want3 = np.zeros(5, np.int64), np.zeros(5, np.int64)
        for b in range(nb):
            r = pr.three_stage(Y[b], pt["W"], L, M, n, pr.VAR, 25, pt["Ab"], pt["Az"], pt["beta0"][b], Lu, pt["c"])
            want2 += pr.counters(r["map2"], idx[b], r["app"], info[b], Lu, logM, pipe.c.K)
            want3 += pr.counters(r["map3"], idx[b], r["app"], info[b], Lu, logM, pipe.c.K)
        print(f"restatement: two-stage {want2.tolist()}, three-stage {want3.tolist()}")
        assert np.array_equal(two, want2)
        assert np.array_equal(three, want3)


def test_pipeline_device_batches_rank_invariant():
    """make_batch_device through ConcatTrial: the counters of four blocks are
    the same decoded by one rank and dealt to two (the Philox key of a block
    is (seed, point, block)), and final_t_max reaches the last pass."""
    pipe = _pipe(DctConcat3Pipeline, "f32", final_t_max=12)
    assert pipe.final_t_max == 12 and _pipe(DctConcat3Pipeline, "f32").final_t_max == 25
    tr = montecarlo.ConcatTrial(pipe, [pr.VAR], seed=4)
    one = tr(0, 0, 4, 8)
    shards = [montecarlo.shard_range(4, r, 2) for r in range(2)]
    split = sum(tr(0, lo, hi - lo, 8) for lo, hi in shards)
    assert int(one[0]) == 32 and np.array_equal(one, split)
    assert one[3] + one[4] == one[1]
