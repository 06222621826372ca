"""GPU tests of the complex AMP decode with known sections
(sg_camp_decode_partial*: the complex engine's own kernels, amp_cfft.hip, with
CampBufs::known_idx given), the section-word unpacker
(sg_psk_unpack_sections_device) and the three-stage concatenated K-PSK decoder
built on them (pipeline.CsparcConcat3Pipeline).

The yardstick is tests/camp_partial_ref.py: csparc_ref.amp with known sections,
per codeword, and its composition with csparc_concat_ref's AMP -> LLR -> BP.

Bars (those of test_amp_partial_gpu.py): locations, symbols and t_final equal
and nmse / psi at atol 1e-9 (the f64 parity bar of the suite) on every codeword
whose restatement moves by less than 1e-10 when the received values move by
one ulp; at most one codeword of a batch falls outside.

Inputs (chosen on the CPU with the restatement alone): the golden complex
designs and two flat ones, eight codewords at noise sigma 1 to 2.2 decoded at
awgn_var = 1, and per codeword its own known set
(camp_partial_ref.mixed_known): none, every protected section, the same with
one wrong location, the same with one wrong symbol, random subsets."""
import numpy as np
import pytest

import camp_partial_ref as pr
import csparc_cases as cc
import csparc_concat_ref as cref
import csparc_ref
from ldpc_sparc_amd import _native, montecarlo, sparc
from ldpc_sparc_amd.pipeline import CsparcConcat3Pipeline, CsparcConcatPipeline

pytestmark = pytest.mark.gpu

B = 8
VAR = 1.0
SIGMAS = [1.0, 1.0, 1.5, 1.0, 1.7, 1.2, 2.2, 1.0]
ATOL = 1e-9
G = pr.GEOM


class Case:
    """A design, a batch of received words with a known set per codeword, the
    GPU operator and the restatement per (t_max, phi_method), each computed once."""

    def __init__(self, W, L, M, n, K, o0, o1, seed, L_unp, sigmas=SIGMAS, nb=B):
        self.W, self.L, self.M, self.n, self.K, self.nb = np.asarray(W, dtype=float), L, M, n, K, nb
        self.Ab, self.Az = csparc_ref.fft_operators(W, L, M, n, o0, o1)
        rng = np.random.RandomState(seed)
        self.idx = rng.randint(0, M, (nb, L)).astype(np.int32)
        self.sym = rng.randint(0, K, (nb, L)).astype(np.int32)
        self.beta0 = pr.one_hots(self.idx, self.sym, M, K)
        noise = (rng.randn(nb, n) + 1j * rng.randn(nb, n)) / np.sqrt(2)
        sig = np.broadcast_to(np.asarray(sigmas, dtype=float), (nb,))
        self.Y = np.stack([self.Ab(b).reshape(n) for b in self.beta0]) + sig[:, None] * noise
        self.kidx, self.ksym = pr.mixed_known(self.idx, self.sym, L_unp, M, K, seed + 1)
        self.L_unp = L_unp
        self.o0, self.o1 = o0, o1
        self._op, self._ref = None, {}

    @property
    def op(self):
        if self._op is None:
            self._op = sparc.ComplexDesignOperator(self.W, self.L, self.M, self.n, self.o0, self.o1)
        return self._op

    def _run(self, Y, t_max, phi_method):
        res = [pr.amp_partial(Y[b], self.W, self.L, self.M, self.n, self.K, self.Ab, self.Az, VAR, t_max,
                              self.beta0[b], self.kidx[b], self.ksym[b], 1e-6, phi_method) for b in range(self.nb)]
        return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res]),
                np.stack([np.asarray(r[3]).reshape(t_max, -1) for r in res]),
                np.stack([np.atleast_1d(r[4]) for r in res]))

    def restatement(self, t_max, phi_method=1):
        """(map_idx, map_sym [B, L], t_final [B], nmse [B, t_max, Lc], psi [B, Lc])."""
        key = (t_max, phi_method)
        if key not in self._ref:
            self._ref[key] = self._run(self.Y, t_max, phi_method)
        return self._ref[key]

    def moves(self, t_max, phi_method=1):
        """How far the restatement's nmse and psi of each codeword move when
        every received value moves by one ulp [B]."""
        _, _, _, nm, ps = self.restatement(t_max, phi_method)
        Y1 = np.nextafter(self.Y.real, np.inf) + 1j * np.nextafter(self.Y.imag, np.inf)
        _, _, _, nm1, ps1 = self._run(Y1, t_max, phi_method)
        return np.maximum(np.max(np.abs(nm1 - nm), axis=(1, 2)), np.max(np.abs(ps1 - ps), axis=1))

    def decode(self, t_max, known=None, rows=slice(None), phi_method=1):
        kidx, ksym = (self.kidx, self.ksym) if known is None else known
        return sparc.camp_decode_partial_batch(self.Y[rows], self.op, kidx[rows], ksym[rows], VAR, t_max,
                                               phi_est_method=phi_method, K=self.K, true_idx=self.idx[rows],
                                               true_sym=self.sym[rows])


def _golden(name, seed, **kw):
    _, cp, _, _ = next(c for c in cc.CSPARC_CASES if c[0] == name)
    cp = cc.code_params(cp)
    K = cp['K'] if cp.get('modulated') else 1
    W, L, M, n, o0, o1 = cc.design(cc.golden(), name, cp)
    return Case(W, L, M, n, K, o0, o1, seed, L // 4, **kw)


def _flat(L, M, n, K, seed, L_unp, **kw):
    W = np.array(cc.P)
    o0, o1 = sparc.generate_ordering(W, n, L * M, 3, csparc=True)
    return Case(W, L, M, n, K, o0, o1, seed, L_unp, **kw)


MAKERS = {
    "flat4": lambda: _golden("cpsk4", 21),   # L = 64, M = 32, K = 4
    "pa4": lambda: _golden("cpa4", 21),      # four column blocks, each with its own tau and psi
    "sc4": lambda: _golden("csc4", 24),      # spatially coupled: phi per row block
    "k1": lambda: _flat(16, 64, 40, 1, 21, 4),   # creg's design (R = 2.4, M = 64) at L = 16
    "k8": lambda: _golden("cpsk8", 21),      # L = 64, M = 16, K = 8: the general-K branches
    "k2": lambda: _golden("cpsk2m2", 21),    # L = 64, M = 32, K = 2
    # section sizes and tails, B = 5 clean codewords: M = 2 (62 idle lanes), 16, 128 (two entries per lane), 2048
    # with L = 4, and L = 13 (no multiple of the four wavefronts of a workgroup)
    "m2": lambda: _flat(128, 2, 192, 4, 5, 32, sigmas=1.0, nb=5),
    "m16": lambda: _flat(32, 16, 96, 4, 5, 8, sigmas=1.0, nb=5),
    "m128": lambda: _flat(16, 128, 72, 4, 5, 4, sigmas=1.0, nb=5),
    "m2048": lambda: _flat(4, 2048, 26, 4, 5, 0, sigmas=1.0, nb=5),
    "l13": lambda: _flat(13, 32, 46, 4, 5, 3, sigmas=1.0, nb=5),
}
_made = {}


def case(name):
    if name not in _made:
        _made[name] = MAKERS[name]()
    return _made[name]


def _check(c, t_max, phi_method, want_stops):
    mi_r, ms_r, tf_r, nm_r, ps_r = c.restatement(t_max, phi_method)
    stable = c.moves(t_max, phi_method) < 1e-10
    assert np.count_nonzero(~stable) <= 1, stable
    assert len(set(tf_r.tolist())) >= want_stops, tf_r
    mi, ms, tf, nm, ps = c.decode(t_max, phi_method=phi_method)
    err = np.maximum(np.max(np.abs(nm - nm_r), axis=(1, 2)), np.max(np.abs(ps - ps_r), axis=1))
    print(f"t_max {t_max} phi {phi_method}: t_final {tf.tolist()}, stable {stable.tolist()}, "
          f"max |nmse, psi - ref| {err}")
    assert np.array_equal(tf[stable], tf_r[stable])
    assert np.array_equal(mi[stable], mi_r[stable]) and np.array_equal(ms[stable], ms_r[stable])
    np.testing.assert_allclose(nm[stable], nm_r[stable], rtol=0, atol=ATOL)
    np.testing.assert_allclose(ps[stable], ps_r[stable], rtol=0, atol=ATOL)
    # the known sections come back as given, the wrong ones included
    kn = c.kidx >= 0
    assert np.array_equal(mi[kn], c.kidx[kn]) and np.array_equal(ms[kn], c.ksym[kn])
    return mi, ms


# ---------------------------------------------------------------- 1: against the restatement

@pytest.mark.parametrize("name,phi_method", [("flat4", 1), ("flat4", 2), ("pa4", 1), ("sc4", 1), ("k1", 1), ("k8", 1),
                                             ("k2", 2)])
def test_vs_restatement(name, phi_method):
    c = case(name)
    t_max = 40 if name == "sc4" else 25
    mi, ms = _check(c, t_max, phi_method, 3)
    Lu = c.L_unp
    assert mi[2, Lu + 3] != c.idx[2, Lu + 3]
    assert (ms[3, Lu + 1] != c.sym[3, Lu + 1]) if c.K > 1 else (mi[3, Lu + 1] != c.idx[3, Lu + 1])


# ---------------------------------------------------------------- 2: section sizes and tails

@pytest.mark.parametrize("t_max", [3, 25])
@pytest.mark.parametrize("name", ["m2", "m16", "m128", "m2048", "l13"])
def test_section_sizes_and_tails(name, t_max):
    _check(case(name), t_max, 1, 1)


# ---------------------------------------------------------------- 3: all unknown = the plain decode

@pytest.mark.parametrize("name", ["flat4", "pa4", "sc4", "k1", "k8"])
def test_all_unknown_is_the_plain_decode(name):
    c = case(name)
    # (without the hopeless codeword: two decoders pin its stalled state no better than the restatement does)
    rows = np.array(SIGMAS) < 2.0
    t_max = 40 if name == "sc4" else 25
    mi0, ms0, tf0, nm0, ps0 = sparc.camp_decode_batch(c.Y[rows], c.op, VAR, t_max, K=c.K, true_idx=c.idx[rows],
                                                      true_sym=c.sym[rows])
    none = (np.full_like(c.kidx, -1), np.zeros_like(c.ksym))
    mi, ms, tf, nm, ps = c.decode(t_max, known=none, rows=rows)
    assert np.array_equal(mi, mi0) and np.array_equal(ms, ms0) and np.array_equal(tf, tf0)
    print(f"{name}: max |psi - decode| = {np.max(np.abs(ps - ps0)):.3e}, "
          f"max |nmse - decode| = {np.max(np.abs(nm - nm0)):.3e}")
    # the same kernels ran every operation of the plain loop (psi0 = 1, gamma0 = W 1, z0 = y - 0): the same bits
    assert nm.tobytes() == nm0.tobytes() and ps.tobytes() == ps0.tobytes()


# ---------------------------------------------------------------- 4: batch independence

@pytest.mark.parametrize("name", ["flat4", "sc4"])
def test_codeword_does_not_depend_on_its_batch(name):
    c = case(name)
    t_max = 40 if name == "sc4" else 25
    whole = c.decode(t_max)
    assert len(set(whole[2].tolist())) >= 3
    for b in (0, 2, 3, 7):
        one = c.decode(t_max, rows=slice(b, b + 1))
        for w, o in zip(whole, one):
            assert np.array_equal(w[b], o[0]), (name, b)


# ---------------------------------------------------------------- 5: the plan's state

def test_plan_reuse_and_soft_output_state():
    c = case("flat4")
    lib, p = _native.lib(), _native.ptr
    c.op.soft_output(True)
    try:
        before = sparc.camp_decode_batch(c.Y, c.op, VAR, 25, K=c.K, true_idx=c.idx, true_sym=c.sym)
        llr = sparc.camp_llr(c.op, B, c.K, 0, c.L)
        c.decode(25)
        cs = sparc._interleaved(sparc.psk_constel(c.K))
        assert lib.sg_camp_llr(c.op.plan(), B, c.K, p(cs), 0, c.L, 0, p(np.empty_like(llr))) == _native.SG_ERR_BAD_ARG
        after = sparc.camp_decode_batch(c.Y, c.op, VAR, 25, K=c.K, true_idx=c.idx, true_sym=c.sym)
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        assert np.array_equal(sparc.camp_llr(c.op, B, c.K, 0, c.L), llr)
    finally:
        c.op.soft_output(False)


# ---------------------------------------------------------------- 6: the unpacker

@pytest.mark.parametrize("K", [1, 2, 4, 64])
def test_unpack_sections_kernel(K):
    lib = _native.lib()
    logK = int(np.log2(K))
    rng = np.random.default_rng(K)
    nb, L = 3, 301
    words = cref.section_words(rng.integers(0, 2048, (nb, L)), rng.integers(0, K, (nb, L)), K).astype(np.int32)
    words[rng.random((nb, L)) < 0.3] = -1
    d_w = _native.DeviceBuffer.from_array(words)
    d_i, d_s, d_p = (_native.DeviceBuffer.from_array(np.full((nb, L), -7, np.int32)) for _ in range(3))
    _native.check(lib.sg_psk_unpack_sections_device(d_w.ptr, nb, L, logK, d_i.ptr, d_s.ptr, None))
    _native.check(lib.sg_psk_pack_sections_device(d_i.ptr, d_s.ptr, nb, L, logK, d_p.ptr, None))
    _native.synchronize()
    gi, gs, gp = (d.download(np.empty((nb, L), np.int32)) for d in (d_i, d_s, d_p))
    wi, ws = pr.unpack_words(words, K)
    assert np.array_equal(gi, wi) and np.array_equal(gs, ws)
    assert np.array_equal(gp[words >= 0], words[words >= 0])


# ---------------------------------------------------------------- 7: refusals before any launch

def test_refusals_before_any_launch():
    c = case("flat4")
    lib, p = _native.lib(), _native.ptr
    plan = c.op.plan()
    mi, ms, tf = (np.full((B, c.L), -7, np.int32), np.full((B, c.L), -7, np.int32), np.full(B, -7, np.int32))
    nm, ps = np.full((B, 25, 1), -7.0), np.full((B, 1), -7.0)
    cs = sparc._interleaved(sparc.psk_constel(c.K))

    def host(nb=B, K=c.K, t_max=25, kidx=c.kidx, ksym=c.ksym, constel=cs):
        return lib.sg_camp_decode_partial(plan, p(c.Y), nb, K, p(constel), p(kidx), p(ksym), None, None, VAR, t_max,
                                          1e-6, 1, p(mi), p(ms), p(tf), p(nm), p(ps))
    c128 = sparc._interleaved(np.exp(2j * np.pi * np.arange(128) / 128))
    assert host(K=128, constel=c128) == _native.SG_ERR_UNSUPPORTED
    assert host(t_max=1) == _native.SG_ERR_INVALID
    for bad in (-2, c.M):
        k = c.kidx.copy()
        k[3, 7] = bad
        assert host(kidx=k) == _native.SG_ERR_INVALID and b"known_idx" in lib.sg_last_error()
    for bad in (-1, c.K):
        k, s = c.kidx.copy(), c.ksym.copy()
        k[1, 5], s[1, 5] = 0, bad
        assert host(kidx=k, ksym=s) == _native.SG_ERR_INVALID and b"known_sym" in lib.sg_last_error()
    s = c.ksym.copy()
    s[0, :] = c.K + 3  # ... but not on a section to decode
    assert np.all(c.kidx[0] == -1)
    assert lib.sg_camp_decode_partial(plan, p(c.Y), B, c.K, p(cs), None, p(c.ksym), None, None, VAR, 25, 1e-6, 1,
                                      p(mi), p(ms), p(tf), p(nm), p(ps)) == _native.SG_ERR_INVALID
    assert lib.sg_camp_decode_partial(plan, p(c.Y), B, c.K, p(cs), p(c.kidx), None, None, None, VAR, 25, 1e-6, 1,
                                      p(mi), p(ms), p(tf), p(nm), p(ps)) == _native.SG_ERR_INVALID
    assert host(nb=0) == _native.SG_OK
    for a in (mi, ms, tf, nm, ps):
        assert np.all(a == -7)
    assert host(ksym=s) == _native.SG_OK and np.array_equal(mi, c.decode(25)[0])
    # the device variant takes a location out of range as unknown and the symbol modulo K
    k, s = c.kidx.copy(), c.ksym.copy()
    k[0, :], k[4, 2] = c.M + 5, -9
    s[1, c.L_unp:] += c.K
    wk = c.kidx.copy()
    wk[4, 2] = -1
    d_y, d_k, d_s = (_native.DeviceBuffer.from_array(a) for a in (c.Y, k, s))
    d_m = _native.DeviceBuffer(B * c.L * 4)
    _native.check(lib.sg_camp_decode_partial_device(plan, d_y.ptr, B, c.K, p(cs), d_k.ptr, d_s.ptr, None, None, VAR,
                                                    25, 1e-6, 1, d_m.ptr, None, None, None, None, None))
    _native.synchronize()
    assert np.array_equal(d_m.download(np.empty((B, c.L), np.int32)), c.decode(25, known=(wk, c.ksym))[0])


# ---------------------------------------------------------------- 8: pipeline

def _pipe(cls, **kw):
    return cls(G["L"], G["M"], G["K"], G["n"], G["P"], G["L_unp"], G["mults"], ldpc=G["ldpc"],
               design_seed=pr.DESIGN_SEED, **kw)


def test_pipeline_at_the_operating_point(oracle_built):
    """The operating point of tests/test_camp_partial_host.py with host-made
    batches: the five counters are the restatement's on the received words the
    pipeline holds, and the protected-bit counter is the two-stage pipeline's."""
    L, M, K, n, Lu = G["L"], G["M"], G["K"], G["n"], G["L_unp"]
    nb, per = pr.B_POINT, 6
    cnt = {}
    for cls in (CsparcConcatPipeline, CsparcConcat3Pipeline):
        pipe = _pipe(cls)
        idx, sym, info = pipe.make_batch(nb, pr.VAR, np.random.default_rng(pr.BATCH_SEED))
        pipe.reset_counts()
        pipe.decode()
        cnt[cls] = pipe.counts()
    two, three = cnt[CsparcConcatPipeline], cnt[CsparcConcat3Pipeline]
    pt = pr.point()
    assert np.array_equal(idx, pt["idx"]) and np.array_equal(sym, pt["sym"])  # the host test's batch
    assert np.array_equal(pipe.op.order0[0], np.ravel(pt["o0"]))
    assert np.array_equal(pipe.op.order1[0], np.ravel(pt["o1"]))
    Y = pipe.d_y.download(np.empty((nb, n), np.complex128))
    truth = np.stack([np.concatenate([cref.word_bits(cref.section_words(idx[b, :Lu], sym[b, :Lu], K), per),
                                      info.reshape(nb, -1)[b]]) for b in range(nb)])
    b2, b3 = [], []
    for b in range(nb):
        r = pr.three_stage(Y[b], pt["W"], L, M, n, K, pt["Ab"], pt["Az"], pr.VAR, 25, pt["beta0"][b], Lu, pt["c"])
        b2.append(pr.user_bits(r["idx2"], r["sym2"], r["app"], Lu, M, K, pt["c"]))
        b3.append(pr.user_bits(r["idx3"], r["sym3"], r["app"], Lu, M, K, pt["c"]))
    want2, want3 = cref.counters(np.stack(b2), truth, Lu * per), cref.counters(np.stack(b3), truth, Lu * per)
    print(f"two-stage {two.tolist()} (restatement {want2.tolist()}), three-stage {three.tolist()} "
          f"(restatement {want3.tolist()})")
    assert three[0] == nb and three[3] + three[4] == three[1]
    assert three[4] == two[4]  # the same BP output counts the protected bits
    assert np.array_equal(two, want2)
    assert np.array_equal(three, want3)


def test_pipeline_device_batches():
    """make_batch_device: reproducible per (seed, stream_id); ConcatTrial takes
    the pipeline; final_t_max reaches the last pass."""
    pipe = _pipe(CsparcConcat3Pipeline, final_t_max=12)
    assert pipe.final_t_max == 12 and _pipe(CsparcConcat3Pipeline).final_t_max == 25
    got = []
    for stream in (5, 6, 5):
        pipe.make_batch_device(8, pr.VAR, 4, stream)
        pipe.reset_counts()
        pipe.decode()
        got.append(pipe.counts())
    assert np.array_equal(got[0], got[2]) and got[0][0] == 8
    tr = montecarlo.ConcatTrial(pipe, [pr.VAR], seed=4)
    one = tr(0, 0, 4, 8)
    shards = [montecarlo.shard_range(4, r, 2) for r in range(2)]
    split = sum(tr(0, lo, hi - lo, 8) for lo, hi in shards)
    assert int(one[0]) == 32 and np.array_equal(one, split) and one[3] + one[4] == one[1]


# ---------------------------------------------------------------- 9: sweep

def test_fft3_sweep_checkpoints_and_resumes(tmp_path):
    import json
    kw = dict(codewords=16, block=8, ldpc=G["ldpc"], checkpoint_dir=str(tmp_path), precision="f64", design="fft",
              K=G["K"], final_amp=True, design_seed=pr.DESIGN_SEED)
    first = montecarlo.concat_ber_sweep(G["L"], G["M"], G["n"], G["P"], G["L_unp"], 1, [5.0, 7.0], **kw)
    tag = f"concat_fft3_L{G['L']}_M{G['M']}_K{G['K']}_n{G['n']}"
    for pt in (0, 1):
        params = json.load(open(tmp_path / f"{tag}_pt{pt}.json"))["params"]
        assert params["design"] == "fft3" and params["final_t_max"] == 25 and params["K"] == G["K"]
    again = montecarlo.concat_ber_sweep(G["L"], G["M"], G["n"], G["P"], G["L_unp"], 1, [5.0, 7.0], **kw)
    assert [o["codewords"] for o in first] == [16, 16]
    for a, b in zip(first, again):
        assert a["unprotected_bit_errors"] == b["unprotected_bit_errors"] and a["ber"] == b["ber"]
        assert a["protected_bit_errors"] == b["protected_bit_errors"]
