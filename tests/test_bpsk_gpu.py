"""GPU tests of the real K = 2 (BPSK) modulated AMP decode (sg_amp_decode_bpsk*,
sg_amp_encode_bpsk_device, amp_oploop.hip), of the drop-in surface behind
sparc.enable_real_psk() and of montecarlo.SparcTrial(K=2).

The yardsticks are the reference's fixture tests/golden/bpsk_golden.npz (every
case and seed of tests/bpsk_cases.py) and the restatement tests/amp_bpsk_ref.py,
which tests/test_bpsk_host.py holds against that fixture.

Bars (those of test_csparc_gpu.py and test_amp_partial_gpu.py): in double
precision x at atol 1e-9, map words and t_final equal, nmse and psi at atol
1e-9; in single precision the map words of every codeword the restatement
decodes without a section error, and nmse at 1e-3 at t_max = 4; a codeword's
outputs bit-identical alone and in a batch, in both precisions."""
import numpy as np
import pytest

import amp_bpsk_ref as br
import section_size_cases as ssc
from bpsk_cases import AWGN_VAR, IDS, all_seeds, code_params, golden, seed_of, true_words, words
from ldpc_sparc_amd import _native, montecarlo, sparc, sparc_sim

pytestmark = pytest.mark.gpu

F64, F32 = _native.SG_F64, _native.SG_F32
SEEDS = list(all_seeds())


class Seed:
    """One case and seed of the fixture: the design sparc_transforms draws from
    the seed, as GPU operator and as CPU operators, and the transmitted words."""

    def __init__(self, name, cp, dp, si):
        g, self.key = golden(), f"{name}_s{si}"
        cp, dp = dict(cp), dict(dp)
        sparc.check_code_params(cp)
        sparc.check_decode_params(dp)
        self.dp, self.L, self.M, self.n = dp, cp['L'], cp['M'], int(g[self.key + "_n"])
        tmp = cp.copy()
        tmp.update({'awgn_var': AWGN_VAR})
        self.W = sparc.create_base_matrix(**tmp)
        Ab, Az = sparc.sparc_transforms(self.W, self.L, self.M, self.n, seed_of(si))
        self.op = sparc.operator_of(Ab, Az)
        self.tw = true_words(g[self.key + "_bits"], self.M)
        self.y = g[self.key + "_y"]
        self.g = {k[len(self.key) + 1:]: v for k, v in g.items() if k.startswith(self.key + "_")}

    def cpu_operators(self):
        nd = self.W.ndim
        o0, o1 = self.op.order0, self.op.order1
        if nd == 0:
            o0, o1 = o0[0], o1[0]
        elif nd == 2:
            Lr, Lc = self.W.shape
            O0 = np.zeros((Lr, Lc, o0.shape[1]), np.uint32)
            O1 = np.zeros((Lr, Lc, o1.shape[1]), np.uint32)
            nz = [(r, c) for r in range(Lr) for c in range(Lc) if self.W[r, c] != 0]
            for t, (r, c) in enumerate(nz):
                O0[r, c], O1[r, c] = o0[t], o1[t]
            o0, o1 = O0, O1
        return br.operators(self.W, self.L, self.M, self.n, o0, o1)

    def decode(self, prec, t_max=None):
        dp = self.dp
        return sparc.amp_decode_bpsk_batch(self.y[None], self.op, AWGN_VAR, t_max or dp['t_max'], dp['rtol'],
                                           dp['phi_est_method'], self.tw[None], prec)


_seeds = {}


def seed_case(name, cp, dp, si):
    if (name, si) not in _seeds:
        _seeds[name, si] = Seed(name, cp, dp, si)
    return _seeds[name, si]


def _encode_device(op, tw, prec):
    dt = np.float64 if prec == F64 else np.float32
    B = tw.shape[0]
    d_w = _native.DeviceBuffer.from_array(np.ascontiguousarray(tw, dtype=np.int32))
    d_x = _native.DeviceBuffer(B * op.n * dt().itemsize)
    _native.check(_native.lib().sg_amp_encode_bpsk_device(op.plan(prec), d_w.ptr, B, d_x.ptr, None))
    _native.synchronize()
    return d_x.download(np.empty((B, op.n), dt))


# ---------------------------------------------------------------- double precision against the fixture

@pytest.mark.parametrize("name,cp,dp,si", SEEDS, ids=IDS)
def test_f64_matches_reference(name, cp, dp, si):
    c = seed_case(name, cp, dp, si)
    x = _encode_device(c.op, c.tw[None], F64)[0]
    print(c.key, "max |x - ref|", np.abs(x - c.g["x"]).max())
    np.testing.assert_allclose(x, c.g["x"], rtol=0, atol=1e-9)
    mw, tf, nmse, psi = c.decode(F64)
    ref_nmse, ref_psi = c.g["nmse"], c.g["psi"]
    print(c.key, "t_final", tf[0], int(c.g["t_final"]), "max |nmse - ref|",
          np.abs(nmse[0].reshape(ref_nmse.shape) - ref_nmse).max(), "max |psi - ref|",
          np.abs(psi[0].reshape(ref_psi.shape) - ref_psi).max())
    assert tf[0] == int(c.g["t_final"])
    assert np.array_equal(mw[0], words(c.g["map"], c.g["map_sym"]))
    np.testing.assert_allclose(nmse[0].reshape(ref_nmse.shape), ref_nmse, rtol=0, atol=1e-9)
    np.testing.assert_allclose(psi[0].reshape(ref_psi.shape), ref_psi, rtol=0, atol=1e-9)


@pytest.mark.parametrize("name,cp,dp,si", SEEDS, ids=IDS)
def test_sparc_sim_dropin_matches_reference(name, cp, dp, si):
    """sparc_sim (the reference's call surface) end to end on the GPU, behind the switch."""
    g, key = golden(), f"{name}_s{si}"
    prev = sparc.enable_real_psk()
    try:
        res = sparc_sim.sparc_sim(dict(cp), dict(dp), AWGN_VAR, seed_of(si))
    finally:
        sparc.enable_real_psk(prev)
    assert sparc._real_psk is prev
    sim = {k[len(key) + 5:]: v for k, v in g.items() if k.startswith(key + "_sim_")}
    assert set(res) == set(sim) | {'nmse'}
    for k, v in sim.items():
        if v.ndim == 0:
            assert res[k] == v.item(), (key, k)
        else:
            assert np.array_equal(res[k], v), (key, k)
    assert res['nmse'].shape == g[key + "_nmse"].shape and res['nmse'].dtype == np.float64
    np.testing.assert_allclose(res['nmse'], g[key + "_nmse"], rtol=0, atol=1e-9)


def test_dropin_shapes_and_dtypes():
    """sparc_encode / sparc_decode with the switch on: the reference's returns, f32 through decode_params."""
    name, cp, dp, si = SEEDS[0]
    g, key = golden(), f"{name}_s{si}"
    prev = sparc.enable_real_psk()
    try:
        cp = dict(cp)
        bits, beta0, x, Ab, Az = sparc.sparc_encode(cp, AWGN_VAR, seed_of(si))
        assert beta0.dtype == np.float64 and x.dtype == np.float64 and np.array_equal(bits, g[key + "_bits"])
        dp = dict(dp, precision='f32')
        bits_o, beta, T, nmse, expect = sparc.sparc_decode(g[key + "_y"], cp, dp, AWGN_VAR, seed_of(si), beta0, Ab, Az)
    finally:
        sparc.enable_real_psk(prev)
    assert beta.dtype == np.float64 and nmse.shape == (dp['t_max'],) and not expect
    assert np.array_equal(bits_o, g[key + "_bits_out"]) and np.array_equal(beta, beta0)


# ---------------------------------------------------------------- single precision

@pytest.mark.parametrize("name,cp,dp,si", SEEDS, ids=IDS)
def test_f32_vs_restatement(name, cp, dp, si):
    c = seed_case(name, cp, dp, si)
    ref_words = words(c.g["map"], c.g["map_sym"])  # the restatement's (test_bpsk_host.py)
    if np.array_equal(ref_words, c.tw):
        mw, _, _, _ = c.decode(F32)
        assert np.array_equal(mw[0], ref_words)
    Ab, Az = c.cpu_operators()
    _, _, nm_r, _ = br.amp_bpsk(c.y, c.W, c.L, c.M, c.n, AWGN_VAR, 4, Ab, Az, br.beta_of_words(c.tw, c.M),
                                c.dp['rtol'], c.dp['phi_est_method'])
    _, _, nm, _ = c.decode(F32, t_max=4)
    nm_r = np.asarray(nm_r).reshape(4, -1)
    print(f"{c.key} f32 t_max=4: max |nmse - ref| = {np.max(np.abs(nm[0] - nm_r)):.3e}")
    np.testing.assert_allclose(nm[0], nm_r, rtol=0, atol=1e-3)


def test_f32_cases_cover_clean_and_failing_codewords():
    g = golden()
    clean = [np.array_equal(words(g[f"{n}_s{si}_map"], g[f"{n}_s{si}_map_sym"]),
                            true_words(g[f"{n}_s{si}_bits"], cp['M'])) for n, cp, _, si in SEEDS]
    assert sum(clean) >= 15 and not all(clean)


# ---------------------------------------------------------------- one batch

SIGMAS = [0.5, 1.0, 2.5, 1.0, 2.0, 1.5, 2.2, 0.8]

_batch = {}


def batch():
    """breg's design of seed 0 with eight codewords at noise sigma 0.5 to 2.5."""
    if not _batch:
        name, cp, dp, si = SEEDS[0]
        c = seed_case(name, cp, dp, si)
        rng = np.random.RandomState(41)
        tw = rng.randint(0, 2 * c.M, (8, c.L)).astype(np.int32)
        X = _encode_device(c.op, tw, F64)
        Y = X + np.array(SIGMAS)[:, None] * rng.randn(8, c.n)
        _batch.update(c=c, tw=tw, Y=Y)
    return _batch


@pytest.mark.parametrize("prec", [F64, F32])
def test_codeword_does_not_depend_on_its_batch(prec):
    bt = batch()
    c, tw, Y = bt["c"], bt["tw"], bt["Y"]
    t_max = 25
    whole = sparc.amp_decode_bpsk_batch(Y, c.op, AWGN_VAR, t_max, true_word=tw, precision=prec)
    mw, tf, nm, ps = whole
    print("t_final", tf.tolist(), "section errors", (mw != tw).sum(axis=1).tolist())
    assert tf.min() < t_max - 1 and tf.max() == t_max - 1  # easy and non-decoding codewords in one batch
    assert np.array_equal(mw[0], tw[0]) and np.any(mw[2] != tw[2])
    for b in range(8):
        one = sparc.amp_decode_bpsk_batch(Y[b:b + 1], c.op, AWGN_VAR, t_max, true_word=tw[b:b + 1], precision=prec)
        for w, o in zip(whole, one):
            assert np.array_equal(w[b], o[0]), (prec, b)
        # a stopped codeword keeps its t_final and its tail nmse[t:] = nmse[t], t = t_final - 1
        if tf[b] < t_max - 1:
            assert np.all(nm[b, tf[b] - 1:] == nm[b, tf[b] - 1])
        assert np.all(nm[b, 0] == 1.0) and np.all(np.isfinite(nm[b]))


def test_batch_f64_vs_restatement():
    """The converging codewords of the batch against the restatement (the
    stalled ones are pinned by the fixture's bhard and bM2048 seeds)."""
    bt = batch()
    c, tw, Y = bt["c"], bt["tw"], bt["Y"]
    Ab, Az = c.cpu_operators()
    rows = [b for b, s in enumerate(SIGMAS) if s <= 1.0]
    mw_r, tf_r, nm_r, ps_r = br.decode_batch(Y[rows], c.W, c.L, c.M, c.n, AWGN_VAR, 25, Ab, Az, tw[rows])
    mw, tf, nm, ps = sparc.amp_decode_bpsk_batch(Y, c.op, AWGN_VAR, 25, true_word=tw)
    assert np.array_equal(tf[rows], tf_r) and np.array_equal(mw[rows], mw_r)
    np.testing.assert_allclose(nm[rows], nm_r, rtol=0, atol=1e-9)
    np.testing.assert_allclose(ps[rows], ps_r, rtol=0, atol=1e-9)


# ---------------------------------------------------------------- refusals

def test_refusals():
    name, cp, dp, si = SEEDS[0]
    c = seed_case(name, cp, dp, si)
    W, L, M, n = np.array(15.0), 4, 8, 12
    o0, o1 = sparc.generate_ordering(W, n, L * M, 1, True)
    with pytest.raises(ValueError, match="real DesignOperator"):
        sparc.amp_decode_bpsk_batch(np.zeros((1, n), complex), sparc.ComplexDesignOperator(W, L, M, n, o0, o1), 1.0, 5)
    with pytest.raises(_native.NativeError, match="t_max"):
        sparc.amp_decode_bpsk_batch(c.y[None], c.op, 1.0, 1)
    lib, p = _native.lib(), _native.ptr
    assert lib.sg_amp_decode_bpsk_device(c.op.plan(F64), None, 1, None, 1.0, 1, 1e-6, 1, None, None, None, None,
                                         None) == _native.SG_ERR_INVALID
    s = ssc.case("m4096")
    op = sparc.DesignOperator(s.W, s.L, s.M, s.n, s.o0, s.o1)
    mw, tf = np.full((ssc.B, s.L), -7, np.int32), np.full(ssc.B, -7, np.int32)
    nm, ps = np.full((ssc.B, 25, 1), -7.0), np.full((ssc.B, 1), -7.0)
    for prec in (F64, F32):
        rc = lib.sg_amp_decode_bpsk(op.plan(prec), p(s.Y), ssc.B, None, 1.0, 25, 1e-6, 1, p(mw), p(tf), p(nm), p(ps))
        assert rc == _native.SG_ERR_UNSUPPORTED and b"2048" in lib.sg_last_error()
    assert np.all(mw == -7) and np.all(tf == -7) and np.all(nm == -7) and np.all(ps == -7)
    # B = 0 does nothing; the plan still decodes
    assert lib.sg_amp_decode_bpsk(c.op.plan(F64), p(np.zeros(0)), 0, None, 1.0, 25, 1e-6, 1, None, None, None,
                                  None) == _native.SG_OK
    assert c.decode(F64)[1][0] == int(c.g["t_final"])


# ---------------------------------------------------------------- campaign

def _trial_inputs(tr, block, K):
    """What SparcTrial draws for block 0 of point 0: (words or indices [block, L],
    Y [block, n] as the device holds it)."""
    op, lib = tr.op, _native.lib()
    L, n, k = op.L, op.n, tr.logM
    dt = np.float64 if tr.prec == F64 else np.float32
    d_bits = _native.DeviceBuffer(block * L * k)
    _native.check(lib.sg_rng_bits_device(tr.seed, 0, block, L * k, d_bits.ptr, None))
    _native.synchronize()
    bits = d_bits.download(np.empty(block * L * k, np.uint8))
    sec = (bits.reshape(block, L, k).astype(np.int64) @ (1 << np.arange(k)[::-1])).astype(np.int32)
    d_sec = _native.DeviceBuffer.from_array(sec)
    d_x = _native.DeviceBuffer(block * n * dt().itemsize)
    d_y = _native.DeviceBuffer(block * n * dt().itemsize)
    enc = lib.sg_amp_encode_bpsk_device if K == 2 else lib.sg_amp_encode_device
    _native.check(enc(op.plan(tr.prec), d_sec.ptr, block, d_x.ptr, None))
    _native.check(lib.sg_awgn_device(tr.prec, tr.seed, 0, d_x.ptr, block, n, float(np.sqrt(tr.vars[0])), d_y.ptr, None))
    _native.synchronize()
    return sec, d_y.download(np.empty((block, n), dt)).astype(np.float64)


def _counters(mp, true, tf):
    wrong = mp != true
    bit_err = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(mp.ravel(), true.ravel()))
    return np.array([len(tf), bit_err, int(np.any(wrong, axis=1).sum()), int(tf.sum()), int(wrong.sum())], np.int64)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_sparc_trial_bpsk(precision):
    name, cp, dp, si = SEEDS[0]
    c = seed_case(name, cp, dp, si)
    var = 5.0  # some codewords fail: every counter moves
    tr = montecarlo.SparcTrial(c.op, [var], t_max=25, precision=precision, seed=5, K=2)
    assert tr.logM == 6
    got = tr(0, 0, 1, 8)
    tw, Y = _trial_inputs(tr, 8, 2)
    assert tw.max() < 2 * c.M and tw.max() >= c.M  # words, not indices
    mw, tf, _, _ = sparc.amp_decode_bpsk_batch(Y, c.op, var, 25, true_word=tw, precision=tr.prec)
    want = _counters(mw, tw, tf)
    print(precision, "SparcTrial(K=2)", got.tolist(), "host", want.tolist())
    assert np.array_equal(got, want) and got[0] == 8 and got[1] > 0


def test_sparc_trial_default_is_unmodulated():
    name, cp, dp, si = SEEDS[0]
    c = seed_case(name, cp, dp, si)
    var = 5.0
    tr = montecarlo.SparcTrial(c.op, [var], t_max=25, precision="f64", seed=5)
    assert tr.K == 1 and tr.logM == 5
    got = tr(0, 0, 1, 8)
    ti, Y = _trial_inputs(tr, 8, 1)
    assert ti.max() < c.M
    mi, tf, _, _ = sparc.amp_decode_batch(Y, c.op, var, 25, true_idx=ti, precision=F64)
    assert np.array_equal(got, _counters(mi, ti, tf))
