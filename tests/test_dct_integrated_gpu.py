"""GPU tests of the integrated AMP <-> BP decoders on the sub-sampled DCT design
(integrated_dct.hip, sg_amp_integrated_decode) against oracle/integrated_ref.py
run on the explicit matrix of the same design (dct_integrated_cases; the host
tests of test_dct_integrated_host.py pin that oracle on these inputs).

Bars:
  * double precision, cases A-E x four modes, batches of three: information
    bits identical on every codeword, tau^2 of every iteration within 1e-9
    relative (the bar of the dense integrated tests);
  * the dense engine on the uploaded explicit matrix (case A): the same bits,
    tau^2 within 1e-9;
  * a batch equals its codewords decoded alone (bits identical, tau^2 to
    1e-12) and a second run of the batch is bit-identical;
  * single precision: B, C and D decode to the transmitted bits in all four
    modes; tau^2 against the double-precision oracle within F32_TAU_RTOL (the
    measured maximum over these cases times 8, rounded up to a power of ten:
    DESIGN.md "Integrated decoders on the DCT design");
  * d_app: app[:, :K] < 0 is d_bits; refusals leave the outputs untouched;
    sg_amp_llr after an integrated decode is SG_ERR_BAD_ARG; sg_amp_decode and
    sg_amp_apply on the plan are bit for bit what they were.
"""
import ctypes as ct

import numpy as np
import pytest

import dct_integrated_cases as dc
from ldpc_sparc_amd import _native, sparc, sparc_new

pytestmark = pytest.mark.gpu

# measured maximum relative tau^2 difference of the f32 decode against the f64 oracle over B, C, D x four modes
# (MI355X): 3.9e-4 (case C, naive; 4.2e-5 C integrated_posteriors, 8.6e-6 B naive, every other case <= 2.2e-6);
# times 8 = 3.1e-3, rounded up to a power of ten.  The naive decoder at M = 2048 is also where the oracle itself
# moves most under one ulp of y (test_dct_integrated_host.py).
F32_TAU_RTOL = 1e-2


@pytest.fixture(scope="module")
def designs(oracle_built):
    made = {}

    def get(name):
        if name not in made:
            made[name] = sparc_new.DctDesign(dc.operator(dc.build(name)))
        return made[name]
    yield get
    for d in made.values():
        d.release()


def decode(design, c, mode, Y=None, precision=_native.SG_F64):
    return sparc_new.integrated_decode_batch(c.Y if Y is None else Y, design, c.code, dc.API_MODES[mode], dc.T_MAX,
                                             precision=precision)


@pytest.mark.parametrize("mode", dc.ORACLE_MODES)
@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_f64_matches_oracle(designs, name, mode):
    c = dc.build(name)
    ref_bits, ref_tau = dc.oracle(name, mode)
    bits, tau2 = decode(designs(name), c, mode)
    rel = np.max(np.abs(tau2 - ref_tau) / np.abs(ref_tau))
    print(f"{name} {mode}: max relative tau^2 difference {rel:.2e}")
    assert np.array_equal(bits, ref_bits)
    np.testing.assert_allclose(tau2, ref_tau, rtol=1e-9, atol=0)


@pytest.mark.parametrize("mode", dc.ORACLE_MODES)
def test_matches_dense_engine_on_the_explicit_matrix(designs, mode):
    c = dc.build("A")
    dense = sparc_new.DenseDesign(c.A, dc.P, c.L, c.M)
    try:
        db, dt = sparc_new.integrated_decode_batch(c.Y, dense, c.code, dc.API_MODES[mode], dc.T_MAX)
    finally:
        dense.release()
    bits, tau2 = decode(designs("A"), c, mode)
    assert np.array_equal(bits, db)
    np.testing.assert_allclose(tau2, dt, rtol=1e-9, atol=0)


@pytest.mark.parametrize("name,mode", [("A", "naivepost"), ("B", "integ"), ("C", "integpost"), ("D", "naive")])
def test_batched_equals_single_and_repeats(designs, name, mode):
    c = dc.build(name)
    d = designs(name)
    bits, tau2 = decode(d, c, mode)
    for b in range(dc.B):
        b1, t1 = decode(d, c, mode, Y=c.Y[b:b + 1])
        assert np.array_equal(b1[0], bits[b])
        np.testing.assert_allclose(t1[0], tau2[b], rtol=1e-12, atol=0)
    bits2, tau22 = decode(d, c, mode)
    assert np.array_equal(bits2, bits)
    assert np.array_equal(tau22.view(np.uint64), tau2.view(np.uint64))


@pytest.mark.parametrize("mode", dc.ORACLE_MODES)
@pytest.mark.parametrize("name", ["B", "C", "D"])
def test_f32_decodes(designs, name, mode):
    c = dc.build(name)
    _, ref_tau = dc.oracle(name, mode)
    bits, tau2 = decode(designs(name), c, mode, precision=_native.SG_F32)
    rel = np.max(np.abs(tau2 - ref_tau) / np.abs(ref_tau))
    print(f"{name} {mode} f32: max relative tau^2 difference {rel:.2e}")
    assert np.array_equal(bits, c.bits_in)
    assert rel <= F32_TAU_RTOL


# ------------------------------------------------------------------ the device entry point


def device_decode(plan, c, mode, prec, Y, fill=None, t_max=dc.T_MAX):
    """sg_amp_integrated_decode_device on fresh device buffers: (rc, bits, app, tau2)."""
    dt = np.float64 if prec == _native.SG_F64 else np.float32
    B = Y.shape[0]
    nblk = max(1, c.L * c.logM // c.N)
    d_y = _native.DeviceBuffer.from_array(Y.astype(dt))
    bits = np.full((B, nblk * c.K), 0 if fill is None else fill, np.uint8)
    app = np.full((B * nblk, c.N), 0 if fill is None else 7.25, dt)
    tau2 = np.full((B, t_max), 0 if fill is None else -3.5)
    d_bits, d_app, d_tau = (_native.DeviceBuffer.from_array(a) for a in (bits, app, tau2))
    rc = _native.lib().sg_amp_integrated_decode_device(
        plan, c.code._device_graph(), _native.INTEGRATED_MODES[dc.API_MODES[mode]], c.K, d_y.ptr, B, t_max, 6, 200,
        d_bits.ptr, d_app.ptr, d_tau.ptr, None)
    _native.synchronize()
    return rc, d_bits.download(np.empty_like(bits)), d_app.download(np.empty_like(app)), \
        d_tau.download(np.empty_like(tau2))


@pytest.mark.parametrize("prec", [_native.SG_F64, _native.SG_F32])
def test_device_app_gives_the_bits(designs, prec):
    c = dc.build("B")
    rc, bits, app, tau2 = device_decode(designs("B").plan(prec), c, "integ", prec, c.Y)
    assert rc == _native.SG_OK
    assert np.array_equal((app[:, :c.K] < 0).reshape(dc.B, -1), bits.astype(bool))
    assert np.array_equal(bits, c.bits_in)
    host_bits, host_tau = decode(designs("B"), c, "integ", precision=prec)
    assert np.array_equal(bits, host_bits)
    if prec == _native.SG_F64:
        assert np.array_equal(tau2.view(np.uint64), host_tau.view(np.uint64))


def test_refusals_touch_nothing():
    c = dc.build("A")
    LM = c.L * c.M
    # a power-allocated design (W of ndim 1)
    W = np.array([1.2 * dc.P, 0.8 * dc.P])
    o0, o1 = sparc.generate_ordering(W, c.n, LM // 2, 1)
    pa = sparc.DesignOperator(W, c.L, c.M, c.n, o0, o1)
    rc, bits, app, tau2 = device_decode(pa.plan(), c, "integ", _native.SG_F64, c.Y, fill=0xA5)
    assert rc == _native.SG_ERR_UNSUPPORTED
    assert b"flat" in _native.lib().sg_last_error()
    assert np.all(bits == 0xA5) and np.all(app == 7.25) and np.all(tau2 == -3.5)
    # L = 25 sections of M = 64: 150 bits are no multiple of N = 72
    Wf = np.array(dc.P)
    o0, o1 = sparc.generate_ordering(Wf, c.n, 25 * c.M, 1)
    odd = sparc.DesignOperator(Wf, 25, c.M, c.n, o0, o1)
    rc, bits, app, tau2 = device_decode(odd.plan(), c, "integ", _native.SG_F64, c.Y, fill=0xA5)
    assert rc == _native.SG_ERR_INVALID
    assert np.all(bits == 0xA5) and np.all(app == 7.25) and np.all(tau2 == -3.5)
    # bad counts on a good plan, and an empty batch
    good = dc.operator(c)
    rc, bits, app, tau2 = device_decode(good.plan(), c, "integ", _native.SG_F64, c.Y, fill=0xA5, t_max=0)
    assert rc == _native.SG_ERR_INVALID and np.all(bits == 0xA5)
    lib = _native.lib()
    assert lib.sg_amp_integrated_decode(good.plan(), c.code._device_graph(), 2, c.K, _native.ptr(c.Y), 0, dc.T_MAX, 6,
                                        200, _native.ptr(np.zeros(1, np.uint8)), None) == _native.SG_OK


def test_llr_after_an_integrated_decode_is_refused(designs):
    c = dc.build("A")
    op = designs("A").op
    sparc.amp_decode_batch(c.Y, op, dc.SIGMA2, 25)
    sparc.amp_llr(op, dc.B, 0, c.L)  # the AMP decode's state is there
    decode(designs("A"), c, "integ")
    out = np.zeros((dc.B, c.L * c.logM))
    rc = _native.lib().sg_amp_llr(op.plan(), dc.B, 0, c.L, 0, _native.ptr(out))
    assert rc == _native.SG_ERR_BAD_ARG


@pytest.mark.parametrize("prec", [_native.SG_F64, _native.SG_F32])
def test_plan_reuse_and_apply_unchanged(designs, prec):
    c = dc.build("B")
    fresh = dc.operator(c)
    used = designs("B").op
    rng = np.random.default_rng(11)
    xb, xz = rng.standard_normal((2, c.L * c.M)), rng.standard_normal((2, c.n))
    before = used.apply(xb, False, prec), used.apply(xz, True, prec)
    decode(designs("B"), c, "integpost", precision=prec)
    after = used.apply(xb, False, prec), used.apply(xz, True, prec)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    decode(designs("B"), c, "naive", precision=prec)
    got = sparc.amp_decode_batch(c.Y, used, dc.SIGMA2, 25, true_idx=c.idx, precision=prec)
    ref = sparc.amp_decode_batch(c.Y, fresh, dc.SIGMA2, 25, true_idx=c.idx, precision=prec)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0])
    assert np.array_equal(got[2].view(np.uint64), ref[2].view(np.uint64))


def test_general_engine_branch(monkeypatch):
    """A flat plan on the general four-step engine (SG_AMP_ENGINE=legacy at plan creation) decodes like the
    regular one."""
    c = dc.build("D")
    ref_bits, ref_tau = dc.oracle("D", "integ")
    monkeypatch.setenv("SG_AMP_ENGINE", "legacy")
    d = sparc_new.DctDesign(dc.operator(c))
    try:
        assert _native.lib().sg_amp_plan_engine(d.plan(), dc.B) == 0
        bits, tau2 = decode(d, c, "integ")
    finally:
        d.release()
    assert np.array_equal(bits, ref_bits)
    np.testing.assert_allclose(tau2, ref_tau, rtol=1e-9, atol=0)


def test_pipeline_counts():
    from ldpc_sparc_amd.pipeline import DctIntegratedPipeline
    c = dc.build("B")
    ldpc, L, M, n = dc.CASES["B"][:4]
    pipe = DctIntegratedPipeline(L, M, n, dc.P, ldpc=ldpc, design_seed=2, precision="f64", t_max=dc.T_MAX,
                                 mode="integrated")
    rng = np.random.default_rng(5)
    expect = np.zeros(5, np.int64)

    def run(var):
        _, info = pipe.make_batch(4, var, rng)
        if not expect[0]:
            pipe.reset_counts()  # (the counters exist once the first batch has sized the buffers)
        pipe.decode()
        _native.synchronize()
        app = pipe.d_app.download(np.empty((4 * pipe.mults, c.N)))
        wrong = ((app[:, :c.K] < 0) != info.astype(bool)).reshape(4, -1).sum(axis=1)
        expect[:] += [4, wrong.sum(), (wrong > 0).sum(), 0, wrong.sum()]
        return int(wrong.sum())

    assert run(1.0) == 0 and run(1.0) == 0
    cnt = pipe.counts()
    assert cnt[0] == 8 and cnt[1] == 0 and np.array_equal(cnt, expect)
    assert run(25.0) > 0
    assert np.array_equal(pipe.counts(), expect)
