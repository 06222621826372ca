"""Section-size sweep of the DCT-design AMP path, M = 2 to 2048 (and the upper
bound, M = 4096), against the oracle: every kernel that is instantiated per
section size -- reg_llr_kernel<T, 1 / 8 / 32> (amp_llr.hip), eta_kernel<T, 1 ..
32> (amp_dct.hip), the trips of glue_llr_kernel's j += 64 loop (dense.hip) and
the staged regular engine's section addressing, statistics, merge and MAP
(amp_fused.hip) -- at geometries a few hundred values wide
(tests/section_size_cases.py; tests/test_section_sizes_host.py pins the
operating points with the oracle alone).

Two engines per geometry: the regular engine (the default for these designs;
with B = 3 never a per-codeword plan's engine, which is asserted, not assumed)
and the general four-step engine (SG_AMP_ENGINE=legacy while the plan is built).

Bars (the project's own, fixed): t_final and MAP equal to the oracle's, NMSE
1e-9 (test_decode_f64_matches_reference), bit probabilities 1e-9 in double and
1e-3 in single precision at t_max = 3 (ATOL of test_dct_concat_gpu.py), LLR
against the clip / log of the same call's probabilities rtol 1e-12 / 1e-5,
single precision at t_max = 25: MAP = truth and |t_final - oracle| <= 2
(test_decode_f32_tolerance)."""
import ctypes as ct

import numpy as np
import pytest

import dct_concat_ref as ref
import section_size_cases as ssc
from ldpc_sparc_amd import _native, sparc

pytestmark = pytest.mark.gpu

F64, F32 = _native.SG_F64, _native.SG_F32
ATOL = {F64: 1e-9, F32: 1e-3}
LLR_RTOL = {F64: 1e-12, F32: 1e-5}
NMSE_ATOL = 1e-9
ENGINES = {"regular": 1, "general": 0}  # sg_amp_plan_engine / amp_last_decode codes
B = ssc.B

_ops = {}


def _set_engine(monkeypatch, engine):
    if engine == "general":
        monkeypatch.setenv("SG_AMP_ENGINE", "legacy")
    else:
        monkeypatch.delenv("SG_AMP_ENGINE", raising=False)


def _op(monkeypatch, name, engine):
    """The geometry's operator with both plans built for `engine` (the plan
    builder reads SG_AMP_ENGINE; built once per (geometry, engine))."""
    _set_engine(monkeypatch, engine)
    if (name, engine) not in _ops:
        c = ssc.case(name)
        op = sparc.DesignOperator(c.W, c.L, c.M, c.n, c.o0, c.o1)
        for prec in (F64, F32):
            op.plan(prec)
        _ops[name, engine] = op
    return _ops[name, engine]


def _decode(c, op, engine, t_max, prec, Y=None, true=None):
    """amp_decode_batch, and which engine ran it: asserted, never assumed."""
    Y = c.Y if Y is None else Y
    true = c.true if true is None else true
    assert _native.lib().sg_amp_plan_engine(op.plan(prec), len(Y)) == ENGINES[engine]
    out = sparc.amp_decode_batch(Y, op, ssc.VAR, t_max, rtol=1e-6, true_idx=true, precision=prec)
    assert _native.amp_last_decode(op.plan(prec))["engine"] == ENGINES[engine]
    return out


def _soft(op, nb, L, prec):
    return (sparc.amp_llr(op, nb, 0, L, probs_only=True, precision=prec),
            sparc.amp_llr(op, nb, 0, L, precision=prec))


# ---------------------------------------------------------------- double precision against the oracle

def _check_f64(monkeypatch, name, engine, t_max):
    c = ssc.case(name)
    op = _op(monkeypatch, name, engine)
    o = c.oracle(t_max)
    mi, tf, nmse, _ = _decode(c, op, engine, t_max, F64)
    p, llr = _soft(op, B, c.L, F64)
    d_nmse = np.max(np.abs(nmse - o["nmse"]))
    d_p = np.max(np.abs(p - o["probs"]))
    want_llr = ref.llr_of_probs(p)
    d_llr = np.max(np.abs(llr - want_llr) / np.maximum(np.abs(want_llr), 1e-300))
    print(f"{name} M={c.M} {engine} f64 t_max={t_max}: t_final {tf.tolist()}, max |nmse - oracle| = {d_nmse:.3e}, "
          f"max |p - oracle| = {d_p:.3e}, max rel |llr - clip/log(p)| = {d_llr:.3e}")
    assert np.array_equal(tf, o["t_final"])
    assert np.array_equal(mi, o["map"])
    np.testing.assert_allclose(nmse, o["nmse"], rtol=0, atol=NMSE_ATOL)
    np.testing.assert_allclose(p, o["probs"], rtol=0, atol=ATOL[F64])
    assert np.all(np.isfinite(llr))
    np.testing.assert_allclose(llr, want_llr, rtol=LLR_RTOL[F64], atol=0)


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", ssc.NAMES)
def test_f64_soft_point_vs_oracle(monkeypatch, name, engine):
    _check_f64(monkeypatch, name, engine, ssc.T_SOFT)


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", ssc.CONVERGING)
def test_f64_full_decode_vs_oracle(monkeypatch, name, engine):
    _check_f64(monkeypatch, name, engine, ssc.T_FULL)


# ---------------------------------------------------------------- single precision

@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", ssc.NAMES)
def test_f32_soft_point_vs_oracle(monkeypatch, name, engine):
    c = ssc.case(name)
    op = _op(monkeypatch, name, engine)
    o = c.oracle(ssc.T_SOFT)
    _decode(c, op, engine, ssc.T_SOFT, F32)
    p, llr = _soft(op, B, c.L, F32)
    want_llr = ref.llr_of_probs(p)
    d_llr = np.max(np.abs(llr - want_llr) / np.maximum(np.abs(want_llr), 1e-300))
    print(f"{name} M={c.M} {engine} f32 t_max={ssc.T_SOFT}: max |p - oracle| = {np.max(np.abs(p - o['probs'])):.3e}, "
          f"max rel |llr - clip/log(p)| = {d_llr:.3e}")
    np.testing.assert_allclose(p, o["probs"], rtol=0, atol=ATOL[F32])
    assert np.all(np.isfinite(llr))
    np.testing.assert_allclose(llr, want_llr, rtol=LLR_RTOL[F32], atol=0)


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", ssc.CONVERGING)
def test_f32_full_decode(monkeypatch, name, engine):
    c = ssc.case(name)
    op = _op(monkeypatch, name, engine)
    o = c.oracle(ssc.T_FULL)
    mi, tf, _, _ = _decode(c, op, engine, ssc.T_FULL, F32)
    print(f"{name} M={c.M} {engine} f32 t_max={ssc.T_FULL}: t_final {tf.tolist()} (oracle {o['t_final'].tolist()})")
    assert np.array_equal(mi, c.true)
    assert np.all(np.abs(tf.astype(int) - o["t_final"].astype(int)) <= 2)


# ---------------------------------------------------------------- section range and stride at the wide sizes

@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", ["m256", "m2048"])
def test_section_range_and_stride(monkeypatch, name, engine, prec):
    """Sections [1, L - 1) -- a count that is no multiple of the four wavefronts
    of a workgroup -- into rows 3 values longer than the range: the slice of the
    full call bit for bit, every other element untouched."""
    c = ssc.case(name)
    op = _op(monkeypatch, name, engine)
    _decode(c, op, engine, ssc.T_SOFT, prec)
    l0, nl = 1, c.L - 2
    assert nl % 4 != 0
    ld = nl * c.logM + 3
    dt = np.float64 if prec == F64 else np.float32
    for probs_only in (0, 1):
        whole = sparc.amp_llr(op, B, 0, c.L, probs_only=bool(probs_only), precision=prec)
        host = np.full((B, ld), -777.0, dt)
        buf = _native.DeviceBuffer.from_array(host)
        _native.check(_native.lib().sg_amp_llr_device(op.plan(prec), B, l0, nl, ld, probs_only, buf.ptr, None))
        _native.synchronize()
        out = buf.download(np.empty((B, ld), dt))
        assert np.all(out[:, nl * c.logM:] == -777.0)
        assert np.array_equal(out[:, :nl * c.logM].astype(np.float64), whole[:, l0 * c.logM:(l0 + nl) * c.logM])


# ---------------------------------------------------------------- first-index MAP at a tie

@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("name", ["m256", "m2048"])
def test_map_tie_takes_first_index(monkeypatch, name, engine):
    """A received word of zeros leaves s = 0 in every entry after the first
    iteration, an exact tie over each whole section: the MAP index is the
    lowest one (numpy.argmax, sparc.py:485-487), 0 in every section, as the
    oracle's.  t_max = 2 is the shortest decode that runs an iteration (t_max
    counts the initial state: t_max = 1 runs none, and the oracle then has no
    s to take a maximum of)."""
    c = ssc.case(name)
    op = _op(monkeypatch, name, engine)
    Y = np.zeros((B, c.n))
    o = c.oracle_of(Y, 2)
    assert np.all(o["map"] == 0) and np.all(o["probs"] == 0.5)  # the tie is exact on the oracle's side
    mi, tf, nmse, _ = _decode(c, op, engine, 2, F64, Y=Y)
    assert np.array_equal(mi, np.zeros((B, c.L), np.int32))
    assert np.array_equal(mi, o["map"])
    assert np.array_equal(tf, o["t_final"])
    np.testing.assert_allclose(nmse, o["nmse"], rtol=0, atol=NMSE_ATOL)
    p = sparc.amp_llr(op, B, 0, c.L, probs_only=True)
    np.testing.assert_allclose(p, o["probs"], rtol=0, atol=ATOL[F64])


# ---------------------------------------------------------------- batch = single

@pytest.mark.parametrize("engine", list(ENGINES))
def test_batch_equals_single_m1024(monkeypatch, engine):
    c = ssc.case("m1024")
    op = _op(monkeypatch, "m1024", engine)
    for t_max in (ssc.T_SOFT, ssc.T_FULL):
        mb, tb, nb, _ = _decode(c, op, engine, t_max, F64)
        pb = sparc.amp_llr(op, B, 0, c.L, probs_only=True)
        m1, t1, n1, _ = _decode(c, op, engine, t_max, F64, Y=c.Y[2:3], true=c.true[2:3])
        p1 = sparc.amp_llr(op, 1, 0, c.L, probs_only=True)
        assert t1[0] == tb[2]
        assert np.array_equal(m1[0], mb[2])
        assert np.array_equal(n1[0], nb[2])
        assert np.array_equal(p1[0], pb[2])


# ---------------------------------------------------------------- the upper bound, M = 4096

def test_m4096_regular_engine_decodes_without_soft_output(monkeypatch):
    """The staged regular engine has no bound on M: it addresses a section
    through qpos at ll * M, keeps section numbers and LDS positions in 16 bits
    each (bounds on L / Lc and P, checked at plan creation) and takes a
    section's statistics over class segments of any length.  So M = 4096
    decodes to the oracle; the bit LLRs, whose kernel holds at most 32 entries
    per lane, are SG_ERR_UNSUPPORTED naming the M."""
    c = ssc.case("m4096")
    _set_engine(monkeypatch, "regular")
    op = sparc.DesignOperator(c.W, c.L, c.M, c.n, c.o0, c.o1)
    o = c.oracle(ssc.T_FULL)
    mi, tf, nmse, _ = _decode(c, op, "regular", ssc.T_FULL, F64)
    print(f"m4096 regular f64: t_final {tf.tolist()}, max |nmse - oracle| = {np.max(np.abs(nmse - o['nmse'])):.3e}")
    assert np.array_equal(tf, o["t_final"])
    assert np.array_equal(mi, o["map"])
    np.testing.assert_allclose(nmse, o["nmse"], rtol=0, atol=NMSE_ATOL)
    lib = _native.lib()
    out = np.full((B, c.L * c.logM), -777.0)
    for probs_only in (0, 1):
        assert lib.sg_amp_llr(op.plan(F64), B, 0, c.L, probs_only, _native.ptr(out)) == _native.SG_ERR_UNSUPPORTED
        assert b"4096" in lib.sg_last_error()
    assert np.all(out == -777.0)
    buf = _native.DeviceBuffer.from_array(out)
    assert lib.sg_amp_llr_device(op.plan(F64), B, 0, c.L, c.L * c.logM, 0, buf.ptr, None) == _native.SG_ERR_UNSUPPORTED
    assert b"4096" in lib.sg_last_error()
    _native.synchronize()
    assert np.all(buf.download(np.empty_like(out)) == -777.0)


def _create(W, L, M, n, o0, o1, prec):
    """sg_amp_plan_create as DesignOperator.plan calls it: (status, handle)."""
    op = sparc.DesignOperator(W, L, M, n, o0, o1)
    h = ct.c_void_p()
    Wf = np.ascontiguousarray(op.W.reshape(-1), dtype=np.float64)
    rc = _native.lib().sg_amp_plan_create(op.W.ndim, _native.ptr(Wf), op.Lr, op.Lc, op.L, op.M, op.n,
                                          _native.ptr(op.order0), _native.ptr(op.order1), prec, ct.byref(h))
    return rc, h


@pytest.mark.parametrize("prec", [F64, F32])
def test_m4096_general_engine_refused_at_plan_creation(monkeypatch, prec):
    """The general engine's section kernel holds at most 32 entries per lane
    (M <= 2048): a plan that would run it on larger sections is refused when it
    is created -- never in the middle of a decode -- with the M in the message
    and no handle; the same geometry at M = 2048 gets its plan."""
    lib = _native.lib()
    c = ssc.case("m4096")
    _set_engine(monkeypatch, "general")
    rc, h = _create(c.W, c.L, c.M, c.n, c.o0, c.o1, prec)
    assert rc == _native.SG_ERR_UNSUPPORTED
    msg = lib.sg_last_error()
    assert b"4096" in msg and b"2048" in msg and b"general engine" in msg, msg
    assert h.value is None
    with pytest.raises(_native.NativeError, match="4096"):
        sparc.DesignOperator(c.W, c.L, c.M, c.n, c.o0, c.o1).plan(prec)
    # a spatially coupled base matrix reaches the general engine without any override
    monkeypatch.delenv("SG_AMP_ENGINE", raising=False)
    W = sparc.sc_basic(np.array(ssc.P), 2, 4)
    Lr, Lc = W.shape
    Mr = 24
    o0, o1 = sparc.generate_ordering(W, Mr, c.L * c.M // Lc, ssc.DESIGN_SEED)
    rc, h = _create(W, c.L, c.M, Mr * Lr, o0, o1, prec)
    assert rc == _native.SG_ERR_UNSUPPORTED and b"4096" in lib.sg_last_error()
    assert h.value is None
    o0, o1 = sparc.generate_ordering(W, Mr, c.L * 2048 // Lc, ssc.DESIGN_SEED)
    rc, h = _create(W, c.L, 2048, Mr * Lr, o0, o1, prec)
    assert rc == _native.SG_OK and h.value
    assert lib.sg_amp_plan_engine(h, B) == 0
    lib.sg_amp_plan_destroy(h)
