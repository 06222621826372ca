"""Regrow and reuse of a plan's workspaces (ensure_ws, ensure_io of
amp_plan.cpp, IntegWs::ensure of integ_ws.hpp): a plan that has grown its batch, grown its NMSE
history, run the design operators in the same buffers and shrunk again computes,
bit for bit, what a freshly created plan computes for the same call.

Design: flat, L = 16, M = 32, on the regular engine (f32 and f64) and on the
general engine (SG_AMP_ENGINE=legacy while the plan is built); P, noise level
and seeds are those of tests/section_size_cases.py.  The integrated workspace:
case A of tests/dct_integrated_cases.py, its smallest."""
import numpy as np
import pytest

import dct_concat_ref as ref
import dct_integrated_cases as dc
import section_size_cases as ssc
from ldpc_sparc_amd import _native, sparc, sparc_new
from oracle import sparc_ref

pytestmark = pytest.mark.gpu

F64, F32 = _native.SG_F64, _native.SG_F32
L, M = 16, 32
N = ssc.n_of(L, M)
BMAX = 5
ENGINES = {"regular": 1, "general": 0}  # sg_amp_plan_engine codes
REFUSAL = "no decode through this plan yet (or its state was overwritten)"


@pytest.fixture(scope="module")
def words(oracle_built):
    """The design and BMAX received words, all of which the oracle decodes to the truth."""
    W, o0, o1 = ref.flat_design(L, M, N, ssc.P, ssc.DESIGN_SEED)
    Ab, Az = sparc_ref.dct_operators(W, L, M, N, o0, o1)
    true, beta0, Y = ref.batch(Ab, L, M, N, BMAX, ssc.SIGMA, ssc.BATCH_SEED)
    for b in range(BMAX):
        bmap, _, _, _ = sparc_ref.amp(Y[b], W, L, M, N, ssc.VAR, ssc.T_FULL, Ab, Az, beta0[b], 1e-6, 1)
        assert np.array_equal(np.argmax(bmap.reshape(L, M), 1), true[b])
    for a in (true, Y):
        a.setflags(write=False)
    return (W, o0, o1), true, Y


def _operator(monkeypatch, design, engine, prec):
    """A fresh operator whose plan of `prec` is built for `engine` (the builder reads SG_AMP_ENGINE)."""
    if engine == "general":
        monkeypatch.setenv("SG_AMP_ENGINE", "legacy")
    else:
        monkeypatch.delenv("SG_AMP_ENGINE", raising=False)
    op = sparc.DesignOperator(design[0], L, M, N, design[1], design[2])
    assert _native.lib().sg_amp_plan_engine(op.plan(prec), BMAX) == ENGINES[engine]
    return op


def _decode(op, true, Y, B, t_max, prec):
    return sparc.amp_decode_batch(Y[:B], op, ssc.VAR, t_max, rtol=1e-6, true_idx=true[:B], precision=prec)


def _same(got, want):
    for g, w in zip(got, want):  # MAP indices, t_final, NMSE history, psi
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def _destroy(op):
    for h in op._plans.values():
        assert _native.lib().sg_amp_plan_destroy(h) == _native.SG_OK
    op._plans = {}


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_decode_after_regrow_equals_fresh_plan(monkeypatch, words, engine, prec):
    design, true, Y = words
    calls = [(2, 4), (5, 4), (5, 9), (2, 4)]  # grow B, grow the NMSE history, back to the first call
    op = _operator(monkeypatch, design, engine, prec)
    outs = []
    for B, t_max in calls:
        outs.append(_decode(op, true, Y, B, t_max, prec))
        fresh = _operator(monkeypatch, design, engine, prec)
        _same(outs[-1], _decode(fresh, true, Y, B, t_max, prec))
        _destroy(fresh)
    _same(outs[3], outs[0])
    _destroy(op)


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_operators_between_decodes(monkeypatch, words, engine, prec):
    """sg_amp_apply at a larger B than any decode regrows the workspace under the decode's final state: the
    soft output is refused as it is after any apply, and the next decode is a fresh plan's."""
    design, true, Y = words
    op = _operator(monkeypatch, design, engine, prec)
    fresh = _operator(monkeypatch, design, engine, prec)
    want = _decode(fresh, true, Y, 2, 4, prec)
    _same(_decode(op, true, Y, 2, 4, prec), want)
    rng = np.random.RandomState(5)
    X, Z = rng.randn(BMAX + 2, L * M), rng.randn(BMAX + 2, N)
    ab, az = op.apply(X, False, prec), op.apply(Z, True, prec)
    assert ab.tobytes() == fresh.apply(X, False, prec).tobytes()
    assert az.tobytes() == fresh.apply(Z, True, prec).tobytes()
    with pytest.raises(_native.NativeError) as e:
        sparc.amp_llr(op, 2, 0, L, precision=prec)
    assert REFUSAL in str(e.value)
    _same(_decode(op, true, Y, 2, 4, prec), want)
    p = sparc.amp_llr(op, 2, 0, L, probs_only=True, precision=prec)
    _decode(fresh, true, Y, 2, 4, prec)
    assert p.tobytes() == sparc.amp_llr(fresh, 2, 0, L, probs_only=True, precision=prec).tobytes()
    _destroy(op)
    _destroy(fresh)


@pytest.mark.parametrize("prec", [F64, F32])
def test_integrated_workspace_regrow(oracle_built, prec):
    c = dc.build("A")
    used = sparc_new.DctDesign(dc.operator(c))
    for B in (1, 3, 1):
        fresh = sparc_new.DctDesign(dc.operator(c))
        bits, tau2 = sparc_new.integrated_decode_batch(c.Y[:B], used, c.code, "integrated", dc.T_MAX, precision=prec)
        fbits, ftau2 = sparc_new.integrated_decode_batch(c.Y[:B], fresh, c.code, "integrated", dc.T_MAX, precision=prec)
        assert bits.tobytes() == fbits.tobytes() and tau2.tobytes() == ftau2.tobytes()
        _destroy(fresh.op)
    _destroy(used.op)
