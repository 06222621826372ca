"""Device-memory ownership of the dense plan, the complex plan and the LDPC graph handle (DevMem / DevPool,
csrc/device_mem.hpp), as tests/test_amp_workspace_gpu.py has it for sg_amp_plan: a handle that has grown, been
reused and shrunk computes, bit for bit, what a freshly created handle computes for the same call, and every
handle is destroyed.  The stand-alone host shims, whose scratch is a local DevMem, are pure functions of their
inputs: called twice and compared with the NumPy restatements.

Cases are those of the existing suites: the smallest dense design of tests/test_dense_gpu.py and the smallest
integrated fixture (integ0: L = 108, M = 64, n = 648); creg (K = 1) and cpsk4 (K = 4) of tests/csparc_cases.py;
802.11n rate 1/2, z = 27.  No allocation failure is provoked here: tests/test_device_mem_host.py covers those."""
import numpy as np
import pytest

import csparc_cases as cc
import csparc_concat_ref
import csparc_ref
from ldpc_sparc_amd import _native, sparc, sparc_new
from ldpc_sparc_amd.ldpc import code
from oracle import bp
from test_oracle_pin import integrated_case

pytestmark = pytest.mark.gpu

F64, F32 = _native.SG_F64, _native.SG_F32
OK = _native.SG_OK


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


# ---------------------------------------------------------------- dense plan

def _destroy_dense(d):
    for h in d._plans.values():
        assert _native.lib().sg_dense_plan_destroy(h) == OK
    d._plans = {}


@pytest.mark.parametrize("prec", [F64, F32])
def test_dense_plan_regrow_equals_fresh_plan(prec):
    """sg_dense_amp (host entry: workspace pool and staging buffer) at B = 2, 5, 2 on the design of
    test_single_iteration_vs_oracle."""
    rng = np.random.default_rng(7)
    L, M, n, t_max = 16, 32, 100, 3
    A = rng.normal(0, 1 / np.sqrt(n), (n, L * M))
    Y = rng.standard_normal((5, n)) * 3
    used = sparc_new.DenseDesign(A, 15.0, L, M)
    outs = []
    for B in (2, 5, 2):
        outs.append(sparc_new.dense_amp_batch(Y[:B], used, t_max, prec))
        fresh = sparc_new.DenseDesign(A, 15.0, L, M)
        _same(outs[-1], sparc_new.dense_amp_batch(Y[:B], fresh, t_max, prec))
        _destroy_dense(fresh)
    _same(outs[2], outs[0])
    _destroy_dense(used)


@pytest.mark.parametrize("prec", [F64, F32])
def test_dense_plan_integrated_decode_between(integrated_golden, prec):
    """The same B = 2, 5, 2 on the integ0 design with one sg_integrated_decode (the integrated pool, the staging
    buffer carved differently) before the last call."""
    y, A, L, M, P, graph, N, K, t_max = integrated_case(integrated_golden, "integ0")
    rng = np.random.default_rng(3)
    Y = np.stack([y + 0.1 * b * rng.standard_normal(y.size) for b in range(5)])
    c = code('802.11n', '1/2', 27)
    used = sparc_new.DenseDesign(A, P, L, M)
    calls = [("amp", 2), ("amp", 5), ("integ", 3), ("amp", 2)]
    outs = []
    for what, B in calls:
        def run(d):
            if what == "amp":
                return sparc_new.dense_amp_batch(Y[:B], d, 2, prec)
            return sparc_new.integrated_decode_batch(Y[:B], d, c, "integrated", t_max, precision=prec)
        outs.append(run(used))
        fresh = sparc_new.DenseDesign(A, P, L, M)
        _same(outs[-1], run(fresh))
        _destroy_dense(fresh)
    _same(outs[3], outs[0])
    _destroy_dense(used)


# ---------------------------------------------------------------- complex plan

def _destroy_camp(op):
    for h in op._plans.values():
        assert _native.lib().sg_camp_plan_destroy(h) == OK
    op._plans = {}


@pytest.mark.parametrize("name,K", [("creg", 1), ("cpsk4", 4)])
def test_complex_plan_recarve_equals_fresh_plan(name, K):
    """Decode at B = 2; soft output on (the workspace is carved again, with s_keep) and B = 3 with sg_camp_llr;
    soft output off and B = 2 again."""
    g = cc.golden()
    cp = cc.code_params(dict(next(c[1] for c in cc.CSPARC_CASES if c[0] == name)))
    W, L, M, n, o0, o1 = cc.design(g, name, cp)
    x = g[f"{name}_s0_x"]
    rng = np.random.RandomState(3)
    Y = np.stack([x + np.sqrt(v / 2) * (rng.randn(n) + 1j * rng.randn(n)) for v in (0.5, 1.0, 1.5)])
    t_max = 25

    def operator(soft):
        op = sparc.ComplexDesignOperator(W, L, M, n, o0, o1)
        op.soft_output(soft)
        return op

    def decode(op, B):
        return sparc.camp_decode_batch(Y[:B], op, cc.AWGN_VAR, t_max, 1e-6, 1, K)

    used = operator(False)
    first = decode(used, 2)
    fresh = operator(False)
    _same(first, decode(fresh, 2))
    _destroy_camp(fresh)

    used.soft_output(True)
    fresh = operator(True)
    _same(decode(used, 3), decode(fresh, 3))
    llr = sparc.camp_llr(used, 3, K, 0, L)
    assert np.all(np.isfinite(llr))
    assert llr.tobytes() == sparc.camp_llr(fresh, 3, K, 0, L).tobytes()
    assert llr.tobytes() == sparc.camp_llr(used, 3, K, 0, L).tobytes()  # its own staging each time
    _destroy_camp(fresh)

    used.soft_output(False)
    _same(decode(used, 2), first)
    _destroy_camp(used)


@pytest.mark.parametrize("K", [1, 4])
def test_standalone_shims_are_pure(K):
    """sg_section_mmse_psk / sg_section_softmax, sg_section_map_psk / sg_section_argmax and sg_section_llr_psk:
    the same inputs twice give the same bytes, within the existing bars of tests/csparc_ref.py (MMSE 1e-12,
    MAP identical) and of the enumeration (1e-12)."""
    g = cc.golden()
    M = cc.EST_M
    s, tau = g[f"est{K}_s"], float(g[f"est{K}_tau"])  # complex s for every K
    inputs = [s] if K > 1 else [s, s.real.copy()]     # real s at K = 1: the softmax shim
    for sv in inputs:
        mm = sparc.msg_vector_mmse_estimator(sv.copy(), tau, M, K)
        assert mm.tobytes() == sparc.msg_vector_mmse_estimator(sv.copy(), tau, M, K).tobytes()
        # (the restatement halves tau as for complex s; the estimator does not for real s)
        want = csparc_ref.mmse(sv.astype(complex), tau if np.iscomplexobj(sv) else 2 * tau, M, K)
        assert np.max(np.abs(mm - (want if np.iscomplexobj(mm) else want.real))) < 1e-12
    mp = sparc.msg_vector_map_estimator(s.copy(), M, K)
    assert mp.tobytes() == sparc.msg_vector_map_estimator(s.copy(), M, K).tobytes()
    idx, sym = csparc_ref.map_indices(s, M, K)
    assert np.array_equal(mp, sparc._msg_vector_from_indices(idx, sym, M, K))
    x = s / (tau / 2)
    p = sparc.section_llr_psk(x, 2.0, M, K, probs_only=True)  # tau = 2 for complex input: x = s exactly
    assert p.tobytes() == sparc.section_llr_psk(x, 2.0, M, K, probs_only=True).tobytes()
    enum = csparc_concat_ref.bit_probs(x if K > 2 else x.real.astype(complex), M, K)
    np.testing.assert_allclose(p.reshape(enum.shape), enum, rtol=0, atol=1e-12)


# ---------------------------------------------------------------- LDPC graph handle

def _destroy_graph(c):
    assert _native.lib().sg_ldpc_graph_destroy(c._graph) == OK
    c._graph = None


@pytest.fixture(scope="module")
def channel():
    c = code('802.11n', '1/2', 27)
    rng = np.random.default_rng(3)
    X = c.encode_batch(rng.integers(0, 2, (5, c.K)))
    ch = 2 * ((1 - 2 * X) + 0.7 * rng.standard_normal(X.shape)) / 0.49
    ch.setflags(write=False)
    return ch


@pytest.mark.parametrize("dectype,precision", [("sumprod2", "f64"), ("minsum", "f32")])
def test_graph_staging_regrow_equals_fresh_graph(channel, dectype, precision):
    """Host sg_ldpc_decode at B = 2, 5, 2: the table kernel in f64, the grouped kernel (whose tables share the
    graph's pool) in f32 min-sum."""
    used = code('802.11n', '1/2', 27)
    if precision == "f32":
        assert used.decode_kernel(dectype, F32).startswith("bp_grouped_minsum_kernel")
    outs = []
    for B in (2, 5, 2):
        outs.append(used.decode_batch(channel[:B], 20, dectype, 0.7, precision))
        fresh = code('802.11n', '1/2', 27)
        _same(outs[-1], fresh.decode_batch(channel[:B], 20, dectype, 0.7, precision))
        _destroy_graph(fresh)
    _same(outs[2], outs[0])
    _destroy_graph(used)


def _layered(c, ch, layer):
    app, it = np.zeros_like(ch), np.zeros(len(ch), np.int32)
    _native.check(_native.lib().sg_ldpc_decode_layered(
        c._device_graph(), _native.DECTYPES["sumprod2"], F64, layer, _native.ptr(np.ascontiguousarray(ch)), len(ch), 20,
        0.7, _native.ptr(app), _native.ptr(it)))
    return app, it


def test_layer_plans_on_one_graph(channel):
    """sg_ldpc_decode_layered at layer sizes 27, 9, 27 through one handle: the second size adds a plan to the
    handle's container, and the first plan's tables must be where they were."""
    used = code('802.11n', '1/2', 27)
    outs = []
    for layer in (27, 9, 27):
        outs.append(_layered(used, channel[:3], layer))
        fresh = code('802.11n', '1/2', 27)
        _same(outs[-1], _layered(fresh, channel[:3], layer))
        _destroy_graph(fresh)
    _same(outs[2], outs[0])
    _destroy_graph(used)


def test_lxfb_twice(oracle_built):
    c = code()
    L = np.random.default_rng(9).standard_normal(6) * 3
    oagg, oout = bp.lxfb(L, 1)
    for _ in range(2):
        agg, out = c.Lxfb(L, 1)
        np.testing.assert_allclose(agg, oagg, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(out, oout, rtol=1e-12, atol=1e-14)
