"""cw2_az recomputes beta_prev from s (amp_cw2.hip c2_beta) instead of reading
back a beta that cw2_ab stored over s.  Operands and operations are those of
cw2_ab, so the split engine's results are required to be the bits of the
library before the change: tests/golden/amp_cw2_beta_golden.npz holds map_idx,
t_final, NMSE and psi recorded from that library for the cases below
(`python tests/test_amp_cw2_beta_gpu.py OUT.npz` records them with whichever
library is loaded).  The same decodes are also held against the one-workgroup
engine (SG_AMP_CW2=0) with the bars of test_amp_cw2_gpu.py.

The C2 design of test_amp_cw2_gpu.py; the plan is told to assume one CU
(sg_amp_plan_set_cus), so that these tiny batches run the split engine, on two
streams where B >= 2 and t_max > 2 unless SG_AMP_PIPE=0.

  R = 1.5 (12 outputs per thread), B = 1, 2, 3 (one stream; even and uneven
  halves), t_max = 2 (only the t = 0 path and one recomputation) and 3;
  R = 1.3 (14 outputs per thread: the slice requested after the transform),
  B = 8, t_max = 25, the data of test_amp_pipelined_gpu.py: codewords stop, np
  goes 2 -> 4 and the staged engine takes over at iteration 17, reading s.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "amp_cw2_beta_golden.npz")
SEED_STOPS = 4  # test_amp_pipelined_gpu.py: the R = 1.3 batch of 8 that stops, switches np and hands over

# name -> (R, data seed, B, t_max)
CASES = {f"r15_b{B}_t{t}": (1.5, 5, B, t) for B in (1, 2, 3) for t in (2, 3)}
CASES["r13_b8_t25"] = (1.3, SEED_STOPS, 8, 25)

_designs = {}


def _design(R, seed):
    """Operator, true indices and received words of the largest batch of (R, seed), built once."""
    if (R, seed) not in _designs:
        from test_amp_cw2_gpu import _batch
        from ldpc_sparc_amd import _native
        Bmax = max(B for (r, s, B, _) in CASES.values() if (r, s) == (R, seed))
        op, true, Y = _batch(1024, 512, R, Bmax, 41, seed)
        _native.check(_native.lib().sg_amp_plan_set_cus(op.plan(_native.SG_F32), 1))
        _designs[R, seed] = (op, true, Y)
    return _designs[R, seed]


def _decode(name, env):
    """(map_idx, t_final, nmse, psi, [pipelined, engine, hand-over iteration]) of a case under SG_AMP_* = env."""
    import ctypes as ct
    from ldpc_sparc_amd import _native, sparc
    R, seed, B, t_max = CASES[name]
    op, true, Y = _design(R, seed)
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("SG_AMP_")}
    os.environ.update(env)
    try:
        m, t, n, p = sparc.amp_decode_batch(Y[:B], op, 1.0, t_max, true_idx=true[:B], precision=_native.SG_F32)
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)
    plan = op.plan(_native.SG_F32)
    piped = ct.c_int(-1)
    _native.check(_native.lib().sg_amp_last_pipelined(plan, ct.byref(piped)))
    last = _native.amp_last_decode(plan)
    return m, t, n, p, np.array([piped.value, last["engine"], last["handover_iter"]])


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("pipe", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_library_before(golden, name, pipe):
    """map_idx, t_final, NMSE and psi bit-identical to the recorded ones, on one stream and on two."""
    R, seed, B, t_max = CASES[name]
    m, t, n, p, info = _decode(name, {} if pipe else {"SG_AMP_PIPE": "0"})
    assert info[1] == 2  # the split engine
    assert info[0] == (1 if pipe and B >= 2 and t_max > 2 else 0)
    for k, v in (("map", m), ("tf", t), ("nmse", n), ("psi", p)):
        g = golden[f"{name}_{k}"]
        assert g.dtype == v.dtype and np.array_equal(g, v), (name, k, int(np.sum(g != v)))
    assert info[2] == golden[f"{name}_info"][2]  # hand-over at the same iteration
    if name == "r13_b8_t25":
        assert info[2] == 17 and (t <= 12).any() and (t > 17).any() and (t < 24).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_one_workgroup_engine(name):
    """The bars of test_amp_cw2_gpu.py: NMSE of the first iterations within 2e-4, psi after 1-3 iterations
    within 2e-6 relative, t_final within 1, decisions identical on >= 99.9 % of the sections and on every
    codeword that the one-workgroup engine decodes."""
    R, seed, B, t_max = CASES[name]
    _, true, _ = _design(R, seed)
    ma, ta, na, pa, ia = _decode(name, {})
    mb, tb, nb, pb, ib = _decode(name, {"SG_AMP_CW2": "0"})
    assert ia[1] == 2 and ib[1] == 2  # both per-codeword engines
    np.testing.assert_allclose(na[:, :4, 0], nb[:, :4, 0], atol=2e-4)
    if t_max <= 4:
        np.testing.assert_allclose(pa[:, 0], pb[:, 0], rtol=2e-6)
    assert (np.abs(ta - tb) <= 1).all(), (ta, tb)
    assert np.mean(ma == mb) >= 0.999
    dec_b = (mb == true[:B]).all(1)
    assert np.array_equal(ma[dec_b], mb[dec_b])
    if R <= 1.3:
        assert dec_b.mean() >= 0.75


if __name__ == "__main__":  # record the golden arrays with the loaded library
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    out = {}
    for name in sorted(CASES):
        one, two = _decode(name, {"SG_AMP_PIPE": "0"}), _decode(name, {})
        for a, b in zip(one[:4], two[:4]):
            assert np.array_equal(a, b), name  # one stream and two agree in the recording library
        for k, v in zip(("map", "tf", "nmse", "psi", "info"), two):
            out[f"{name}_{k}"] = v
        print(name, "t_final", two[1], "info", two[4])
    np.savez_compressed(sys.argv[1], **out)
