"""CPU tests around the real K = 2 AMP decode with known section words and the
three-stage K = 2 decoder: the yardstick (tests/bpsk_partial_ref.py) is tied
to amp_bpsk_ref.amp_bpsk, its known-word rule is checked on cases with a
closed-form answer, the operating points are pinned, the cases that
tests/test_bpsk_partial_gpu.py decodes are stable under the one-ulp rule -- all
on the restatement alone -- and the new C-ABI entry points are declared, bound,
exported and refuse without a GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import amp_bpsk_ref as br
import bpsk_concat_ref as cr
import bpsk_partial_ref as ref
from ldpc_sparc_amd import _native, pipeline, sparc

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ldpc_sparc_amd.h")


# ---------------------------------------------------------------- the yardstick

@pytest.mark.parametrize("phi_method", [1, 2])
@pytest.mark.parametrize("name", ["flat", "pa", "bsc"])
def test_nothing_known_is_amp_bpsk(name, phi_method):
    """Exactly: every operation is amp_bpsk's, in its order (psi0 = 1.0 and z0 = y - 0)."""
    c = ref.case(name)
    got = ref.decode_batch(c.Y, c.W, c.L, c.M, c.n, c.var, c.t_max, c.Ab, c.Az, c.true, c.none, phi_method=phi_method)
    want = br.decode_batch(c.Y, c.W, c.L, c.M, c.n, c.var, c.t_max, c.Ab, c.Az, c.true, phi_method=phi_method)
    assert len(set(want[1].tolist())) >= 3
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def _small(name):
    W, L, M, n, o0, o1, words, Y, (Ab, Az) = cr.size_case(name)
    Lc = W.shape[-1] if W.ndim else 1
    return W, L, M, n, Ab, Az, words, Y, Lc


@pytest.mark.parametrize("name", ["m64", "pa256"])
def test_every_section_known(name):
    W, L, M, n, Ab, Az, words, Y, Lc = _small(name)
    mp, tf, nm, ps = ref.decode_batch(Y, W, L, M, n, 1.0, 10, Ab, Az, words, words)
    assert np.array_equal(mp, words) and np.all(tf == 2)
    assert np.all(ps == 0) and np.all(nm[:, 1:] == 0) and np.all(nm[:, 0] == 1)


@pytest.mark.parametrize("name", ["m64", "pa256"])
def test_a_wrong_known_word_costs_its_distance_and_comes_back(name):
    """Same location, opposite sign: |+1 - (-1)|^2 = 4; another location: 1 + 1 = 2 -- over the L / Lc sections of
    the word's column block."""
    W, L, M, n, Ab, Az, words, Y, Lc = _small(name)
    spc = L // Lc
    l = spc + 1 if Lc > 1 else 5
    for wrong, cost in ((words[0, l] ^ 1, 4.0), (((((words[0, l] >> 1) + 1) % M) << 1) | (words[0, l] & 1), 2.0)):
        known = words[:1].copy()
        known[0, l] = wrong
        mp, tf, nm, ps = ref.decode_batch(Y[:1], W, L, M, n, 1.0, 10, Ab, Az, words[:1], known)
        assert mp[0, l] == wrong and np.array_equal(mp, known)
        want = np.zeros(Lc)
        want[l // spc] = cost / spc
        assert np.array_equal(nm[0, 1:], np.broadcast_to(want, (9, Lc))) and np.all(ps == 0) and tf[0] == 2


# ---------------------------------------------------------------- operating points

@pytest.fixture(scope="module")
def points():
    out = {}

    def get(name):
        if name not in out:
            p = ref.point(name)
            rs = ref.point_three_stage(name)
            out[name] = (p, rs, ref.point_stable(name, p["Y"], rs))
        return out[name]
    return get


WRONG = {"A": ([0, 0, 0, 1, 4, 0, 1, 9], [1, 0, 0, 1, 1, 0, 0, 0], [14, 14, 12, 16, 14, 24, 10, 12]),
         "B": ([0, 0, 14, 2, 0, 3, 0, 0], [0, 0, 14, 0, 0, 0, 0, 0], [16, 8, 24, 14, 6, 6, 10, 13])}


@pytest.mark.parametrize("name", ["A", "B"])
def test_operating_points(points, name):
    """bpsk_concat_ref.POINTS through AMP -> BP -> AMP, wrong unprotected sections per codeword:
      A  two-stage [0, 0, 0, 1, 4, 0, 1, 9] = 15, three-stage [1, 0, 0, 1, 1, 0, 0, 0] = 3; every block converges;
         the final pass stops after [14, 14, 12, 16, 14, 24, 10, 12] iterations; counters [8, 47, 4, 47, 0] ->
         [8, 7, 3, 7, 0]
      B  two-stage [0, 0, 14, 2, 0, 3, 0, 0] = 19, three-stage [0, 0, 14, 0, 0, 0, 0, 0] = 14; codeword 2's block
         does not converge, nothing of it is known and its final pass is its first pass again; final pass
         [16, 8, 24, 14, 6, 6, 10, 13]; counters [8, 153, 3, 78, 75] -> [8, 133, 1, 58, 75]
    Every known word is right at both.  Not monotone per codeword: at A codeword 0 goes from 0 to 1."""
    p, rs, stable = points(name)
    Lu, words = p["L_unp"], p["words"]
    two = [ref.wrong_sections(r["map2"], words[b], Lu) for b, r in enumerate(rs)]
    three = [ref.wrong_sections(r["map3"], words[b], Lu) for b, r in enumerate(rs)]
    conv = np.array([bool(np.all(r["it"] < 200)) for r in rs])
    print(name, "two-stage", two, "three-stage", three, "converged", conv.tolist(), "final t", [r["t3"] for r in rs],
          "stable", stable.tolist())
    assert np.all(conv) if name == "A" else (np.any(conv) and not np.all(conv))
    assert sum(three) < sum(two)
    for b, r in enumerate(rs):
        kn = r["known"] >= 0
        assert np.array_equal(r["known"][kn], words[b][kn]) and not np.any(kn[:Lu])
        assert np.array_equal(r["map3"][kn], r["known"][kn])
        if not np.any(kn):
            assert np.array_equal(r["map3"], r["map2"])
    assert any(not np.any(r["known"] >= 0) for r in rs) == (name == "B")
    assert (two, three, [r["t3"] for r in rs]) == WRONG[name]
    assert np.count_nonzero(~stable) <= 2, stable


# ---------------------------------------------------------------- the GPU test's cases, on the restatement alone

@pytest.mark.parametrize("name,phi_method", ref.VS_NAMES)
def test_gpu_cases_are_stable_and_mixed(name, phi_method):
    """At most one of eight codewords moves by 1e-10 or more under a one-ulp change of y; the codewords stop at
    different iterations; at least five decode cleanly outside their given words (the f32 comparison's rows)."""
    c = ref.case(name)
    mp, tf, nm, ps = c.restatement(c.t_max, phi_method)
    mv = c.moves(c.t_max, phi_method)
    clean = np.all((mp == c.true) | (c.known >= 0), axis=1)
    print(name, phi_method, "t_final", tf.tolist(), "moves", mv, "clean", clean.tolist())
    assert np.count_nonzero(mv >= 1e-10) <= 1
    assert len(set(tf.tolist())) >= 3 and np.count_nonzero(clean) >= 5
    kn = c.known >= 0
    assert np.array_equal(mp[kn], c.known[kn])
    Lu = c.L_unp
    assert mp[2, Lu + ref.WRONG_LOC] >> 1 != c.true[2, Lu + ref.WRONG_LOC] >> 1
    assert mp[3, Lu + ref.WRONG_SIGN] == c.true[3, Lu + ref.WRONG_SIGN] ^ 1
    assert not np.any(kn[0]) and np.all(kn[1, Lu:]) and 0 < np.count_nonzero(kn[5]) < c.L


@pytest.mark.parametrize("name", ref.SIZE_NAMES)
def test_size_cases_are_stable(name):
    c = ref.case(name)
    mp, tf, nm, ps = c.restatement(c.t_max)
    assert np.all(c.moves(c.t_max) < 1e-10)
    assert np.count_nonzero(c.known >= 0) == c.nb * (c.L - c.L // 2)
    assert np.any(nm[:, 1:] > 0) and np.any(ps > 0)


# ---------------------------------------------------------------- ABI and Python surface

def _header_arity(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    return len([a for a in m.group(1).split(",") if a.strip()])


NEW = [("sg_amp_decode_bpsk_partial_device", 14), ("sg_amp_decode_bpsk_partial", 13)]


@pytest.mark.parametrize("name,arity", NEW)
def test_symbols_declared_bound_and_exported(name, arity):
    assert _header_arity(name) == arity
    bound = {n: (r, a) for n, r, a in _native.SIGNATURES}
    assert name in bound and len(bound[name][1]) == arity
    assert hasattr(_native.lib(), name)


def test_new_entry_points_without_a_device():
    if _native.device_count() > 0:
        pytest.skip("GPU present")
    lib, p = _native.lib(), _native.ptr
    y, kn, mp = np.zeros(8), np.full(4, -1, np.int32), np.full(4, -7, np.int32)
    assert lib.sg_amp_decode_bpsk_partial_device(None, p(y), 1, p(kn), None, 1.0, 5, 1e-6, 1, p(mp), None, None, None,
                                                 None) == _native.SG_ERR_NO_DEVICE
    assert b"no GPU" in lib.sg_last_error()
    assert lib.sg_amp_decode_bpsk_partial(None, p(y), 1, p(kn), None, 1.0, 5, 1e-6, 1, p(mp), None, None,
                                          None) == _native.SG_ERR_NO_DEVICE
    assert b"no GPU" in lib.sg_last_error()
    assert np.all(mp == -7)


def test_python_signatures():
    sig = inspect.signature(sparc.amp_decode_bpsk_partial_batch)
    assert list(sig.parameters) == ["Y", "op", "known_word", "awgn_var", "t_max", "rtol", "phi_est_method",
                                    "true_word", "precision"]
    assert sig.parameters["rtol"].default == 1e-6 and sig.parameters["true_word"].default is None
    cls = pipeline.DctBpskConcat3Pipeline
    assert issubclass(cls, pipeline.DctBpskConcatPipeline)
    assert inspect.signature(cls.__init__).parameters["final_t_max"].default is None
    assert "ConcatTrial(DctBpskConcat3Pipeline" in cls.__doc__ and "run_point" in cls.__doc__


def test_python_surface_refuses_a_complex_operator():
    W = np.array(15.0)
    o0, o1 = sparc.generate_ordering(W, 64, 16 * 8, 0, csparc=True)
    op = sparc.ComplexDesignOperator(W, 16, 8, 64, o0, o1)
    with pytest.raises(ValueError, match="real DesignOperator"):
        sparc.amp_decode_bpsk_partial_batch(np.zeros((1, 64)), op, np.full((1, 16), -1), 1.0, 5)
