"""CPU tests of the AMP decode with known sections and the three-stage
concatenated decoder: the restatements of tests/amp_partial_ref.py against
oracle.sparc_ref.amp and on hand-made cases, the operating point at which the
final AMP pass shows its value, and the boundary of the new C-ABI symbols."""
import inspect
import os
import re

import numpy as np
import pytest

import amp_partial_ref as pr
import dct_concat_ref as ref
from ldpc_sparc_amd import _native, montecarlo
from oracle import sparc_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ldpc_sparc_amd.h")
SMALL = (32, 16, 128, 15.0)  # L, M, n, P


def _small(kind):
    L, M, n, P = SMALL
    if kind == "flat":
        W, o0, o1 = ref.flat_design(L, M, n, P, 5)
    else:
        W, o0, o1 = ref.pa_design(L, M, n, P, 5)
    Ab, Az = sparc_ref.dct_operators(W, L, M, n, o0, o1)
    true, beta0, Y = ref.batch(Ab, L, M, n, 3, [0.5, 1.0, 2.0], 13)
    return W, Ab, Az, true, beta0, Y


@pytest.mark.parametrize("phi_method", [1, 2])
@pytest.mark.parametrize("kind", ["flat", "pa"])
def test_no_known_section_is_the_oracle_bit_for_bit(kind, phi_method):
    L, M, n, _ = SMALL
    W, Ab, Az, true, beta0, Y = _small(kind)
    for b in range(3):
        want = sparc_ref.amp(Y[b], W, L, M, n, 1.0, 25, Ab, Az, beta0[b], 1e-6, phi_method)
        mp, tf, nmse, psi, bmap = pr.amp_partial(Y[b], W, L, M, n, 1.0, 25, Ab, Az, beta0[b], np.full(L, -1), 1e-6,
                                                 phi_method)
        assert tf == want[1]
        assert np.array_equal(bmap, want[0]) and np.array_equal(mp, np.argmax(want[0].reshape(L, M), 1))
        assert np.array_equal(nmse, want[2]) and np.array_equal(psi, want[3])


@pytest.mark.parametrize("kind", ["flat", "pa"])
def test_every_section_known_stops_at_once(kind):
    """psi0 = 0, z0 = y - A beta0 is the noise, every iteration returns the
    known one-hots: psi = 0 twice, and the loop stops at its first check."""
    L, M, n, _ = SMALL
    W, Ab, Az, true, beta0, Y = _small(kind)
    b = 2
    assert np.max(np.abs(Y[b] - Ab(beta0[b]))) > 1.0  # the noise is there
    mp, tf, nmse, psi, bmap = pr.amp_partial(Y[b], W, L, M, n, 1.0, 25, Ab, Az, beta0[b], true[b])
    assert tf == 2
    assert np.all(psi == 0) and np.all(nmse[1:] == 0) and np.all(nmse[0] == 1)
    assert np.array_equal(mp, true[b]) and np.array_equal(bmap, beta0[b])
    # a wrong known index stays, and costs 2 / L (or 2 / (L / Lc)) of NMSE
    known = true[b].copy()
    known[5] = (known[5] + 1) % M
    mp, tf, nmse, _, _ = pr.amp_partial(Y[b], W, L, M, n, 1.0, 25, Ab, Az, beta0[b], known)
    assert mp[5] == known[5] and np.array_equal(np.delete(mp, 5), np.delete(true[b], 5))
    Lc = np.asarray(W).size
    assert np.isclose(np.sum(nmse[-1]), 2.0 / (L / Lc), rtol=0, atol=1e-15)


def test_known_sections_on_a_straddling_layout():
    """N = 20, logM = 8, two blocks per codeword, two codewords: sections 0, 1
    lie in block 0, section 2 straddles (bits 16..23), sections 3, 4 in block
    1.  Codeword 0: block 1 unconverged; codeword 1: both converged."""
    N, logM, L_unp, L, mults, B, max_it = 20, 8, 1, 6, 2, 2, 50
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, (B, mults * N))
    app = np.where(bits == 1, -1.0, 1.0) * (0.5 + rng.random((B, mults * N)))
    it = np.array([4, max_it, 7, max_it - 1], dtype=np.int32)
    known = pr.known_sections(app.reshape(B * mults, N), it, max_it, B, mults, L, L_unp, logM)
    idx = bits.reshape(B, -1, logM) @ (1 << np.arange(logM)[::-1])  # sections of the 40 protected bits
    assert known.shape == (B, L)
    assert np.all(known[:, 0] == -1)  # unprotected
    assert known[0].tolist() == [-1, idx[0, 0], idx[0, 1], -1, -1, -1]  # straddled and the failed block's: -1
    assert known[1].tolist() == [-1] + idx[1].tolist()
    # it = max_it is "did not stop": the bound itself is unconverged, max_it - 1 converged
    assert known[1, 3] >= 0


def test_operating_point_shows_the_value_of_the_final_pass(oracle_built):
    """The feature's value, by the restatements alone.

    Operating point (amp_partial_ref.GEOM, point()): L = 144, M = 64, n = 864,
    P = 15, 36 unprotected sections, one 802.11n r1/2 z = 27 block in the other
    108; flat design of seed 2; 8 codewords drawn from default_rng(11);
    awgn_var = 4.0, t_max = 25, rtol 1e-6, phi_est_method 1, 200 sumprod2
    iterations.

    There BP converges on all 8 codewords and freezes all 108 protected
    sections correctly on each.  The two-stage composition leaves 32 wrong
    unprotected sections (per codeword 9, 1, 0, 2, 12, 1, 5, 2), the
    three-stage restatement 4 (1, 1, 0, 0, 2, 0, 0, 0)."""
    g, pt = pr.GEOM, pr.point()
    L, M, n, Lu = g["L"], g["M"], g["n"], g["L_unp"]
    two, three, frozen_ok, conv = [], [], [], []
    for b in range(pr.B_POINT):
        r = pr.three_stage(pt["Y"][b], pt["W"], L, M, n, pr.VAR, 25, pt["Ab"], pt["Az"], pt["beta0"][b], Lu, pt["c"])
        two.append(int(np.sum(r["map2"][:Lu] != pt["idx"][b, :Lu])))
        three.append(int(np.sum(r["map3"][:Lu] != pt["idx"][b, :Lu])))
        conv.append(bool(np.all(r["it"] < 200)))
        frozen_ok.append(bool(np.array_equal(r["known"][Lu:], pt["idx"][b, Lu:])))
    print(f"two-stage {two} = {sum(two)}, three-stage {three} = {sum(three)}, converged {conv}, frozen ok {frozen_ok}")
    assert sum(conv) >= 4 and any(e > 0 and cv for e, cv in zip(two, conv))
    assert sum(three) < sum(two)
    assert all(e3 <= e2 for e2, e3, ok in zip(two, three, frozen_ok) if ok)
    assert two == [9, 1, 0, 2, 12, 1, 5, 2] and three == [1, 1, 0, 0, 2, 0, 0, 0]  # (the docstring's figures)


def test_counters_restatement():
    app = np.array([[1.0, -1.0, 1.0, -2.0, 5.0]])
    cnt = pr.counters(np.array([3, 0, 9]), np.array([1, 0, 9]), app, [0, 1, 1], 2, 4, 3)
    assert cnt.tolist() == [1, 2, 1, 1, 1]  # 3 ^ 1 = one bit; info bit 2 wrong; the third section is protected


@pytest.mark.parametrize("name,arity", [("sg_amp_decode_partial_device", 14), ("sg_amp_decode_partial", 13),
                                        ("sg_concat_known_sections_device", 12)])
def test_symbols_declared_bound_and_exported(name, arity):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == arity
    bound = {n: (r, a) for n, r, a in _native.SIGNATURES}
    assert name in bound and len(bound[name][1]) == arity
    assert hasattr(_native.lib(), name)


def test_entry_points_without_a_device():
    """No GPU: SG_ERR_NO_DEVICE before anything else.  (With one, the same
    calls with their null handles are bad arguments.)"""
    lib = _native.lib()
    want = _native.SG_ERR_NO_DEVICE if _native.device_count() == 0 else _native.SG_ERR_BAD_ARG
    y, known = np.zeros(8), np.full(4, -1, np.int32)
    mp, tf, nm, ps = np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(2), np.zeros(1)
    p = _native.ptr
    assert lib.sg_amp_decode_partial_device(None, p(y), 1, p(known), None, 1.0, 2, 1e-6, 1, p(mp), p(tf), p(nm),
                                            p(ps), None) == want
    assert lib.sg_amp_decode_partial(None, p(y), 1, p(known), None, 1.0, 2, 1e-6, 1, p(mp), p(tf), p(nm),
                                     p(ps)) == want
    assert lib.sg_concat_known_sections_device(_native.SG_F64, None, None, 10, 1, 1, 8, 4, 0, 2, None, None) == want
    if want == _native.SG_ERR_NO_DEVICE:
        assert b"no GPU" in lib.sg_last_error()
    assert np.all(mp == 0)


def test_sweep_switch_default_and_tags(tmp_path):
    """final_amp is off by default, needs the DCT design, and keeps its
    checkpoints under a tag and parameters of its own (rehearsed with a CPU
    trial): a two-stage sweep neither finds nor resumes them."""
    import json
    sig = inspect.signature(montecarlo.concat_ber_sweep)
    assert sig.parameters["final_amp"].default is False and sig.parameters["final_t_max"].default is None
    g = pr.GEOM
    L, M, n, P, Lu = g["L"], g["M"], g["n"], g["P"], g["L_unp"]
    assert montecarlo.concat_checkpoint_tag(L, M, n, "dct3") == "concat_dct3_L144_M64_n864"
    assert montecarlo.concat_checkpoint_tag(L, M, n, "dct3") != montecarlo.concat_checkpoint_tag(L, M, n, "dct")

    def trial(point, first, nb, block):
        return np.array([nb * block, 3, 1, 1, 2], dtype=np.int64)
    kw = dict(codewords=16, block=16, ldpc=g["ldpc"], checkpoint_dir=str(tmp_path), trial=trial)
    with pytest.raises(ValueError, match="final_amp"):
        montecarlo.concat_ber_sweep(L, M, n, P, Lu, 1, [2.0], final_amp=True, **kw)
    montecarlo.concat_ber_sweep(L, M, n, P, Lu, 1, [2.0], design="dct", final_amp=True, final_t_max=9, **kw)
    path = tmp_path / "concat_dct3_L144_M64_n864_pt0.json"
    params = json.load(open(path))["params"]
    assert params["design"] == "dct3" and params["final_t_max"] == 9
    os.rename(path, tmp_path / "concat_dct_L144_M64_n864_pt0.json")
    with pytest.raises(ValueError, match="parameters"):
        montecarlo.concat_ber_sweep(L, M, n, P, Lu, 1, [2.0], design="dct", **kw)
    os.remove(tmp_path / "concat_dct_L144_M64_n864_pt0.json")
    montecarlo.concat_ber_sweep(L, M, n, P, Lu, 1, [2.0], design="dct", **kw)
    two = json.load(open(tmp_path / "concat_dct_L144_M64_n864_pt0.json"))["params"]
    assert two["design"] == "dct" and "final_t_max" not in two
