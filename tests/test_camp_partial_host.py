"""CPU tests of the complex AMP decode with known sections and the three-stage
concatenated K-PSK decoder: the restatements of tests/camp_partial_ref.py
against csparc_ref.amp and on hand-made cases, the operating point at which
the final AMP pass shows its value, and the boundary of the new C-ABI symbols."""
import inspect
import json
import os
import re

import numpy as np
import pytest

import camp_partial_ref as pr
import csparc_cases as cc
import csparc_concat_ref as cref
import csparc_ref
from ldpc_sparc_amd import _native, montecarlo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ldpc_sparc_amd.h")
NB = 2


def _case(name):
    """(W, L, M, n, K, t_max, phi, Ab, Az, idx, sym, beta0, Y) of a golden design, NB codewords at sigma 1 and 1.6."""
    _, cp, dp, _ = next(c for c in cc.CSPARC_CASES if c[0] == name)
    cp = cc.code_params(cp)
    K = cp['K'] if cp.get('modulated') else 1
    W, L, M, n, o0, o1 = cc.design(cc.golden(), name, cp)
    Ab, Az = csparc_ref.fft_operators(W, L, M, n, o0, o1)
    rng = np.random.RandomState(5)
    idx, sym = rng.randint(0, M, (NB, L)), rng.randint(0, K, (NB, L))
    beta0 = pr.one_hots(idx, sym, M, K)
    noise = (rng.randn(NB, n) + 1j * rng.randn(NB, n)) / np.sqrt(2)
    Y = np.stack([Ab(b) for b in beta0]) + np.array([1.0, 1.6])[:, None] * noise
    return W, L, M, n, K, dp['t_max'], dp.get('phi_est_method', 1), Ab, Az, idx, sym, beta0, Y


@pytest.mark.parametrize("name", ["creg", "cpsk4", "cpa4", "csc4"])
def test_no_known_section_is_the_plain_restatement_bit_for_bit(name):
    W, L, M, n, K, t_max, phi, Ab, Az, idx, sym, beta0, Y = _case(name)
    for b in range(NB):
        for method in (phi, 3 - phi):
            want = csparc_ref.amp(Y[b], W, L, M, n, K, Ab, Az, cc.AWGN_VAR, t_max, 1e-6, method, beta0[b])
            got = pr.amp_partial(Y[b], W, L, M, n, K, Ab, Az, cc.AWGN_VAR, t_max, beta0[b], np.full(L, -1),
                                 np.zeros(L, int), 1e-6, method)
            assert got[2] == want[2]
            for g, w in zip(got, want):
                assert np.array_equal(g, w)


@pytest.mark.parametrize("name", ["creg", "cpsk4", "cpa4", "csc4"])
def test_every_section_known_stops_at_once(name):
    """psi0 = 0, z0 = y - A beta0 is the noise, every iteration returns the known
    one-hots: psi = 0 twice, and the loop stops at its first check."""
    W, L, M, n, K, t_max, phi, Ab, Az, idx, sym, beta0, Y = _case(name)
    b = 1
    assert np.max(np.abs(Y[b] - Ab(beta0[b]))) > 1.0  # the noise is there
    mi, ms, tf, nmse, psi = pr.amp_partial(Y[b], W, L, M, n, K, Ab, Az, cc.AWGN_VAR, t_max, beta0[b], idx[b], sym[b])
    assert tf == 2 and np.all(psi == 0) and np.all(nmse[1] == 0) and np.all(nmse[0] == 1)
    assert np.array_equal(mi, idx[b]) and np.array_equal(ms, sym[b])
    # a wrong known location stays and costs 2 / L (or 2 / (L / Lc)) of NMSE; a wrong symbol |c_k - c_k'|^2
    ki = idx[b].copy()
    ki[5] = (ki[5] + 1) % M
    mi, ms, tf, nmse, _ = pr.amp_partial(Y[b], W, L, M, n, K, Ab, Az, cc.AWGN_VAR, t_max, beta0[b], ki, sym[b])
    Lc = W.shape[-1] if W.ndim else 1
    assert mi[5] == ki[5] and np.isclose(np.sum(nmse[-1]), 2.0 / (L / Lc), rtol=0, atol=1e-15)
    if K > 1:
        ks = sym[b].copy()
        ks[7] = (ks[7] + 1) % K
        mi, ms, tf, nmse, _ = pr.amp_partial(Y[b], W, L, M, n, K, Ab, Az, cc.AWGN_VAR, t_max, beta0[b], idx[b], ks)
        c = cref.constel(K)
        assert ms[7] == ks[7] and np.isclose(np.sum(nmse[-1]), abs(c[1] - c[0]) ** 2 / (L / Lc), rtol=0, atol=1e-15)


@pytest.mark.parametrize("K", [1, 2, 4, 64])
def test_unpack_words_inverts_section_words(K):
    rng = np.random.default_rng(K)
    idx, sym = rng.integers(0, 512, 300), rng.integers(0, K, 300)
    words = cref.section_words(idx, sym, K)
    words[::7] = -1
    gi, gs = pr.unpack_words(words, K)
    keep = words >= 0
    assert np.array_equal(gi[keep], idx[keep]) and np.array_equal(gs[keep], sym[keep])
    assert np.all(gi[~keep] == -1) and np.all(gs[~keep] == 0)


def test_operating_point_shows_the_value_of_the_final_pass(oracle_built):
    """The feature's value, by the restatements alone.

    Operating point (camp_partial_ref.GEOM, point()): L = 144, M = 16, K = 4
    (6 bits per section), n = 432 complex channel uses, P = 15, 36 unprotected
    sections, one 802.11n r1/2 z = 27 block in the other 108; flat design of
    seed 2; 8 codewords drawn from default_rng(11); awgn_var = 4.0, t_max = 25,
    rtol 1e-6, phi_est_method 1, 200 sumprod2 iterations.  (n and awgn_var
    were searched over n = 432 ... 600 and awgn_var = 1 ... 4: at the lower
    noise levels the first AMP leaves no unprotected section wrong.)

    There BP stops on its syndrome on all 8 codewords.  The two-stage
    composition leaves 24 wrong unprotected sections (per codeword 5, 1, 0, 0,
    9, 5, 0, 4), the three-stage restatement 6 (0, 1, 0, 1, 0, 2, 0, 2)."""
    g, pt = pr.GEOM, pr.point()
    L, M, K, n, Lu = g["L"], g["M"], g["K"], g["n"], g["L_unp"]
    two, three, conv = [], [], []
    for b in range(pr.B_POINT):
        r = pr.three_stage(pt["Y"][b], pt["W"], L, M, n, K, pt["Ab"], pt["Az"], pr.VAR, 25, pt["beta0"][b], Lu,
                           pt["c"])
        ti, ts = pt["idx"][b, :Lu], pt["sym"][b, :Lu]
        two.append(int(np.sum((r["idx2"][:Lu] != ti) | (r["sym2"][:Lu] != ts))))
        three.append(int(np.sum((r["idx3"][:Lu] != ti) | (r["sym3"][:Lu] != ts))))
        conv.append(bool(np.all(r["it"] < 200)))
    print(f"two-stage {two} = {sum(two)}, three-stage {three} = {sum(three)}, converged {conv}")
    assert sum(two) > 0 and sum(conv) >= pr.B_POINT // 2
    assert sum(three) < sum(two)
    assert two == [5, 1, 0, 0, 9, 5, 0, 4] and three == [0, 1, 0, 1, 0, 2, 0, 2]  # (the docstring's figures)


@pytest.mark.parametrize("name,arity", [("sg_camp_decode_partial_device", 19), ("sg_camp_decode_partial", 18),
                                        ("sg_psk_unpack_sections_device", 7)])
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
    lib, p = _native.lib(), _native.ptr
    want = _native.SG_ERR_NO_DEVICE if _native.device_count() == 0 else _native.SG_ERR_BAD_ARG
    y, known = np.zeros(16), np.full(4, -1, np.int32)
    mp, tf, nm, ps = np.zeros(4, np.int32), np.zeros(1, np.int32), np.zeros(2), np.zeros(1)
    assert lib.sg_camp_decode_partial_device(None, p(y), 1, 1, None, p(known), None, None, None, 1.0, 2, 1e-6, 1, p(mp),
                                             None, p(tf), p(nm), p(ps), None) == want
    assert lib.sg_camp_decode_partial(None, p(y), 1, 1, None, p(known), None, None, None, 1.0, 2, 1e-6, 1, p(mp), None,
                                      p(tf), p(nm), p(ps)) == want
    assert lib.sg_psk_unpack_sections_device(None, 1, 4, 2, None, None, None) == want
    if want == _native.SG_ERR_NO_DEVICE:
        assert b"no GPU" in lib.sg_last_error()
    assert np.all(mp == 0)


def test_sweep_switch_and_tags(tmp_path):
    """final_amp with the FFT design keeps its checkpoints under a tag and
    parameters of its own (rehearsed with a CPU trial): a two-stage sweep
    neither finds nor resumes them; the dense design still refuses it."""
    sig = inspect.signature(montecarlo.concat_ber_sweep)
    assert sig.parameters["final_amp"].default is False and sig.parameters["final_t_max"].default is None
    g = pr.GEOM
    L, M, K, n, P, Lu = g["L"], g["M"], g["K"], g["n"], g["P"], g["L_unp"]
    assert montecarlo.concat_checkpoint_tag(L, M, n, "fft3", K) == "concat_fft3_L144_M16_K4_n432"
    assert montecarlo.concat_checkpoint_tag(L, M, n, "fft", K) == "concat_fft_L144_M16_K4_n432"

    def trial(point, first, nb, block):
        return np.array([nb * block, 3, 1, 1, 2], dtype=np.int64)
    kw = dict(codewords=16, block=16, ldpc=g["ldpc"], checkpoint_dir=str(tmp_path), trial=trial, precision="f64")
    with pytest.raises(ValueError, match="final_amp"):
        montecarlo.concat_ber_sweep(L, M, n, P, Lu, 1, [2.0], final_amp=True, **kw)
    montecarlo.concat_ber_sweep(L, M, n, P, Lu, 1, [2.0], design="fft", K=K, final_amp=True, final_t_max=9, **kw)
    path = tmp_path / "concat_fft3_L144_M16_K4_n432_pt0.json"
    params = json.load(open(path))["params"]
    assert params["design"] == "fft3" and params["final_t_max"] == 9 and params["K"] == K
    os.rename(path, tmp_path / "concat_fft_L144_M16_K4_n432_pt0.json")
    with pytest.raises(ValueError, match="parameters"):
        montecarlo.concat_ber_sweep(L, M, n, P, Lu, 1, [2.0], design="fft", K=K, **kw)
    os.remove(tmp_path / "concat_fft_L144_M16_K4_n432_pt0.json")
    montecarlo.concat_ber_sweep(L, M, n, P, Lu, 1, [2.0], design="fft", K=K, **kw)
    two = json.load(open(tmp_path / "concat_fft_L144_M16_K4_n432_pt0.json"))["params"]
    assert two["design"] == "fft" and "final_t_max" not in two
