"""CPU tests of the layered BP schedule: the NumPy restatement
(tests/bp_layered_ref.py) on noiseless and noisy words, its convergence
against the flooding restatement (oracle/bp.py), and the host-only layer
validation of the C ABI (sg_ldpc_layer_check)."""
import numpy as np
import pytest

import bp_layered_ref as lr
from bp_layered_cases import awgn_llrs
from ldpc_sparc_amd import _native
from ldpc_sparc_amd.ldpc import code
from oracle import bp


def layer_check(c, layer):
    v, cd, i = (np.ascontiguousarray(a, np.int64) for a in (c.vdeg, c.cdeg, c.intrlv))
    L = _native.lib()
    rc = L.sg_ldpc_layer_check(_native.ptr(v), _native.ptr(cd), _native.ptr(i), c.Nv, c.Nc, c.Nmsg, int(layer))
    return rc, L.sg_last_error().decode()


@pytest.mark.parametrize("dectype", ["minsum", "sumprod2"])
@pytest.mark.parametrize("spec", [("802.11n", "1/2", 27), ("802.16", "5/6", 24)])
def test_noiseless_word_stops_at_once(spec, dectype):
    c = code(*spec)
    x = c.encode(np.random.default_rng(1).integers(0, 2, c.K))
    assert x.any()
    app, it = lr.layered(c.vdeg, c.cdeg, c.intrlv, 10 * (0.5 - x), c.z, 20, dectype)
    assert it == 0
    assert np.array_equal(app < 0, x == 1)


def test_serial_schedule_differs_from_flooding_but_agrees_in_decisions(oracle_built):
    """Layer size 1 (the smallest divisor of Nc, always valid: one check's
    ports are distinct variables) is the fully serial schedule: another
    message order than flooding, so other posteriors, but on a word both
    decode the same decisions."""
    c = code("802.11n", "1/2", 27)
    assert lr.layer_ok(c.vdeg, c.cdeg, c.intrlv, 1)
    X, ch = awgn_llrs(c, 1, 5.0, 2)  # (flooding stops at iteration 11, the serial schedule at 2)
    fapp, fit = bp.decode("minsum", ch[0], c.vdeg, c.cdeg, c.intrlv, 50, 0.7)
    lapp, lit = lr.layered(c.vdeg, c.cdeg, c.intrlv, ch[0], 1, 50, "minsum", 0.7)
    assert fit < 50 and lit < fit
    assert not np.array_equal(fapp, lapp)
    assert np.array_equal(fapp < 0, lapp < 0) and np.array_equal(lapp < 0, X[0] == 1)


def test_float32_restatement_is_float32_throughout():
    c = code("802.11n", "1/2", 27)
    _, ch = awgn_llrs(c, 4, 2.0, 3)
    for dectype in ("minsum", "sumprod2"):
        app, it = lr.layered(c.vdeg, c.cdeg, c.intrlv, ch, c.z, 5, dectype, 0.7, np.float32)
        assert app.dtype == np.float32 and it.dtype == np.int32


def test_restatement_refuses_what_the_decoder_refuses():
    c = code("802.11n", "1/2", 27)
    ch = np.ones((1, c.N))
    with pytest.raises(ValueError):
        lr.layered(c.vdeg, c.cdeg, c.intrlv, ch, c.z, 0, "minsum")
    with pytest.raises(ValueError):
        lr.layered(c.vdeg, c.cdeg, c.intrlv, ch, c.z, 5, "sumprod")
    with pytest.raises(ValueError):
        lr.layered(c.vdeg, c.cdeg, c.intrlv, ch, 2 * c.z, 5, "minsum")


@pytest.mark.parametrize("spec", [("802.11n", "1/2", 27), ("802.16", "5/6", 24)])
def test_layer_check_accepts_z(spec):
    c = code(*spec)
    rc, _ = layer_check(c, c.z)
    assert rc == _native.SG_OK
    assert lr.layer_ok(c.vdeg, c.cdeg, c.intrlv, c.z)


@pytest.mark.parametrize("spec", [("802.11n", "1/2", 27), ("802.16", "5/6", 24)])
def test_layer_check_rejects_two_block_rows_sharing_a_block(spec):
    c = code(*spec)
    mask = c.proto != -1
    assert (mask[0] & mask[1]).any()  # block rows 0 and 1 share a variable block
    rc, msg = layer_check(c, 2 * c.z)
    assert rc == _native.SG_ERR_INVALID
    # the first offender: layer 0, and the first variable of block row 1 that block row 0 has met
    coff, mvar = lr.edge_variables(c.vdeg, c.cdeg, c.intrlv)
    seen, first = set(), None
    for m in range(coff[2 * c.z]):
        if mvar[m] in seen:
            first = int(mvar[m])
            break
        seen.add(mvar[m])
    assert f"variable {first} occurs twice in layer 0 " in msg, msg
    assert not lr.layer_ok(c.vdeg, c.cdeg, c.intrlv, 2 * c.z)


def test_layer_check_rejects_a_layer_that_does_not_divide_nc():
    c = code("802.11n", "1/2", 27)
    for layer in (c.z + 1, 0, -3, c.Nc + c.z):
        rc, msg = layer_check(c, layer)
        assert rc == _native.SG_ERR_INVALID and "does not divide" in msg, (layer, msg)


def test_layer_check_validates_the_graph():
    c = code("802.11n", "1/2", 27)
    v, cd = (np.ascontiguousarray(a, np.int64) for a in (c.vdeg, c.cdeg))
    bad = np.ascontiguousarray(c.intrlv, np.int64).copy()
    bad[1] = bad[0]
    L = _native.lib()
    rc = L.sg_ldpc_layer_check(_native.ptr(v), _native.ptr(cd), _native.ptr(bad), c.Nv, c.Nc, c.Nmsg, c.z)
    assert rc == _native.SG_ERR_INVALID and b"permutation" in L.sg_last_error()


def test_schedule_keyword_is_checked_before_the_gpu():
    c = code("802.11n", "1/2", 27)
    with pytest.raises(NameError, match="Schedule unknown"):
        c.decode(np.ones(c.N), schedule="serial")
    with pytest.raises(NameError, match="Schedule unknown"):
        c.decode_batch(np.ones((1, c.N)), schedule="serial")
    from ldpc_sparc_amd import montecarlo as mc
    with pytest.raises(NameError, match="Schedule unknown"):
        mc.LdpcTrial(c, [1.0], schedule="serial")


def test_layered_converges_in_fewer_iterations_than_flooding(oracle_built):
    """802.11n r1/2 z=27, 256 random codewords at Eb/N0 2.0 dB, float64
    min-sum (factor 0.7), layers of z checks against the flooding restatement.
    Observed with this seed at max_it = 50: 98 codewords stop in both
    schedules before max_it with the right word, over which flooding executes
    2159 iterations and layered 462; at max_it = 10 flooding leaves 137 frame
    errors and layered 38 (at 50: 21 and 19).  Flooding's iteration counts are
    this high because its stopping rule (c_ldpc.c:191-197) waits for every
    check aggregate of the extrinsic messages, layered's for the syndrome of
    the posteriors."""
    c = code("802.11n", "1/2", 27)
    X, ch = awgn_llrs(c, 256, 2.0, 5)
    fapp, fit = bp.decode_batch("minsum", ch, c.vdeg, c.cdeg, c.intrlv, 50, 0.7)
    lapp, lit = lr.layered(c.vdeg, c.cdeg, c.intrlv, ch, c.z, 50, "minsum", 0.7)
    both = (fit < 50) & (lit < 50) & ((fapp < 0) == X).all(1) & ((lapp < 0) == X).all(1)
    f_total, l_total = int((fit[both] + 1).sum()), int((lit[both] + 1).sum())
    print(f"both decode {int(both.sum())}: flooding {f_total} iterations, layered {l_total}")
    assert both.sum() >= 64
    assert l_total < f_total
    f10, _ = bp.decode_batch("minsum", ch, c.vdeg, c.cdeg, c.intrlv, 10, 0.7)
    l10, _ = lr.layered(c.vdeg, c.cdeg, c.intrlv, ch, c.z, 10, "minsum", 0.7)
    f_fe, l_fe = int(((f10 < 0) != X).any(1).sum()), int(((l10 < 0) != X).any(1).sum())
    print(f"frame errors at max_it = 10: flooding {f_fe}, layered {l_fe}")
    assert l_fe <= f_fe


def test_campaign_checkpoints_keep_the_schedules_apart(tmp_path):
    """A flooding checkpoint is never resumed as layered: the layered campaign
    writes its own tag and carries the schedule in its parameters."""
    import json
    import os
    from ldpc_sparc_amd import montecarlo as mc

    class Fake:  # one frame error per codeword: every point ends after MIN_ERRORS codewords
        per_unit = True
        snrs = []

        def __call__(self, point, first_block, n_blocks, block):
            n = n_blocks * block
            return np.stack([np.ones(n, np.int64), np.ones(n, np.int64), np.ones(n, np.int64),
                             np.zeros(n, np.int64), np.zeros(n, np.int64)], 1)

    kw = dict(N_MEASUREMENTS=1, MIN_ERRORS=4, MAX_BLOCKS=64, block=4, blocks_per_round=1, dectype="minsum",
              max_it=10, checkpoint_dir=str(tmp_path))
    mc.ldpc_awgn_campaign("802.11n", "1/2", 27, trial=Fake(), **kw)
    mc.ldpc_awgn_campaign("802.11n", "1/2", 27, trial=Fake(), schedule="layered", **kw)
    names = sorted(os.listdir(tmp_path))
    assert names == ["ldpc_802.11n_12_27_A_layered_pt0.json", "ldpc_802.11n_12_27_A_pt0.json"]
    with open(tmp_path / names[0]) as f:
        assert json.load(f)["params"]["schedule"] == "layered"
    with open(tmp_path / names[1]) as f:
        assert "schedule" not in json.load(f)["params"]
    with pytest.raises(NameError, match="Schedule unknown"):
        mc.ldpc_awgn_campaign("802.11n", "1/2", 27, trial=Fake(), schedule="serial", **kw)
