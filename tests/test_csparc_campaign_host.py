"""montecarlo.run_point with trials that declare their own counter length
(`nc`, as CSparcTrial's seven counters), on the CPU with fake trials: totals,
the exact per-codeword stopping rule, checkpoints, and the unchanged
five-counter default."""
import json

import numpy as np

from ldpc_sparc_amd import montecarlo as mc


def _row(point, unit, nc):
    """Deterministic counters of codeword `unit`: a frame error every third codeword."""
    err = int(unit % 3 == 2)
    r = [1, 2 * err, err, 5 + unit % 4, 3 * err, err, unit % 2]
    return np.array((r + [0] * nc)[:nc], dtype=np.int64)


class FakeTrial:
    def __init__(self, nc=None, per_unit=False):
        if nc is not None:
            self.nc = nc
        self.width = nc if nc is not None else mc.NC
        self.per_unit = per_unit
        self.calls = []

    def __call__(self, point, first_block, n_blocks, block):
        self.calls.append((point, first_block, n_blocks, block))
        units = range(first_block * block, (first_block + n_blocks) * block)
        rows = np.stack([_row(point, u, self.width) for u in units])
        return rows if self.per_unit else rows.sum(axis=0)


def _expected(units, nc):
    return np.stack([_row(0, u, nc) for u in range(units)]).sum(axis=0)


def _run(trial, **kw):
    args = dict(block=4, blocks_per_round=2, rank=0, world=1, agg=mc.Aggregator())
    args.update(kw)
    return mc.run_point(trial, 0, **args)


def test_nc7_totals_block_counters():
    tot = _run(FakeTrial(7), max_units=24)
    assert tot.shape == (7,) and tot.dtype == np.int64
    assert np.array_equal(tot, _expected(24, 7))


def test_nc7_two_ranks_sum_to_one():
    # one round of two blocks; each rank alone (the `none` aggregator) returns its own block's counters
    one = _run(FakeTrial(7))
    parts = [_run(FakeTrial(7), rank=r, world=2) for r in range(2)]
    assert np.array_equal(parts[0] + parts[1], one)
    assert np.array_equal(one, _expected(8, 7))


def test_nc7_per_unit_stops_at_the_exact_codeword():
    # frame errors at codewords 2, 5, 8, 11, ...: the 4th is codeword 11, i.e. 12 codewords
    tot = _run(FakeTrial(7, per_unit=True), min_errors=4, max_units=1000)
    assert np.array_equal(tot, _expected(12, 7))
    assert tot[0] == 12 and tot[2] == 4
    # the block-counter form of the same trial can only stop at a round boundary (8 codewords per round)
    coarse = _run(FakeTrial(7), min_errors=4, max_units=1000)
    assert np.array_equal(coarse, _expected(16, 7))


def test_nc7_per_unit_max_units_cut():
    tot = _run(FakeTrial(7, per_unit=True), max_units=10)
    assert np.array_equal(tot, _expected(10, 7))


def test_nc7_checkpoint_round_trip(tmp_path):
    ck = str(tmp_path)
    for per_unit in (False, True):
        tag = f"fake{int(per_unit)}"
        first = _run(FakeTrial(7, per_unit), max_units=24, checkpoint_dir=ck, tag=tag, max_rounds=1)
        assert np.array_equal(first, _expected(8, 7))
        with open(mc._ckpt_path(ck, tag, 0)) as f:
            st = json.load(f)
        assert len(st["counts"]) == 7 and st["next_block"] == 2 and not st["done"]
        resumed_trial = FakeTrial(7, per_unit)
        resumed = _run(resumed_trial, max_units=24, checkpoint_dir=ck, tag=tag)
        assert resumed_trial.calls[0][1] == 2  # continued at block 2, nothing redone
        assert np.array_equal(resumed, _run(FakeTrial(7, per_unit), max_units=24))
        assert np.array_equal(resumed, _expected(24, 7))


def test_trial_without_nc_keeps_five_counters(tmp_path):
    assert mc.NC == 5
    for per_unit in (False, True):
        tot = _run(FakeTrial(None, per_unit), max_units=16, checkpoint_dir=str(tmp_path), tag=f"plain{int(per_unit)}")
        assert tot.shape == (5,)
        assert np.array_equal(tot, _expected(16, 5))
        with open(mc._ckpt_path(str(tmp_path), f"plain{int(per_unit)}", 0)) as f:
            assert len(json.load(f)["counts"]) == 5


def test_csparc_trial_declares_seven_counters():
    assert mc.CSparcTrial.nc == 7
