"""The pipelined split engine (capi_amp.cpp Cw2Pipe: two half-batches on two
streams) against the same decode on one stream (SG_AMP_PIPE=0): bit-identical
map_idx, t_final, nmse and psi, on the C2 design fixtures of
test_amp_cw2_gpu.py.  Each side runs in a fresh child process; the plan is told
to assume one CU (sg_amp_plan_set_cus), so that the split engine and, by
default, its pipelined form run at these small batches with every batch-level
decision (poll, np 2 -> 4, hand-over) left automatic."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# argv: output .npz, JSON {"R", "seed": data seed, "decodes": [[B, t_max], ...], "prof": level or 0}
CHILD = r"""
import ctypes as ct, json, sys
import numpy as np
sys.path.insert(0, "tests")
from test_amp_cw2_gpu import _batch
from ldpc_sparc_amd import _native, sparc
out, spec = sys.argv[1], json.loads(sys.argv[2])
Bmax = max(b for b, _ in spec["decodes"])
op, true, Y = _batch(1024, 512, spec["R"], Bmax, 41, spec["seed"])
plan = op.plan(_native.SG_F32)
_native.check(_native.lib().sg_amp_plan_set_cus(plan, 1))
res = {}
for i, (B, t_max) in enumerate(spec["decodes"]):
    prof = _native.Profiler(spec["prof"]) if spec["prof"] else None
    m, t, n, p = sparc.amp_decode_batch(Y[:B], op, 1.0, t_max, true_idx=true[:B], precision=_native.SG_F32)
    ph = prof.stop() if prof else {}
    piped = ct.c_int(-1)
    _native.check(_native.lib().sg_amp_last_pipelined(plan, ct.byref(piped)))
    last = _native.amp_last_decode(plan)
    res.update({f"map{i}": m, f"tf{i}": t, f"nmse{i}": n, f"psi{i}": p,
                f"info{i}": np.array([piped.value, last["engine"], last["handover_iter"]]),
                f"iter{i}": np.array(ph.get("amp_iter", (0.0, 0)))})
np.savez(out, **res)
"""


# data seed of the R = 1.3 batch of 8: its codewords stop after 12 to 19 iterations, one before the poll after
# iteration 11 and more than half before the one after 15 (seed 5, the R = 1.5 cases', has exactly half active
# there and never hands over)
SEED_STOPS = 4


def _run(tmp_path, tag, pipe, spec):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SG_AMP_")}
    if not pipe:
        env["SG_AMP_PIPE"] = "0"
    out = str(tmp_path / f"{tag}.npz")
    r = subprocess.run([sys.executable, "-c", CHILD, out, json.dumps(spec)], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def _both(tmp_path, spec):
    one, two = _run(tmp_path, "one", False, spec), _run(tmp_path, "two", True, spec)
    for i, (B, _) in enumerate(spec["decodes"]):
        assert one[f"info{i}"][0] == 0 and one[f"info{i}"][1] == 2  # split engine, one stream
        assert two[f"info{i}"][0] == (1 if B >= 2 else 0) and two[f"info{i}"][1] == 2
        for k in ("map", "tf", "nmse", "psi"):  # bit-identical (NaN-free: every entry is written)
            assert np.array_equal(one[f"{k}{i}"], two[f"{k}{i}"]), (k, i)
        assert one[f"info{i}"][2] == two[f"info{i}"][2]  # hand-over at the same iteration
    return one, two


@pytest.mark.parametrize("B", [2, 3])
def test_halves_even_and_uneven(tmp_path, B):
    """R = 1.5, t_max = 4: even and uneven halves and the offset start at iteration 0."""
    _both(tmp_path, {"R": 1.5, "seed": 5, "decodes": [[B, 4]], "prof": 0})


def test_stops_poll_parts_and_handover(tmp_path):
    """B = 8, R = 1.3, t_max = 25: codewords stop, so the poll, the switch to four parts per codeword and the
    hand-over to the staged engine all happen, at the same iterations on one and on two streams."""
    one, _ = _both(tmp_path, {"R": 1.3, "seed": SEED_STOPS, "decodes": [[8, 25]], "prof": 0})
    print("t_final", one["tf0"], "hand-over at", one["info0"][2])
    assert (one["tf0"] < 24).all()  # stopped by the rule, not by t_max
    assert (one["tf0"] <= 12).any()  # a codeword has stopped at the poll after iteration 11: np = 4 from 13 on
    assert one["info0"][2] == 17  # under half active at the poll after iteration 15: staged from 17 on
    assert (one["tf0"] > 17).any()  # and the staged engine still had codewords to finish


def test_second_stream_reused(tmp_path):
    """Two decodes on one plan, then B = 1 (one stream), then B = 8 again: the plan's second stream and events
    serve every decode."""
    one, two = _both(tmp_path, {"R": 1.3, "seed": SEED_STOPS, "decodes": [[8, 25], [8, 25], [1, 25], [8, 25]],
                                "prof": 0})
    for k in ("map", "tf", "nmse", "psi"):
        assert np.array_equal(two[f"{k}0"], two[f"{k}1"]) and np.array_equal(two[f"{k}0"], two[f"{k}3"])


# The single-stream amp_iter sum of this decode, five fresh processes on the parent commit:
# 2.064, 2.038, 2.085, 2.176, 2.057 ms; largest run-to-run ratio 1.068.  Margin: twice that excess, 13.6 %.
# (A double count of the two halves would show as about 2x.)
ITER_SUM_MARGIN = 2 * 0.068


def test_profiler_counts_a_pipelined_iteration_once(tmp_path):
    """Level-2 profiler, B = 3, R = 1.5, t_max = 4: as many amp_iter scopes as on one stream, and their summed
    time (the union of the two halves' intervals) not above the single-stream sum plus the margin."""
    one, two = _both(tmp_path, {"R": 1.5, "seed": 5, "decodes": [[3, 4]], "prof": 2})
    print("amp_iter (ms, n): one stream", one["iter0"], "two streams", two["iter0"])
    assert one["iter0"][1] == two["iter0"][1] == 3
    assert two["iter0"][0] <= one["iter0"][0] * (1 + ITER_SUM_MARGIN)
