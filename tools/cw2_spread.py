"""Start ramp and drain tail of the split engine's two big launches: one C2
batch decode (bench design, B = 256, single stream: SG_AMP_PIPE=0) with the
C2_TP entry / exit stamps of every workgroup (amp_cw2.hip stamps 10 / 11 of
cw2_ab, 42 / 43 of cw2_az; last iteration), then per kernel the spread of the
start and of the end stamps over the grid and the mean CU-slot time that is
idle inside the launch: mean(start - first start) + mean(last end - end).
The shader clock is read per CU (or CU pair) and the CUs' clocks do not
agree, so the workgroups are grouped by clock (start stamps within a few
workgroup lengths of each other).  A group of two to four workgroups is one
CU or CU pair and its figures are meaningful; clocks that happen to lie close
chain into larger groups, which are counted and left out of the mean.
CW2_SPREAD_RAW=path.npy also saves the stamps.  Needs a library with the
stamps compiled in (make DIAG=1, loaded through LDPC_SPARC_AMD_LIB).

usage: python tools/cw2_spread.py [B] [R]"""
import ctypes as ct
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["SG_AMP_TPROF"] = "1"
os.environ["SG_AMP_PIPE"] = "0"
from ldpc_sparc_amd import _native, sparc  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
R = float(sys.argv[2]) if len(sys.argv) > 2 else 1.5
L, M = 1024, 512
n = int(round(L * 9 / R))
W = np.array(15.0)
o0, o1 = sparc.generate_ordering(W, n, L * M, 0)
op = sparc.DesignOperator(W, L, M, n, o0, o1)
rng = np.random.default_rng(1)
true = rng.integers(0, M, (B, L))
beta0 = np.zeros((B, L * M))
beta0[np.arange(B)[:, None], np.arange(L) * M + true] = 1
Y = op.apply(beta0, False) + rng.standard_normal((B, n))
lib = _native.lib()
plan = op.plan(_native.SG_F32)
sparc.amp_decode_batch(Y, op, 1.0, 6, true_idx=true, precision=_native.SG_F32)
items = ct.c_size_t()
_native.check(lib.sg_amp_stage_raw(plan, 0, None, ct.byref(items)))
out = np.zeros((items.value, 10), np.uint64)
_native.check(lib.sg_amp_stage_raw(plan, 0, out.ctypes.data_as(ct.POINTER(ct.c_uint64)), ct.byref(items)))
st = out[:, :8].reshape(-1)[:2 * B * 64].reshape(2 * B, 64).astype(np.int64)
if os.environ.get("CW2_SPREAD_RAW"):
    np.save(os.environ["CW2_SPREAD_RAW"], st)


def report(name, a, b):
    s, e = st[:, a], st[:, b]
    if not ((s > 0) & (e > s)).all():
        print(f"{name}: stamps missing (library without C2_STAMPS?)")
        return
    dur = (e - s).mean()
    # clock domains: workgroups whose start stamps lie within a few workgroup lengths of each other
    order = np.argsort(s)
    cuts = np.nonzero(np.diff(s[order]) > 4 * dur)[0] + 1
    xi, wsum, mixed = 0.0, 0, 0
    for g, ix in enumerate(np.split(order, cuts)):
        if not 2 <= len(ix) <= 4:
            mixed += len(ix)
            continue
        ss, ee = s[ix], e[ix]
        ramp, tail = ss.max() - ss.min(), ee.max() - ee.min()
        idle = (ss - ss.min()).mean() + (ee.max() - ee).mean()
        span = ee.max() - ss.min()
        xi += idle / span * len(ix)
        wsum += len(ix)
        print(f"{name} clock {g:2d} ({len(ix):3d} workgroups, ids mod 8: {sorted(set((ix % 8).tolist()))}) workgroup "
              f"{(ee - ss).mean():8.0f} cyc  start spread {ramp:7d}  end spread {tail:7d}  span {span:8d}  "
              f"idle slot {idle:7.0f} cyc = {idle / span:6.2%} of the span")
    print(f"{name} idle slot share, mean over the {wsum} workgroups of the one-clock groups: {xi / max(wsum, 1):.2%}  "
          f"(workgroup mean {dur:.0f} cycles; {mixed} workgroups in groups of several clocks left out)")


report("cw2_ab", 10, 11)
report("cw2_az", 42, 43)
