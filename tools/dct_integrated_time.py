#!/usr/bin/env python
"""Timing of the integrated AMP <-> BP decoder on the sub-sampled DCT design
(pipeline.DctIntegratedPipeline, sg_amp_integrated_decode_device) against the
same decoder on the dense Gaussian design (sg_integrated_decode_device):
L = 1024, M = 512, n = 9216, LDPC 802.16 r1/2 z = 96 (N = 2304, four blocks
per codeword), B = 256, single precision, t_max = 25, mode `integrated`,
6 inner and 200 final sumprod2 iterations, batches generated on the GPU.  The
dense design's f32 matrix is 19 GB.

Steps, each in a child process of its own under a time limit, in order; the
first step that fails or runs out of time ends the run (nothing further is
started on the GPU):

  dct, dense
        codewords/s of one decode of a device batch: host clock around `steps`
        decodes that end in a device synchronise, after a warm-up decode;
        median of `repeats` windows;
  dct_split
        per-phase device time of one DCT decode from sg_profile_* (HIP events
        around every launch, which hold the stream back: shares, not a rate):
        operator pair (ab_*, az_*), section kernel (eta), residual (control),
        BP (bp_flood), BP -> beta (integ_glue), differentiated eta (integ_deta).

The two designs are different codes of one ensemble at the same noise level;
the decoder, its iteration counts and the batch are the same.  Results go to
profiles/dct_integrated.json with the library's hash.  Needs a GPU.

    python tools/dct_integrated_time.py [--batch 256] [--steps 2] [--repeats 5] [--var 1.0]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

L, M, N_CH, P, MULTS = 1024, 512, 9216, 15.0, 4
LDPC = ("802.16", "1/2", 96)
T_MAX, BP_ITS, BP_ITS_FINAL, MODE = 25, 6, 200, "integrated"
STEPS = ["dct", "dct_split", "dense"]
LIMIT_S = {"dct": 240, "dct_split": 240, "dense": 480}  # per child, its plan build and warm-up included


def _windows(fn, steps, repeats):
    from ldpc_sparc_amd import _native
    out = []
    for _ in range(repeats):
        _native.device_synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        _native.device_synchronize()
        out.append(time.perf_counter() - t0)
    return out


def run_step(step, a):
    from ldpc_sparc_amd import _native
    from ldpc_sparc_amd.pipeline import ConcatPipeline, DctIntegratedPipeline
    _native.require_gpu()
    B = a.batch
    if step == "dense":
        pipe = ConcatPipeline(L, M, N_CH, P, 0, MULTS, ldpc=LDPC, design_seed=1234, precision="f32", t_max=T_MAX)
        d_bits = _native.DeviceBuffer(B * MULTS * pipe.c.K)
        lib = _native.lib()

        def decode():
            _native.check(lib.sg_integrated_decode_device(pipe.plan, pipe.graph, _native.INTEGRATED_MODES[MODE],
                                                          pipe.c.K, pipe.d_y.ptr, B, T_MAX, BP_ITS, BP_ITS_FINAL,
                                                          d_bits.ptr, None, None))
    else:
        pipe = DctIntegratedPipeline(L, M, N_CH, P, ldpc=LDPC, design_seed=1234, precision="f32", t_max=T_MAX,
                                     mode=MODE, bp_its=BP_ITS, bp_its_final=BP_ITS_FINAL)
        decode = pipe.decode
    pipe.make_batch_device(B, a.var, 5000, 0)
    pipe.reset_counts()
    decode()  # warm-up: workspace, code objects
    _native.device_synchronize()
    res = {"step": step, "batch": B, "steps": a.steps, "repeats": a.repeats, "awgn_var": a.var}
    if step == "dct":
        cnt = pipe.counts()
        res.update(warmup_counts=[int(c) for c in cnt], warmup_ber=float(cnt[1]) / (cnt[0] * MULTS * pipe.c.K))
    if step == "dct_split":
        prof = _native.Profiler(1)
        decode()
        ph = prof.stop()
        total = sum(ms for ms, _ in ph.values())
        groups = {"operator_pair": ("ab_passA", "ab_passB", "az_passA", "az_passB"), "section_kernel": ("eta",),
                  "residual": ("control",), "bp": ("bp_flood",), "bp_to_beta": ("integ_glue",),
                  "deta": ("integ_deta",)}
        res.update(phases_ms={k: v[0] for k, v in ph.items()}, launches={k: v[1] for k, v in ph.items()},
                   per_iteration_ms={g: sum(ph.get(k, (0.0, 0))[0] for k in ks) / T_MAX for g, ks in groups.items()},
                   share={g: sum(ph.get(k, (0.0, 0))[0] for k in ks) / total for g, ks in groups.items()},
                   profiled_total_ms=total)
        return res
    t = _windows(decode, a.steps, a.repeats)
    res.update(window_seconds=t, codewords_per_s=B * a.steps / float(np.median(t)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--var", type=float, default=1.0)
    ap.add_argument("--only", nargs="*", default=STEPS, choices=STEPS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dct_integrated.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)      # child mode: one step, result to --json
    ap.add_argument("--json", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        with open(a.json, "w") as f:
            json.dump(run_step(a.step, a), f)
        return 0
    from ldpc_sparc_amd import _native
    with open(_native.LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    results, failed = {}, None
    for step in a.only:
        limit = LIMIT_S[step]
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "step.json")
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--json", path, "--batch", str(a.batch), "--steps", str(a.steps), "--repeats", str(a.repeats),
                   "--var", str(a.var)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:  # a fault, an abort or the time limit: start nothing more on the GPU
                failed = {"step": step, "exit_status": rc, "limit_s": limit}
                break
            with open(path) as f:
                results[step] = json.load(f)
        print(json.dumps({k: v for k, v in results[step].items() if not k.endswith("window_seconds")}), flush=True)
    out = {"geometry": {"L": L, "M": M, "n": N_CH, "P": P, "ldpc": list(LDPC), "blocks_per_codeword": MULTS,
                        "t_max": T_MAX, "bp_its": BP_ITS, "bp_its_final": BP_ITS_FINAL, "mode": MODE,
                        "precision": "f32"},
           "lib_sha256": lib_hash,
           "what": "host clock around `steps` decodes of one device batch ending in a device synchronise, after a "
                   "warm-up decode; median of `repeats` windows; one process per step; dct_split: sg_profile events",
           "results": results}
    if "dct" in results and "dense" in results:
        out["dct_over_dense"] = results["dct"]["codewords_per_s"] / results["dense"]["codewords_per_s"]
    if failed:
        out["failed"] = failed
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
