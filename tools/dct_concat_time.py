#!/usr/bin/env python
"""Timing of the concatenated SPARC + LDPC decoder on the sub-sampled DCT design
(pipeline.DctConcatPipeline) against the dense Gaussian design
(pipeline.ConcatPipeline) at the C5 geometry: L=1024, M=512, 160 unprotected
sections + 4 x LDPC 802.11n r1/2 z=81, n=9216 and n=6144, single precision,
t_max 25, sumprod2 200 iterations, batches generated on the GPU.

Steps, each in a child process of its own under a time limit, in order; the
first step that fails or runs out of time ends the run (nothing further is
started on the GPU):

  dct_n9216, dense_n9216, dct_n6144, dense_n6144
        codewords/s of pipe.decode() on one device batch: host clock around
        `steps` decodes that end in a device synchronise, after a warm-up
        decode; median of `repeats` windows;
  llr_n9216
        sg_amp_decode_device alone against sg_amp_decode_device +
        sg_amp_llr_device over the protected sections on the same batch
        (alternating windows), and the mean AMP iterations of the batch: the
        LLR pass against one AMP iteration of the same batch.

The two pipelines decode different codes drawn from the same ensemble at the
same Eb/N0; their AMP differs as DctConcatPipeline's docstring says (early
stopping against fixed t_max), so the ratio is end to end, not kernel to
kernel.  Results go to profiles/dct_concat.json.  Needs a GPU.

    python tools/dct_concat_time.py [--batch 256] [--steps 4] [--repeats 5] [--ebn0 5.5]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

L, M, P, LU, MULTS = 1024, 512, 15.0, 160, 4
LDPC = ("802.11n", "1/2", 81)
T_MAX = 25
STEPS = ["dct_n9216", "dense_n9216", "dct_n6144", "dense_n6144", "llr_n9216"]
LIMIT_S = {"dct": 240, "dense": 420, "llr": 240}  # per child, its plan build and warm-up included


def _pipe(kind, n):
    from ldpc_sparc_amd.pipeline import ConcatPipeline, DctConcatPipeline
    make = DctConcatPipeline if kind in ("dct", "llr") else ConcatPipeline
    return make(L, M, n, P, LU, MULTS, ldpc=LDPC, design_seed=1234, precision="f32", t_max=T_MAX)


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
    _native.require_gpu()
    kind, n = step.split("_n")
    n = int(n)
    pipe = _pipe(kind, n)
    user_bits = LU * 9 + MULTS * pipe.c.K
    var = P / (2 * (user_bits / n) * 10 ** (a.ebn0 / 10))
    B = a.batch
    pipe.make_batch_device(B, var, 5000, 0)
    pipe.reset_counts()
    pipe.decode()  # warm-up: workspace, code objects
    cnt = pipe.counts()
    res = {"step": step, "n": n, "batch": B, "steps": a.steps, "repeats": a.repeats, "ebn0_db": a.ebn0,
           "awgn_var": var, "warmup_counts": [int(c) for c in cnt],
           "warmup_ber": float(cnt[1]) / (cnt[0] * user_bits)}
    if kind != "llr":
        pipe.reset_counts()
        t = _windows(pipe.decode, a.steps, a.repeats)
        res.update(window_seconds=t, codewords_per_s=B * a.steps / float(np.median(t)))
        return res
    lib = _native.lib()
    ld = MULTS * pipe.c.N
    d_tf = _native.DeviceBuffer(B * 4)

    def amp():
        _native.check(lib.sg_amp_decode_device(pipe.plan, pipe.d_y.ptr, B, None, var, T_MAX, pipe.rtol,
                                               pipe.phi_method, pipe.d_idx.ptr, d_tf.ptr, None, None, None))

    def amp_llr():
        amp()
        _native.check(lib.sg_amp_llr_device(pipe.plan, B, LU, L - LU, ld, 0, pipe.d_llr.ptr, None))

    amp_llr()
    ta, tl = [], []
    for _ in range(a.repeats):  # alternating windows of the two versions
        ta += _windows(amp, a.steps, 1)
        tl += _windows(amp_llr, a.steps, 1)
    _native.synchronize()
    tf = d_tf.download(np.zeros(B, np.int32))
    ma, ml = float(np.median(ta)) / a.steps, float(np.median(tl)) / a.steps
    its = float(tf.mean())
    res.update(engine=_native.amp_last_decode(pipe.plan), decode_window_seconds=ta, decode_llr_window_seconds=tl,
               decode_ms=1e3 * ma, decode_llr_ms=1e3 * ml, llr_ms=1e3 * (ml - ma), mean_amp_iterations=its,
               amp_iteration_ms=1e3 * ma / its, llr_over_amp_iteration=(ml - ma) / (ma / its),
               window_spread_ms=1e3 * float(np.max(ta) - np.min(ta)) / a.steps,
               llr_values_gathered=B * (L - LU) * M)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ebn0", type=float, default=5.5)
    ap.add_argument("--only", nargs="*", default=STEPS, choices=STEPS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dct_concat.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)      # child mode: one step, result to --json
    ap.add_argument("--json", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        with open(a.json, "w") as f:
            json.dump(run_step(a.step, a), f)
        return 0
    results, failed = {}, None
    for step in a.only:
        limit = LIMIT_S[step.split("_")[0]]
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "step.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--json", path, "--batch", str(a.batch),
                   "--steps", str(a.steps), "--repeats", str(a.repeats), "--ebn0", str(a.ebn0)]
            try:
                rc = subprocess.run(cmd, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:  # a fault, an abort or the time limit: start nothing more on the GPU
                failed = {"step": step, "exit_status": rc, "limit_s": limit}
                break
            with open(path) as f:
                results[step] = json.load(f)
        print(json.dumps({k: results[step][k] for k in results[step] if not k.endswith("window_seconds")}), flush=True)
    out = {"geometry": {"L": L, "M": M, "P": P, "L_unprotected": LU, "mults": MULTS, "ldpc": list(LDPC),
                        "t_max": T_MAX, "precision": "f32"},
           "what": "host clock around `steps` decodes of one device batch ending in a device synchronise, after a "
                   "warm-up decode; median of `repeats` windows; one process per step",
           "results": results}
    for n in (9216, 6144):
        if f"dct_n{n}" in results and f"dense_n{n}" in results:
            out[f"dct_over_dense_n{n}"] = results[f"dct_n{n}"]["codewords_per_s"] / results[f"dense_n{n}"]["codewords_per_s"]
    if failed:
        out["failed"] = failed
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
