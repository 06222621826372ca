#!/usr/bin/env python
"""Timing of the concatenated real K = 2 (BPSK) SPARC + LDPC decoder on the
sub-sampled DCT design (pipeline.DctBpskConcatPipeline): L = 1024, M = 512,
K = 2 (10 bits per section), n = 8192, 64 unprotected sections + 5 x LDPC
802.16 r1/2 z = 80 (N = 1920 = 192 sections each), t_max 25, sumprod2 200
iterations, batches of 256 generated on the GPU.

Steps, each in a child process of its own under a time limit, in order; the
first step that fails or runs out of time ends the run (nothing further is
started on the GPU):

  pipeline
        codewords/s of pipe.decode() on one device batch: host clock around
        `steps` decodes that end in a device synchronise, after a warm-up
        decode; median of `repeats` windows;
  llr   sg_amp_decode_bpsk_device alone against sg_amp_decode_bpsk_device +
        sg_amp_bpsk_llr_device over the protected sections on the same batch
        (alternating windows), and the mean AMP iterations of the batch: the
        LLR pass against one operator-loop iteration of the same batch;
  keep  sg_amp_decode_bpsk_device with sg_amp_bpsk_soft_output on against off
        on the same batch (alternating windows): what storing s costs an
        iteration.

Results go to profiles/bpsk_concat.json.  Needs a GPU.

    python tools/bpsk_concat_time.py [--batch 256] [--steps 4] [--repeats 5] [--ebn0 5.5] [--precision f32]
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

L, M, N, P, LU, MULTS = 1024, 512, 8192, 15.0, 64, 5
PER = 10  # log2 M + 1 bits per section
LDPC = ("802.16", "1/2", 80)
T_MAX = 25
STEPS = ["pipeline", "llr", "keep"]
LIMIT_S = 240  # per child, its plan build and warm-up included


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


def _alternate(f0, f1, steps, repeats):
    """Medians per call of two versions in alternating windows, and the windows."""
    t0, t1 = [], []
    for _ in range(repeats):
        t0 += _windows(f0, steps, 1)
        t1 += _windows(f1, steps, 1)
    return float(np.median(t0)) / steps, float(np.median(t1)) / steps, t0, t1


def run_step(step, a):
    from ldpc_sparc_amd import _native
    from ldpc_sparc_amd.pipeline import DctBpskConcatPipeline
    _native.require_gpu()
    pipe = DctBpskConcatPipeline(L, M, N, P, LU, MULTS, ldpc=LDPC, design_seed=1234, precision=a.precision,
                                 t_max=T_MAX)
    user_bits = LU * PER + MULTS * pipe.c.K
    var = P / (2 * (user_bits / N) * 10 ** (a.ebn0 / 10))
    B = a.batch
    pipe.make_batch_device(B, var, 5000, 0)
    pipe.reset_counts()
    pipe.decode()  # warm-up: workspace, code objects
    cnt = pipe.counts()
    res = {"step": step, "batch": B, "steps": a.steps, "repeats": a.repeats, "ebn0_db": a.ebn0, "awgn_var": var,
           "precision": a.precision, "warmup_counts": [int(c) for c in cnt],
           "warmup_ber": float(cnt[1]) / (cnt[0] * user_bits)}
    if step == "pipeline":
        pipe.reset_counts()
        t = _windows(pipe.decode, a.steps, a.repeats)
        res.update(window_seconds=t, codewords_per_s=B * a.steps / float(np.median(t)))
        return res
    lib = _native.lib()
    ld = MULTS * pipe.c.N
    d_tf = _native.DeviceBuffer(B * 4)

    def amp():
        _native.check(lib.sg_amp_decode_bpsk_device(pipe.plan, pipe.d_y.ptr, B, None, var, T_MAX, pipe.rtol,
                                                    pipe.phi_method, pipe.d_idx.ptr, d_tf.ptr, None, None, None))

    def mean_iterations():
        _native.synchronize()
        return float(d_tf.download(np.zeros(B, np.int32)).mean())

    if step == "llr":
        def amp_llr():
            amp()
            _native.check(lib.sg_amp_bpsk_llr_device(pipe.plan, B, LU, L - LU, ld, 0, pipe.d_llr.ptr, None))

        amp_llr()
        ma, ml, ta, tl = _alternate(amp, amp_llr, a.steps, a.repeats)
        its = mean_iterations()
        res.update(decode_window_seconds=ta, decode_llr_window_seconds=tl, decode_ms=1e3 * ma,
                   decode_llr_ms=1e3 * ml, llr_ms=1e3 * (ml - ma), mean_amp_iterations=its,
                   amp_iteration_ms=1e3 * ma / its, llr_over_amp_iteration=(ml - ma) / (ma / its),
                   window_spread_ms=1e3 * float(np.max(ta) - np.min(ta)) / a.steps,
                   llr_values_read=B * (L - LU) * M)
        return res

    def amp_off():
        _native.check(lib.sg_amp_bpsk_soft_output(pipe.plan, 0))
        amp()

    def amp_on():
        _native.check(lib.sg_amp_bpsk_soft_output(pipe.plan, 1))
        amp()

    amp_off()
    m0, m1, t0, t1 = _alternate(amp_off, amp_on, a.steps, a.repeats)
    its = mean_iterations()
    res.update(off_window_seconds=t0, on_window_seconds=t1, decode_off_ms=1e3 * m0, decode_on_ms=1e3 * m1,
               mean_amp_iterations=its, amp_iteration_off_ms=1e3 * m0 / its, amp_iteration_on_ms=1e3 * m1 / its,
               on_over_off=m1 / m0, window_spread_ms=1e3 * float(np.max(t0) - np.min(t0)) / a.steps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ebn0", type=float, default=5.5)
    ap.add_argument("--precision", default="f32", choices=["f32", "f64"])
    ap.add_argument("--only", nargs="*", default=STEPS, choices=STEPS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bpsk_concat.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)      # child mode: one step, result to --json
    ap.add_argument("--json", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        with open(a.json, "w") as f:
            json.dump(run_step(a.step, a), f)
        return 0
    results, failed = {}, None
    for step in a.only:
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "step.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--json", path, "--batch", str(a.batch),
                   "--steps", str(a.steps), "--repeats", str(a.repeats), "--ebn0", str(a.ebn0), "--precision",
                   a.precision]
            try:
                rc = subprocess.run(cmd, timeout=LIMIT_S).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:  # a fault, an abort or the time limit: start nothing more on the GPU
                failed = {"step": step, "exit_status": rc, "limit_s": LIMIT_S}
                break
            with open(path) as f:
                results[step] = json.load(f)
        print(json.dumps({k: results[step][k] for k in results[step] if not k.endswith("window_seconds")}), flush=True)
    out = {"geometry": {"L": L, "M": M, "K": 2, "n": N, "P": P, "L_unprotected": LU, "mults": MULTS,
                        "ldpc": list(LDPC), "t_max": T_MAX, "precision": a.precision},
           "what": "host clock around `steps` calls on one device batch ending in a device synchronise, after a "
                   "warm-up; median of `repeats` windows, the two versions of a comparison in alternating windows; "
                   "one process per step",
           "results": results}
    if failed:
        out["failed"] = failed
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
