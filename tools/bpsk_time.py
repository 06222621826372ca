#!/usr/bin/env python
"""Time per AMP iteration of the real K = 2 (BPSK) modulated decode
(sg_amp_decode_bpsk_device, csrc/amp_oploop.hip) against
sg_amp_decode_partial_device with no section known on the same plan and
batch: L = 1024, M = 512, n = 6144 (R = 1.5 in unmodulated terms), flat design,
B = 256, both precisions.

The two loops enqueue the identical operator launches (Ab, Az of the plan on
natural-order vectors) and differ in the kernels between them, so the
difference of the two figures is the cost of the K = 2 kernels.  Neither uses a
throughput engine: this is the staged path.

Each loop decodes codewords of its own family (K = 2 words, unmodulated
indices) at awgn_var = 1 with t_max = 7 and rtol = 1e-12: the first six
iterations of a decode, in which psi still moves in every codeword, so that
none stops and every decode runs its t_max - 1 = 6 iterations.  The t_final
range of each loop is recorded, and `all_iterations_ran` says whether that
held.

One child process per precision under a time limit; the first that fails ends
the run.  Per precision: a warm-up decode of each loop, then `repeats`
alternating windows of `steps` decodes, host clock around work that ends in a
device synchronise; the median window and the spread (max - min) per
iteration go to profiles/bpsk_amp.json.  Needs a GPU.

    python tools/bpsk_time.py [--batch 256] [--steps 12] [--repeats 7]
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

L, M, N, P = 1024, 512, 6144, 15.0
T_MAX, RTOL, VAR, DESIGN_SEED = 7, 1e-12, 1.0, 1234
LIMIT_S = 300


def run_precision(precision, a):
    from ldpc_sparc_amd import _native, sparc
    _native.require_gpu()
    lib = _native.lib()
    prec = _native.SG_F64 if precision == "f64" else _native.SG_F32
    dt = np.float64 if precision == "f64" else np.float32
    B = a.batch
    W = np.array(P)
    o0, o1 = sparc.generate_ordering(W, N, L * M, DESIGN_SEED)
    op = sparc.DesignOperator(W, L, M, N, o0, o1)
    plan = op.plan(prec)
    rng = np.random.RandomState(7)
    d_word = _native.DeviceBuffer.from_array(rng.randint(0, 2 * M, (B, L)).astype(np.int32))
    d_known = _native.DeviceBuffer.from_array(np.full((B, L), -1, np.int32))
    d_idx = _native.DeviceBuffer.from_array(rng.randint(0, M, (B, L)).astype(np.int32))
    d_x = _native.DeviceBuffer(B * N * dt().itemsize)
    noise = np.sqrt(VAR) * rng.randn(B, N)
    d_y = {}
    for name, enc, d_sec in (("bpsk", lib.sg_amp_encode_bpsk_device, d_word),
                             ("partial", lib.sg_amp_encode_device, d_idx)):
        _native.check(enc(plan, d_sec.ptr, B, d_x.ptr, None))
        _native.synchronize()
        d_y[name] = _native.DeviceBuffer.from_array((d_x.download(np.empty((B, N), dt)) + noise).astype(dt))
    d_map = _native.DeviceBuffer(B * L * 4)
    d_tf = _native.DeviceBuffer(B * 4)

    def bpsk():
        _native.check(lib.sg_amp_decode_bpsk_device(plan, d_y["bpsk"].ptr, B, None, VAR, T_MAX, RTOL, 1, d_map.ptr,
                                                    d_tf.ptr, None, None, None))

    def partial():
        _native.check(lib.sg_amp_decode_partial_device(plan, d_y["partial"].ptr, B, d_known.ptr, None, VAR, T_MAX, RTOL,
                                                       1, d_map.ptr, d_tf.ptr, None, None, None))

    def window(fn):
        _native.device_synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        _native.device_synchronize()
        return time.perf_counter() - t0

    res = {"precision": precision, "batch": B, "steps": a.steps, "repeats": a.repeats}
    tfs = {}
    for name, fn in (("bpsk", bpsk), ("partial", partial)):  # warm-up: workspace, code objects
        fn()
        _native.device_synchronize()
        tf = d_tf.download(np.zeros(B, np.int32))
        tfs[name] = tf
        res[name + "_t_final_min_max"] = [int(tf.min()), int(tf.max())]
    tb, tp = [], []
    for _ in range(a.repeats):  # alternating windows of the two loops
        tb.append(window(bpsk))
        tp.append(window(partial))
    its = T_MAX - 1
    res["all_iterations_ran"] = bool(all(tf.min() == its for tf in tfs.values()))
    per = lambda t: 1e3 * float(t) / (a.steps * its)  # noqa: E731
    res.update(bpsk_window_seconds=tb, partial_window_seconds=tp, iterations_per_decode=its,
               bpsk_ms_per_iteration=per(np.median(tb)), partial_ms_per_iteration=per(np.median(tp)),
               bpsk_spread_ms_per_iteration=per(np.max(tb) - np.min(tb)),
               partial_spread_ms_per_iteration=per(np.max(tp) - np.min(tp)))
    res["bpsk_over_partial"] = res["bpsk_ms_per_iteration"] / res["partial_ms_per_iteration"]
    res["bpsk_kernels_extra_ms_per_iteration"] = res["bpsk_ms_per_iteration"] - res["partial_ms_per_iteration"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", nargs="*", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bpsk_amp.json"))
    ap.add_argument("--precision", help=argparse.SUPPRESS)  # child mode: one precision, result to --json
    ap.add_argument("--json", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.precision:
        with open(a.json, "w") as f:
            json.dump(run_precision(a.precision, a), f)
        return 0
    results, failed = {}, None
    for precision in a.only:
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "res.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--precision", precision, "--json", path, "--batch",
                   str(a.batch), "--steps", str(a.steps), "--repeats", str(a.repeats)]
            try:
                rc = subprocess.run(cmd, timeout=LIMIT_S).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:  # a fault, an abort or the time limit: start nothing more on the GPU
                failed = {"precision": precision, "exit_status": rc, "limit_s": LIMIT_S}
                break
            with open(path) as f:
                results[precision] = json.load(f)
        print(json.dumps({k: v for k, v in results[precision].items() if not k.endswith("window_seconds")}), flush=True)
    out = {"geometry": {"L": L, "M": M, "n": N, "P": P, "design": "flat", "t_max": T_MAX, "rtol": RTOL,
                        "awgn_var": VAR},
           "what": "ms per AMP iteration of sg_amp_decode_bpsk_device and of sg_amp_decode_partial_device with no "
                   "section known, same plan and batch size; host clock around `steps` decodes ending in a device "
                   "synchronise, after a warm-up decode of each; median of `repeats` alternating windows, spread = "
                   "max - min window; one process per precision",
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
