#!/usr/bin/env python
"""Timing of the layered BP schedule (bp_layered.hip) against flooding at the
C3 geometry: 802.11n r1/2 z = 81 (n = 1944), B = 4096 random codewords,
single-precision min-sum (factor 0.7), Eb/N0 1.0 / 1.5 / 2.0 dB; information
bits, encoding and noise on the GPU (Philox streams, as the campaigns draw
them).  On the same channel LLRs:

  flooding_50   sg_ldpc_decode_device, max_it = 50 (the C3 decode)
  layered_25    sg_ldpc_decode_layered_device, layer = z, max_it = 25
  layered_50    the same at max_it = 50

each with codewords/s (host clock around `steps` decodes that end in a device
synchronise, after a warm-up decode; median of `repeats` windows), the mean
number of executed iterations and the frame errors over all n bits.

One child process per Eb/N0 under a time limit, in order; the first that
fails or runs out of time ends the run (nothing further is started on the
GPU).  Results go to profiles/bp_layered.json with the library's hash.  Needs
a GPU.

    python tools/bp_layered_time.py [--batch 4096] [--steps 20] [--repeats 5]
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

LDPC = ("802.11n", "1/2", 81)
EBN0 = [1.0, 1.5, 2.0]
CORR, SEED = 0.7, 2000
LIMIT_S = 180  # per child, its graph upload and warm-up included
DECODES = [("flooding_50", "flooding", 50), ("layered_25", "layered", 25), ("layered_50", "layered", 50)]


def run_point(ebn0, a):
    from ldpc_sparc_amd import _native
    from ldpc_sparc_amd.ldpc import code
    _native.require_gpu()
    lib, c, B = _native.lib(), code(*LDPC), a.batch
    g = c._device_graph()
    sigma2 = 1 / (2 * (c.K / c.N) * 10 ** (ebn0 / 10))
    sid = int(round(ebn0 * 100))
    d_info, d_x = _native.DeviceBuffer(B * c.K), _native.DeviceBuffer(B * c.N)
    d_ch, d_app, d_it = _native.DeviceBuffer(B * c.N * 4), _native.DeviceBuffer(B * c.N * 4), _native.DeviceBuffer(B * 4)
    d_cnt = _native.DeviceBuffer(32)
    _native.check(lib.sg_rng_bits_device(SEED, sid, B, c.K, d_info.ptr, None))
    c.encode_device(d_info.ptr, B, d_x.ptr)
    _native.check(lib.sg_bpsk_awgn_llr_device(_native.SG_F32, SEED, sid, d_x.ptr, B, c.N, sigma2, d_ch.ptr, None))
    res = {"ebn0_db": ebn0, "batch": B, "steps": a.steps, "repeats": a.repeats}
    for name, schedule, max_it in DECODES:
        def decode():
            if schedule == "layered":
                _native.check(lib.sg_ldpc_decode_layered_device(g, _native.SG_MINSUM, _native.SG_F32, c.z, d_ch.ptr, B,
                                                                max_it, CORR, d_app.ptr, d_it.ptr, None))
            else:
                _native.check(lib.sg_ldpc_decode_device(g, _native.SG_MINSUM, _native.SG_F32, d_ch.ptr, B, max_it, CORR,
                                                        d_app.ptr, d_it.ptr, None))
        decode()  # warm-up: code object, layer tables
        _native.device_synchronize()
        windows = []
        for _ in range(a.repeats):
            _native.device_synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                decode()
            _native.device_synchronize()
            windows.append(time.perf_counter() - t0)
        d_cnt.zero()
        _native.check(lib.sg_ldpc_count_errors_device(g, _native.SG_F32, d_app.ptr, d_x.ptr, d_it.ptr, B, c.K,
                                                      d_cnt.ptr, None))
        _native.synchronize()
        cnt = d_cnt.download(np.zeros(4, np.int64))
        its = d_it.download(np.zeros(B, np.int32))
        res[name] = {"kernel": c.decode_kernel("minsum", _native.SG_F32, schedule=schedule), "max_it": max_it,
                     "codewords_per_s": B * a.steps / float(np.median(windows)), "window_seconds": windows,
                     "mean_executed_iterations": float(np.where(its < max_it, its + 1, max_it).mean()),
                     "frame_errors": int(cnt[1]), "bit_errors": int(cnt[0])}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bp_layered.json"))
    ap.add_argument("--point", type=float, help=argparse.SUPPRESS)  # child mode: one Eb/N0, result to --json
    ap.add_argument("--json", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.point is not None:
        with open(a.json, "w") as f:
            json.dump(run_point(a.point, a), f)
        return 0
    from ldpc_sparc_amd import _native
    with open(_native.LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    results, failed = [], None
    for ebn0 in EBN0:
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "point.json")
            cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--point", str(ebn0),
                   "--json", path, "--batch", str(a.batch), "--steps", str(a.steps), "--repeats", str(a.repeats)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:  # a fault, an abort or the time limit: start nothing more on the GPU
                failed = {"ebn0_db": ebn0, "exit_status": rc, "limit_s": LIMIT_S}
                break
            with open(path) as f:
                results.append(json.load(f))
        print(json.dumps({k: ({q: w for q, w in v.items() if q != "window_seconds"} if isinstance(v, dict) else v)
                          for k, v in results[-1].items()}), flush=True)
    out = {"geometry": {"ldpc": list(LDPC), "dectype": "minsum", "corr": CORR, "precision": "f32", "layer": LDPC[2],
                        "inputs": "random codewords, BPSK/AWGN, Philox on the GPU (seed %d, stream 100 Eb/N0)" % SEED},
           "lib_sha256": lib_hash,
           "what": "host clock around `steps` decodes of one device batch ending in a device synchronise, after a "
                   "warm-up decode; median of `repeats` windows; one process per Eb/N0; executed iterations = it + 1 "
                   "where the codeword stopped, else max_it; frame errors over all n bits",
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
