#!/usr/bin/env python
"""Timing of the complex AMP engine at transform sizes above 2^16: the golden
cases cbig20 (L = 1024, M = 512, R = 2.4, one 2^20-point transform: the
headline geometry in complex form) and cbig18sc (the same L and M, spatially
coupled, eight 2^18-point transforms) of tests/csparc_large_cases.py, at
B = 64 and B = 256 codewords per decode call.

Per (case, B): codewords/s of the whole sg_camp_decode call (host clock
around a call that ends in a device synchronise, copies included; median of
--repeats calls after --warmup calls), mean t_final, and the device time of
every phase of one further call (sg_profile_enable: HIP events around each
launch, so that call is not among the timed ones).  Beside it the NumPy
restatement (tests/csparc_ref.py) on this host, one codeword at a time.
Writes profiles/csparc_large.json.  Needs a GPU.

    python tools/csparc_large_time.py [--cases cbig20,cbig18sc] [--batches 64,256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import csparc_ref  # noqa: E402
from csparc_large_cases import AWGN_VAR, CASES, K_of, base_matrix, code_params, ref_orders  # noqa: E402
from ldpc_sparc_amd import _native, sparc  # noqa: E402

SEED = [1, 2000]
REAL_F64_HEADLINE = 4.75e3  # README: the real f64 engine at the same (L, M) = (1024, 512), codewords/s


def run_case(name, batches, repeats, warmup, cpu_codewords):
    cp, W = base_matrix(code_params(CASES[name][1]))
    t_max = CASES[name][2]['t_max']
    L, M, K = cp['L'], cp['M'], K_of(cp)
    n = int(round(L * np.log2(K * M) / cp['R']))  # sparc_encode's n (sparc.py:33-41)
    if W.ndim == 2:
        n = int(round(n / W.shape[0])) * W.shape[0]
    Ab, Az = sparc.sparc_transforms(W, L, M, n, SEED, True)
    op = sparc.operator_of(Ab, Az)
    lib = _native.lib()
    constel = sparc._interleaved(sparc.psk_constel(K)) if K != 1 else None
    out = {"case": name, "code_params": CASES[name][1], "t_max": t_max, "awgn_var": AWGN_VAR, "n": n, "w": int(op.w),
           "transforms": int(op.order0.shape[0]), "runs": []}
    rng = np.random.default_rng(7)
    TI = TS = Y = mi = ms = tf = None
    for B in batches:
        TI = rng.integers(0, M, (B, L)).astype(np.int32)
        TS = rng.integers(0, K, (B, L)).astype(np.int32)
        d_idx = _native.DeviceBuffer.from_array(TI)
        d_sym = _native.DeviceBuffer.from_array(TS)
        d_x = _native.DeviceBuffer(B * n * 16)
        _native.check(lib.sg_camp_encode_device(op.plan(), K, _native.ptr(constel), d_idx.ptr,
                                                d_sym.ptr if K != 1 else None, B, d_x.ptr, None))
        _native.synchronize()
        X = d_x.download(np.zeros((B, n), dtype=np.complex128))
        Y = X + np.sqrt(AWGN_VAR / 2) * (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n)))

        def decode():
            return sparc.camp_decode_batch(Y, op, AWGN_VAR, t_max, 1e-6, 1, K, TI, TS)
        for _ in range(warmup):
            mi, ms, tf, _, _ = decode()
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            decode()
            times.append(time.perf_counter() - t0)
        prof = _native.Profiler(1)
        decode()
        phases = prof.stop()
        run = {
            "batch": B, "gpu_call_seconds": times,
            "gpu_codewords_per_s": B / float(np.median(times)),
            "mean_t_final": float(np.mean(tf)),
            "section_error_rate": float(np.mean((mi != TI) | (ms != TS))),
            "phase_ms": {k: v[0] for k, v in phases.items()}, "phase_launches": {k: v[1] for k, v in phases.items()},
        }
        out["runs"].append(run)
        print(name, json.dumps({k: run[k] for k in ("batch", "gpu_codewords_per_s", "mean_t_final",
                                                     "section_error_rate", "phase_ms")}), flush=True)
    # NumPy restatement on this host, the first codewords of the last batch
    o0, o1 = ref_orders(op, W)
    rAb, rAz = csparc_ref.fft_operators(W, L, M, n, o0, o1)
    nc = min(cpu_codewords, len(Y))
    same = True
    t0 = time.perf_counter()
    for b in range(nc):
        beta0 = sparc._msg_vector_from_indices(TI[b], TS[b], M, K)
        ri, rs, rt, _, _ = csparc_ref.amp(Y[b], W, L, M, n, K, rAb, rAz, AWGN_VAR, t_max, 1e-6, 1, beta0)
        same &= bool(np.array_equal(ri, mi[b]) and np.array_equal(rs, ms[b]) and rt == tf[b])
    out.update({"numpy_codewords": nc, "numpy_codewords_per_s": nc / (time.perf_counter() - t0),
                "numpy_decisions_equal": same})
    print(name, "numpy codewords/s", out["numpy_codewords_per_s"], "decisions equal", same, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="cbig20,cbig18sc")
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-codewords", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "csparc_large.json"))
    a = ap.parse_args()
    _native.require_gpu()
    batches = [int(b) for b in a.batches.split(",")]
    res = {
        "split": "asymmetric: P = 256, Q = w / 256, pass B in tiles of 4096 values (512 threads, 64 KB of LDS)",
        "what": "whole sg_camp_decode call (host clock, copies included, ends in a device synchronise), median of "
                "%d calls after %d warm-up calls; phase_ms: device time per phase of one further call; NumPy "
                "restatement tests/csparc_ref.py on the same host, single process" % (a.repeats, a.warmup),
        "context_real_f64_codewords_per_s_same_L_M": REAL_F64_HEADLINE,
        "cases": [run_case(name, batches, a.repeats, a.warmup, a.cpu_codewords) for name in a.cases.split(",")],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("for context: the real f64 engine at the same (L, M):", REAL_F64_HEADLINE, "codewords/s (README)")


if __name__ == "__main__":
    main()
