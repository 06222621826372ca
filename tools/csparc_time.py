#!/usr/bin/env python
"""Baseline timing of the complex AMP engine on the reference notebook's
geometry: complex 4-PSK, L=2048, M=8, R=2.6 (w = 2^15), t_max 25, B=256
codewords per decode call.

Prints codewords/s of the GPU engine (warm-up, then several timed repeats of
the whole call: host clock around a call that ends in a device synchronise,
copies included) and of the NumPy restatement (tests/csparc_ref.py) on this
host, and writes both to profiles/csparc_cnb.json.  Needs a GPU.

    python tools/csparc_time.py [--batch 256] [--repeats 5] [--cpu-codewords 4]
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
from ldpc_sparc_amd import _native, sparc  # noqa: E402

CODE = {'P': 15.0, 'R': 2.6, 'L': 2048, 'M': 8, 'complex': True, 'modulated': True, 'K': 4}
T_MAX, AWGN_VAR, SEED = 25, 1.0, [1, 2000]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-codewords", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "csparc_cnb.json"))
    a = ap.parse_args()
    _native.require_gpu()
    cp = dict(CODE)
    sparc.check_code_params(cp)
    L, M, K = cp['L'], cp['M'], cp['K']
    bit_len = int(round(L * np.log2(K * M)))
    n = int(round(bit_len / cp['R']))
    W = sparc.create_base_matrix(awgn_var=AWGN_VAR, **cp)
    Ab, Az = sparc.sparc_transforms(W, L, M, n, SEED, True)
    op = sparc.operator_of(Ab, Az)
    rng = np.random.RandomState(7)
    B = a.batch
    beta0 = np.stack([sparc.rnd_msg_vector(L, M, [b, 11], K) for b in range(B)])
    X = op.apply(beta0, False)
    Y = X + np.sqrt(AWGN_VAR / 2) * (rng.randn(B, n) + 1j * rng.randn(B, n))
    idx = [sparc._msg_vector_indices(beta0[b], M, K) for b in range(B)]
    TI, TS = np.stack([i[0] for i in idx]), np.stack([i[1] for i in idx])

    def decode():
        return sparc.camp_decode_batch(Y, op, AWGN_VAR, T_MAX, 1e-6, 1, K, TI, TS)
    mi, ms, tf, nmse, psi = decode()  # warm-up (plan, workspace, code objects)
    decode()
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        decode()
        times.append(time.perf_counter() - t0)
    ser = float(np.mean((mi != TI) | (ms != TS)))
    # NumPy restatement on this host, one codeword at a time
    o0, o1 = op.order0[0], op.order1[0]
    rAb, rAz = csparc_ref.fft_operators(W, L, M, n, o0, o1)
    nc = min(a.cpu_codewords, B)
    same = True
    t0 = time.perf_counter()
    for b in range(nc):
        ri, rs, rt, _, _ = csparc_ref.amp(Y[b], W, L, M, n, K, rAb, rAz, AWGN_VAR, T_MAX, 1e-6, 1, beta0[b])
        same &= bool(np.array_equal(ri, mi[b]) and np.array_equal(rs, ms[b]) and rt == tf[b])
    cpu_s = time.perf_counter() - t0
    res = {
        "case": "cnb", "code_params": CODE, "t_max": T_MAX, "awgn_var": AWGN_VAR, "n": n, "w": int(op.w),
        "batch": B, "repeats": a.repeats,
        "gpu_call_seconds": times,
        "gpu_codewords_per_s": B / float(np.median(times)),
        "gpu_codewords_per_s_best": B / float(np.min(times)),
        "mean_t_final": float(np.mean(tf)), "section_error_rate": ser,
        "numpy_codewords": nc, "numpy_codewords_per_s": nc / cpu_s,
        "numpy_decisions_equal": same,
        "what": "whole sg_camp_decode call (host clock, copies included, ends in a device synchronise); "
                "NumPy restatement tests/csparc_ref.py on the same host, single process",
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("gpu_codewords_per_s", "gpu_codewords_per_s_best", "numpy_codewords_per_s",
                                          "mean_t_final", "section_error_rate", "numpy_decisions_equal")}))


if __name__ == "__main__":
    main()
