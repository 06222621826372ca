#!/usr/bin/env python
"""Timing of a Monte-Carlo block of the complex engine on the reference
notebook's geometry (complex 4-PSK, L=2048, M=8, R=2.6, w = 2^15, t_max 25,
B=256 codewords per block), two ways in one run:

  device-resident  montecarlo.CSparcTrial end to end: Philox bits, sections,
                   x = A beta0, noise, AMP and the error counters on the GPU,
                   one download of the counters;
  host-fed         what the package offered before the campaign path: NumPy
                   section draws -> message vectors -> op.Ab -> NumPy noise ->
                   sparc.camp_decode_batch -> calc_ler_ver / calc_ber per
                   codeword on the host.

Host clock around each whole block (both end in a synchronising download),
warm-up first, then several timed repeats; medians, and their ratio, go to
profiles/csparc_campaign.json.  The decode-only figure of
profiles/csparc_cnb.json (tools/csparc_time.py) is the ceiling of both.  Needs
a GPU.

    python tools/csparc_campaign_time.py [--batch 256] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from ldpc_sparc_amd import _native, montecarlo, sparc, sparc_sim  # noqa: E402

CODE = {'P': 15.0, 'R': 2.6, 'L': 2048, 'M': 8, 'complex': True, 'modulated': True, 'K': 4}
T_MAX, AWGN_VAR, SEED = 25, 1.0, [1, 2000]


def host_fed_block(op, K, B, blk):
    """One block through host arrays; returns CSparcTrial's seven counters."""
    L, M, n = op.L, op.M, op.n
    rng = np.random.RandomState([blk, 11])
    ti, ts = rng.randint(0, M, (B, L)), rng.randint(0, K, (B, L))
    beta0 = np.stack([sparc._msg_vector_from_indices(ti[b], ts[b], M, K) for b in range(B)])
    X = op.Ab(beta0)
    Y = X + np.sqrt(AWGN_VAR / 2) * (rng.randn(B, n) + 1j * rng.randn(B, n))
    mi, ms, tf, _, _ = sparc.camp_decode_batch(Y, op, AWGN_VAR, T_MAX, 1e-6, 1, K, ti, ts)
    cnt = np.zeros(7, dtype=np.int64)
    for b in range(B):
        beta = sparc._msg_vector_from_indices(mi[b], ms[b], M, K)
        _, _, (nloc, nval, nsec) = sparc_sim.calc_ler_ver(beta0[b], beta, L, K)
        bits0, bits1 = sparc.msg_vector_2_bin_arr(beta0[b], M, K), sparc.msg_vector_2_bin_arr(beta, M, K)
        nbit = int(round(sparc_sim.calc_ber(bits0, bits1) * bits0.size))
        cnt += np.array([1, nbit, nbit > 0, tf[b], nsec, nloc, nval], dtype=np.int64)
    return cnt


def timed(fn, repeats):
    fn(-2), fn(-1)  # warm-up (plan, workspace, code objects)
    out, times = [], []
    for r in range(repeats):
        t0 = time.perf_counter()
        out.append(fn(r))
        times.append(time.perf_counter() - t0)
    return np.sum(out, axis=0), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "csparc_campaign.json"))
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
    B = a.batch
    trial = montecarlo.CSparcTrial(op, K, [AWGN_VAR], T_MAX, 1e-6, 1, seed=5)
    dev_cnt, dev_t = timed(lambda r: trial(0, r + 2, 1, B), a.repeats)
    host_cnt, host_t = timed(lambda r: host_fed_block(op, K, B, r + 2), a.repeats)
    dev_rate, host_rate = B / float(np.median(dev_t)), B / float(np.median(host_t))
    res = {
        "case": "cnb", "code_params": CODE, "t_max": T_MAX, "awgn_var": AWGN_VAR, "n": n, "w": int(op.w),
        "batch": B, "repeats": a.repeats,
        "device_block_seconds": dev_t, "host_fed_block_seconds": host_t,
        "device_codewords_per_s": dev_rate, "host_fed_codewords_per_s": host_rate,
        "device_over_host_fed": dev_rate / host_rate,
        "device_counts": [int(c) for c in dev_cnt], "host_fed_counts": [int(c) for c in host_cnt],
        "counters": ["codewords", "bit errors", "codeword errors", "AMP iterations", "section errors",
                     "location errors", "value errors"],
        "what": "host clock around one whole Monte-Carlo block of `batch` codewords, generation to counters, "
                "median of the repeats after two warm-up blocks; device: montecarlo.CSparcTrial; host-fed: NumPy "
                "draws -> op.Ab -> NumPy noise -> camp_decode_batch -> calc_ler_ver / calc_ber per codeword "
                "(different random draws, same design and noise level)",
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("device_codewords_per_s", "host_fed_codewords_per_s", "device_over_host_fed",
                                          "device_counts", "host_fed_counts")}))


if __name__ == "__main__":
    main()
