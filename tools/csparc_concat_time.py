#!/usr/bin/env python
"""Timing of the concatenated K-PSK SPARC + LDPC decoder on the complex FFT
design (pipeline.CsparcConcatPipeline): L = 1024, M = 512, K = 4 (11 bits per
section), 64 unprotected sections + 5 x LDPC 802.16 r1/2 z = 88 (N = 2112 =
192 sections each), n = 4096 complex channel uses, double precision, t_max 25,
sumprod2 200 iterations, B = 256, batches generated on the GPU.

  decode   codewords/s of pipe.decode() on one device batch: host clock around
           `steps` decodes that end in a device synchronise, after a warm-up
           decode; median of `repeats` windows;
  llr      sg_camp_decode_device alone against sg_camp_decode_device +
           sg_camp_llr_device over the protected sections on the same batch
           (alternating windows), and the mean AMP iterations of the batch: the
           share of the LLR pass against one AMP iteration.

Results go to profiles/csparc_concat.json.  Needs a GPU.

    python tools/csparc_concat_time.py [--batch 256] [--steps 2] [--repeats 5] [--ebn0 6.0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

L, M, K, N_CH, P, LU, MULTS = 1024, 512, 4, 4096, 15.0, 64, 5
LDPC = ("802.16", "1/2", 88)
T_MAX = 25


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ebn0", type=float, default=6.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "csparc_concat.json"))
    a = ap.parse_args()
    from ldpc_sparc_amd import _native
    from ldpc_sparc_amd.pipeline import CsparcConcatPipeline
    _native.require_gpu()
    pipe = CsparcConcatPipeline(L, M, K, N_CH, P, LU, MULTS, ldpc=LDPC, design_seed=1234, t_max=T_MAX)
    per = pipe.bits_per_section
    user_bits = LU * per + MULTS * pipe.c.K
    var = P / ((user_bits / N_CH) * 10 ** (a.ebn0 / 10))  # complex noise: N0 = awgn_var
    B, lib = a.batch, _native.lib()
    pipe.make_batch_device(B, var, 5000, 0)
    pipe.reset_counts()
    pipe.decode()  # warm-up: workspace, code objects
    cnt = pipe.counts()
    dec = _windows(pipe.decode, a.steps, a.repeats)
    cs = _native.ptr(pipe.constel)
    d_tf = _native.DeviceBuffer(B * 4)

    def amp():
        _native.check(lib.sg_camp_decode_device(pipe.plan, pipe.d_y.ptr, B, K, cs, None, None, var, T_MAX, pipe.rtol,
                                                pipe.phi_method, pipe.d_midx.ptr, pipe.d_msym.ptr, d_tf.ptr, None,
                                                None, None))

    def amp_llr():
        amp()
        _native.check(lib.sg_camp_llr_device(pipe.plan, B, K, cs, LU, L - LU, MULTS * pipe.c.N, 0, pipe.d_llr.ptr,
                                             None))

    t_amp, t_both = [], []
    for _ in range(a.repeats):
        t_amp += _windows(amp, a.steps, 1)
        t_both += _windows(amp_llr, a.steps, 1)
    its = float(d_tf.download(np.zeros(B, np.int32)).mean())
    amp_s, both_s = float(np.median(t_amp)) / a.steps, float(np.median(t_both)) / a.steps
    llr_s = both_s - amp_s
    res = {"geometry": {"L": L, "M": M, "K": K, "n": N_CH, "P": P, "L_unprotected": LU, "mults": MULTS,
                        "ldpc": list(LDPC), "bits_per_section": per, "user_bits": user_bits, "B": B,
                        "precision": "f64", "t_max": T_MAX, "ebn0_db": a.ebn0, "awgn_var": var},
           "warmup_counts": [int(c) for c in cnt],
           "decode": {"codewords_per_s": B * a.steps / float(np.median(dec)), "windows_s": dec},
           "llr": {"amp_s": amp_s, "amp_plus_llr_s": both_s, "llr_s": llr_s, "mean_amp_iterations": its,
                   "llr_over_one_amp_iteration": llr_s / (amp_s / its) if its else None}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["decode"]), json.dumps(res["llr"]))


if __name__ == "__main__":
    main()
