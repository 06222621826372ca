#!/usr/bin/env python
"""Timing of the three-stage concatenated K-PSK decoder AMP -> BP -> AMP
(pipeline.CsparcConcat3Pipeline) against the two-stage one
(pipeline.CsparcConcatPipeline) on the complex sub-sampled FFT design at the
sections and blocks of tools/csparc_concat_time.py: L=1024, M=512, K=4 (11
bits per section), 64 unprotected sections + 5 x LDPC 802.16 r1/2 z=88, double
precision, t_max 25, sumprod2 200 iterations, B = 256, the batch generated on
the GPU; at n=8192 complex channel uses and Eb/N0 4 dB, where BP stops on its
syndrome and the first AMP leaves unprotected sections wrong (at that tool's
n=4096 neither decoder recovers a codeword up to 10 dB, and the final pass is a
second full AMP decode: 0.48 of the batch time).

One pipeline object holds the plan, the graph and the batch; the two-stage
decoder is that object's AMP, soft-output, BP and counting stages without its
final pass, so both decode the same received words through the same plan.  Host clock around `steps` decodes that
end in a device synchronise, after a warm-up decode of each; windows of the two
decoders alternate, `repeats` of each, medians reported.  The final pass's
share of the time is (three - two) / three of the medians per decode: what the
known-sections and unpack kernels, the second AMP and its packing add.  The error counters of both
decoders on the batch are reported beside the times.

The measurement runs in a child process under a time limit; a fault, an abort
or the limit ends the run.  Results go to profiles/csparc_concat3.json.  Needs a
GPU.

    python tools/csparc_concat3_time.py [--batch 256] [--steps 2] [--repeats 5] [--ebn0 4.0] [--n 8192]
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

L, M, K, N, P, LU, MULTS = 1024, 512, 4, 8192, 15.0, 64, 5
LDPC = ("802.16", "1/2", 88)
T_MAX = 25
LIMIT_S = 420  # the child: plan build, warm-up and the windows


def _window(fn, steps):
    from ldpc_sparc_amd import _native
    _native.device_synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    _native.device_synchronize()
    return time.perf_counter() - t0


def measure(a):
    from ldpc_sparc_amd import _native
    from ldpc_sparc_amd.pipeline import CsparcConcat3Pipeline
    _native.require_gpu()
    N = a.n
    pipe = CsparcConcat3Pipeline(L, M, K, N, P, LU, MULTS, ldpc=LDPC, design_seed=1234, t_max=T_MAX,
                                 final_t_max=a.final_t_max)
    user_bits = LU * pipe.bits_per_section + MULTS * pipe.c.K
    var = P / ((user_bits / N) * 10 ** (a.ebn0 / 10))  # complex noise: N0 = awgn_var
    B = a.batch
    pipe.make_batch_device(B, var, 5000, 0)
    def two_stage():  # decode()'s stages without the final pass (CsparcConcatPipeline.decode(pipe) would run pipe's)
        pipe._amp()
        pipe._soft_output()
        pipe._bp()
        pipe._count()

    decoders = {"two_stage": two_stage, "three_stage": pipe.decode}
    res = {"n": N, "batch": B, "steps": a.steps, "repeats": a.repeats, "ebn0_db": a.ebn0, "awgn_var": var,
           "final_t_max": pipe.final_t_max}
    for name, fn in decoders.items():  # warm-up: workspaces, code objects; and the counters of the batch
        pipe.reset_counts()
        fn()
        cnt = pipe.counts()
        res[name] = {"counts": [int(c) for c in cnt], "ber": float(cnt[1]) / (cnt[0] * user_bits),
                     "unprotected_bit_errors": int(cnt[3]), "protected_bit_errors": int(cnt[4])}
    t = {name: [] for name in decoders}
    for _ in range(a.repeats):  # alternating windows
        for name, fn in decoders.items():
            t[name].append(_window(fn, a.steps))
    for name in decoders:
        med = float(np.median(t[name]))
        res[name].update(window_seconds=t[name], decode_ms=1e3 * med / a.steps, codewords_per_s=B * a.steps / med,
                         window_spread_ms=1e3 * float(np.max(t[name]) - np.min(t[name])) / a.steps)
    two, three = res["two_stage"]["decode_ms"], res["three_stage"]["decode_ms"]
    res.update(final_pass_ms=three - two, final_pass_share=(three - two) / three,
               three_over_two_codewords_per_s=res["three_stage"]["codewords_per_s"] / res["two_stage"]["codewords_per_s"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ebn0", type=float, default=4.0)
    ap.add_argument("--n", type=int, default=N, help="complex channel uses")
    ap.add_argument("--final-t-max", type=int, default=None, dest="final_t_max")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "csparc_concat3.json"))
    ap.add_argument("--json", help=argparse.SUPPRESS)  # child mode: measure, result to this file
    a = ap.parse_args()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(measure(a), f)
        return 0
    out = {"geometry": {"L": L, "M": M, "K": K, "n": a.n, "P": P, "L_unprotected": LU, "mults": MULTS,
                        "ldpc": list(LDPC), "t_max": T_MAX, "precision": "f64"},
           "what": "host clock around `steps` decodes of one device batch ending in a device synchronise, after a "
                   "warm-up decode of each decoder; alternating windows, median of `repeats`; both decoders on the "
                   "same pipeline object, plan and batch"}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "result.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--json", path, "--batch", str(a.batch), "--steps",
               str(a.steps), "--repeats", str(a.repeats), "--ebn0", str(a.ebn0), "--n", str(a.n)]
        if a.final_t_max is not None:
            cmd += ["--final-t-max", str(a.final_t_max)]
        try:
            rc = subprocess.run(cmd, timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc == 0:
            with open(path) as f:
                out["result"] = json.load(f)
            print(json.dumps({k: v for k, v in out["result"].items() if not isinstance(v, dict)}), flush=True)
            for name in ("two_stage", "three_stage"):
                r = out["result"][name]
                print(name, json.dumps({k: r[k] for k in r if k != "window_seconds"}), flush=True)
        else:  # a fault, an abort or the time limit
            out["failed"] = {"exit_status": rc, "limit_s": LIMIT_S}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if "result" in out else 1


if __name__ == "__main__":
    sys.exit(main())
