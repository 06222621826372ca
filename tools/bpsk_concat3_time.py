#!/usr/bin/env python
"""Timing of the three-stage concatenated decoder AMP -> BP -> AMP on a real
K = 2 SPARC (pipeline.DctBpskConcat3Pipeline) against the two-stage one
(pipeline.DctBpskConcatPipeline) at the geometry of tools/bpsk_concat_time.py:
L = 1024, M = 512, K = 2 (10 bits per section), n = 8192, 64 unprotected
sections + 5 x LDPC 802.16 r1/2 z = 80, single precision, t_max 25, sumprod2
200 iterations, B = 256, Eb/N0 5.5 dB, the batch generated on the GPU.

One pipeline object holds the plan, the graph and the batch; the two-stage
decoder is that object's stages without the final pass (AMP, soft output, BP,
count), so both decode the same received words through the same plan.  Host
clock around `steps` decodes that end in a device synchronise, after a warm-up
decode of each; windows of the two decoders alternate, `repeats` of each,
medians reported.  The final pass's share of the time is (three - two) / three
of the medians per decode: what the known-sections kernel and the second AMP
add.  The error counters of both decoders on the batch are reported beside
the times.

Then, on the same plan and batch, ms per AMP iteration of
sg_amp_decode_bpsk_partial_device with no word known against
sg_amp_decode_bpsk_device (6 iterations each at rtol 1e-12, alternating
windows): the known branch of the section kernel should cost nothing.

The measurement runs in a child process under a time limit; a fault, an abort
or the limit ends the run.  Results go to profiles/bpsk_concat3.json.  Needs a
GPU.

    python tools/bpsk_concat3_time.py [--batch 256] [--steps 4] [--repeats 5] [--ebn0 5.5]
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
IT_TMAX, IT_RTOL = 7, 1e-12  # the per-iteration comparison: 6 iterations, no early stop
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
    from ldpc_sparc_amd.pipeline import DctBpskConcat3Pipeline
    _native.require_gpu()
    pipe = DctBpskConcat3Pipeline(L, M, N, P, LU, MULTS, ldpc=LDPC, design_seed=1234, precision="f32", t_max=T_MAX,
                                  final_t_max=a.final_t_max)
    user_bits = LU * PER + MULTS * pipe.c.K
    var = P / (2 * (user_bits / N) * 10 ** (a.ebn0 / 10))
    B = a.batch
    pipe.make_batch_device(B, var, 5000, 0)

    def two_stage():  # decode() without _final_pass
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
    cps = {name: res[name]["codewords_per_s"] for name in decoders}
    res.update(final_pass_ms=three - two, final_pass_share=(three - two) / three,
               three_over_two_codewords_per_s=cps["three_stage"] / cps["two_stage"])
    res["iteration"] = iteration_cost(pipe, var, a)
    return res


def iteration_cost(pipe, var, a):
    """ms per AMP iteration of the decode with no word known against the plain K = 2 decode, same plan and batch."""
    from ldpc_sparc_amd import _native
    lib, B = _native.lib(), pipe.B
    pipe.op.soft_output(False, pipe.prec)  # (the plain decode alone would store s; nothing reads it here)
    d_none = _native.DeviceBuffer.from_array(np.full((B, L), -1, np.int32))
    d_tf = _native.DeviceBuffer(B * 4)

    def plain():
        _native.check(lib.sg_amp_decode_bpsk_device(pipe.plan, pipe.d_y.ptr, B, None, var, IT_TMAX, IT_RTOL, 1,
                                                    pipe.d_idx.ptr, d_tf.ptr, None, None, None))

    def partial():
        _native.check(lib.sg_amp_decode_bpsk_partial_device(pipe.plan, pipe.d_y.ptr, B, d_none.ptr, None, var, IT_TMAX,
                                                            IT_RTOL, 1, pipe.d_idx.ptr, d_tf.ptr, None, None, None))
    its = IT_TMAX - 1
    out = {"iterations_per_decode": its}
    ran = []
    for fn in (plain, partial):  # warm-up
        fn()
        _native.device_synchronize()
        ran.append(int(d_tf.download(np.zeros(B, np.int32)).min()))
    out["all_iterations_ran"] = ran == [its, its]
    tb, tp = [], []
    for _ in range(a.repeats):
        tb.append(_window(plain, a.steps))
        tp.append(_window(partial, a.steps))
    per = lambda t: 1e3 * float(t) / (a.steps * its)  # noqa: E731
    out.update(bpsk_window_seconds=tb, partial_window_seconds=tp, bpsk_ms_per_iteration=per(np.median(tb)),
               partial_ms_per_iteration=per(np.median(tp)), bpsk_spread_ms_per_iteration=per(np.max(tb) - np.min(tb)),
               partial_spread_ms_per_iteration=per(np.max(tp) - np.min(tp)))
    out["partial_over_bpsk"] = out["partial_ms_per_iteration"] / out["bpsk_ms_per_iteration"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ebn0", type=float, default=5.5)
    ap.add_argument("--final-t-max", type=int, default=None, dest="final_t_max")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bpsk_concat3.json"))
    ap.add_argument("--json", help=argparse.SUPPRESS)  # child mode: measure, result to this file
    a = ap.parse_args()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(measure(a), f)
        return 0
    out = {"geometry": {"L": L, "M": M, "K": 2, "n": N, "P": P, "L_unprotected": LU, "mults": MULTS,
                        "ldpc": list(LDPC), "t_max": T_MAX, "precision": "f32"},
           "what": "host clock around `steps` decodes of one device batch ending in a device synchronise, after a "
                   "warm-up decode of each decoder; alternating windows, median of `repeats`; both decoders on the "
                   "same pipeline object, plan and batch; `iteration`: ms per AMP iteration of "
                   "sg_amp_decode_bpsk_partial_device with no word known against sg_amp_decode_bpsk_device there"}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "result.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--json", path, "--batch", str(a.batch), "--steps",
               str(a.steps), "--repeats", str(a.repeats), "--ebn0", str(a.ebn0)]
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
            for name in ("two_stage", "three_stage", "iteration"):
                r = out["result"][name]
                print(name, json.dumps({k: r[k] for k in r if not k.endswith("window_seconds")}), flush=True)
        else:  # a fault, an abort or the time limit
            out["failed"] = {"exit_status": rc, "limit_s": LIMIT_S}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if "result" in out else 1


if __name__ == "__main__":
    sys.exit(main())
