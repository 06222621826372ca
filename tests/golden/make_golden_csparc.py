"""Complex / K-PSK SPARC fixtures from the reference (sparc_public), written to
tests/golden/csparc_golden.npz (split into parts if it outgrows one file).

Build-container only (imports the reference via ref_harness).  The hook wraps
sparc.sub_fft to record the row/column orders of every design block the
reference drew (seed 0 of each case).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness  # noqa: E402
from csparc_cases import (AWGN_VAR, CSPARC_CASES, EST_K, EST_L, EST_M, PSK_K, code_params,  # noqa: E402
                          seed_of)


def sym_index(sparc, vals, K):
    if K == 1:
        return np.zeros(vals.size, dtype=np.int32)
    c = sparc.psk_constel(K)
    return np.array([int(np.argwhere(c == v)[0, 0]) for v in vals], dtype=np.int32)


def make():
    _, sparc, sparc_sim, _, _, _ = ref_harness.import_reference()
    out = {}
    orig_sub_fft = sparc.sub_fft
    for name, cp0, dp0, nseeds in CSPARC_CASES:
        for si in range(nseeds):
            seed = seed_of(si)
            cp, dp = code_params(cp0), dict(dp0)
            orders = []

            def sub_fft_hook(m, n, seed=0, order0=None, order1=None):
                orders.append((np.array(order0, dtype=np.uint32), np.array(order1, dtype=np.uint32)))
                return orig_sub_fft(m, n, seed, order0, order1)
            sparc.sub_fft = sub_fft_hook
            try:
                bits_i, beta0, x, Ab, Az = sparc.sparc_encode(cp, AWGN_VAR, seed)
                y = sparc_sim.awgn_channel(x, AWGN_VAR, seed)
                bits_o, beta, T, nmse, expect = sparc.sparc_decode(y, cp, dp, AWGN_VAR, seed, beta0, Ab, Az)
            finally:
                sparc.sub_fft = orig_sub_fft
            L, M = cp['L'], cp['M']
            K = cp['K'] if cp['modulated'] else 1
            assert np.all(np.isfinite(nmse)), name
            key = f"{name}_s{si}"
            out[key + "_n"] = np.array(cp['n'])
            out[key + "_bits"] = bits_i
            out[key + "_y"] = y
            out[key + "_x"] = x
            br = beta.reshape(L, M)
            rows, cols = np.nonzero(br)
            assert np.array_equal(rows, np.arange(L))
            out[key + "_map"] = cols.astype(np.int32)
            out[key + "_map_sym"] = sym_index(sparc, br[rows, cols], K)
            out[key + "_t_final"] = np.array(T)
            out[key + "_nmse"] = np.array(nmse)
            out[key + "_expect"] = np.array(bool(expect))
            out[key + "_bits_out"] = bits_o
            if si == 0:
                out[key + "_order0"] = np.stack([o[0] for o in orders])
                out[key + "_order1"] = np.stack([o[1] for o in orders])
            res = sparc_sim.sparc_sim(code_params(cp0), dict(dp0), AWGN_VAR, seed)
            for k, v in res.items():
                if k != 'nmse':
                    out[key + "_sim_" + k] = np.array(v)
            print(key, "n", cp['n'], "T", T, "ber", res['ber'], "ser", res['ser'], "blocks", len(orders))
    # stand-alone estimators on a random complex s
    rng = np.random.RandomState(20)
    for K in EST_K:
        beta0 = sparc.rnd_msg_vector(EST_L, EST_M, [K, 5], K)
        tau = 0.3
        s = beta0 + np.sqrt(tau / 2) * (rng.randn(EST_L * EST_M) + 1j * rng.randn(EST_L * EST_M))
        out[f"est{K}_s"] = s
        out[f"est{K}_tau"] = np.array(tau)
        out[f"est{K}_mmse"] = np.asarray(sparc.msg_vector_mmse_estimator(s.copy(), tau, EST_M, K))
        out[f"est{K}_map"] = np.asarray(sparc.msg_vector_map_estimator(s.copy(), EST_M, K))
    # PSK modulation on fixed bits
    for K in PSK_K:
        bits = sparc.rnd_bin_arr(24 * int(np.log2(K)), [K, 9])
        sym = sparc.psk_mod(bits, K)
        out[f"psk{K}_bits"] = bits
        out[f"psk{K}_sym"] = sym
        out[f"psk{K}_demod"] = sparc.psk_demod(sym, K)
        out[f"rnd{K}_msg"] = sparc.rnd_msg_vector(12, 8, [K, 3], K)
    # one ordering draw for a 2-D W (the reference's generate_ordering is nested in sparc_transforms)
    W = sparc.sc_basic(np.array(15.0), 2, 4)
    orders = []

    def sub_fft_hook2(m, n, seed=0, order0=None, order1=None):
        orders.append((np.array(order0, dtype=np.uint32), np.array(order1, dtype=np.uint32)))
        return orig_sub_fft(m, n, seed, order0, order1)
    sparc.sub_fft = sub_fft_hook2
    try:
        sparc.sparc_transforms(W, 8, 16, 5 * 9, [4, 44], True)
    finally:
        sparc.sub_fft = orig_sub_fft
    out["ord2d_order0"] = np.stack([o[0] for o in orders])
    out["ord2d_order1"] = np.stack([o[1] for o in orders])
    path = os.path.join(HERE, "csparc_golden.npz")
    np.savez_compressed(path, **out)
    if os.path.getsize(path) > 900 * 1024:
        os.remove(path)
        import golden_parts
        golden_parts.save_parts("csparc_golden", out)
    print("wrote csparc_golden", sum(np.asarray(v).nbytes for v in out.values()) / 1e6, "MB raw")


if __name__ == "__main__":
    make()
