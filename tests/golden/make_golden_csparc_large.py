"""Complex SPARC fixtures with 2^17 to 2^20-point transforms from the reference
(sparc_public), written to tests/golden/csparc_large_golden.npz.

Build-container only (imports the reference via ref_harness).  The orders are
not stored (tests/csparc_large_cases.py).  For every case-seed the generator
also prints how close the reference's stop test np.allclose(psi, psi_prev)
(sparc.py:984) came to its threshold: the smallest over the iterations of
| max_c (|psi - psi_prev| / (atol + rtol |psi_prev|)) - 1 |.  A seed whose
figure is below 1e-10 may stop one iteration apart in another arithmetic.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness  # noqa: E402
from csparc_large_cases import AWGN_VAR, LARGE_CASES, code_params, seed_of  # noqa: E402
from make_golden_csparc import sym_index  # noqa: E402


def make():
    _, sparc, sparc_sim, _, _, _ = ref_harness.import_reference()
    out = {}
    orig_allclose = np.allclose
    for name, cp0, dp0, seeds, lg in LARGE_CASES:
        for si in seeds:
            seed = seed_of(si)
            cp, dp = code_params(cp0), dict(dp0)
            trace = []

            def allclose_hook(a, b, rtol=1e-05, atol=1e-08, **kw):
                a_, b_ = np.atleast_1d(a), np.atleast_1d(b)
                trace.append(float(np.max(np.abs(a_ - b_) / (atol + rtol * np.abs(b_)))))
                return orig_allclose(a, b, rtol, atol, **kw)
            bits_i, beta0, x, Ab, Az = sparc.sparc_encode(cp, AWGN_VAR, seed)
            y = sparc_sim.awgn_channel(x, AWGN_VAR, seed)
            t0 = time.perf_counter()
            np.allclose = allclose_hook
            try:
                bits_o, beta, T, nmse, expect = sparc.sparc_decode(y, cp, dp, AWGN_VAR, seed, beta0, Ab, Az)
            finally:
                np.allclose = orig_allclose
            dt = time.perf_counter() - t0
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
            res = sparc_sim.sparc_sim(code_params(cp0), dict(dp0), AWGN_VAR, seed)
            for k, v in res.items():
                if k != 'nmse':
                    out[key + "_sim_" + k] = np.array(v)
            print(key, "n", cp['n'], "T", T, "ber", res['ber'], "ser", res['ser'], "decode s", round(dt, 2),
                  "stop-test margin", min(abs(r - 1) for r in trace), "ratios",
                  " ".join(f"{r:.6g}" for r in trace), flush=True)
    path = os.path.join(HERE, "csparc_large_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.basename(path), os.path.getsize(path), "bytes;",
          sum(np.asarray(v).nbytes for v in out.values()) / 1e6, "MB raw")


if __name__ == "__main__":
    make()
