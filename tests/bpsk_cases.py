"""Golden real K = 2 (BPSK) modulated SPARC cases (tests/golden/make_golden_bpsk.py
writes their fixture) and the helpers the K = 2 tests share.

The reference's results at generation time, three seeds each:
  breg    n 384, decodes in 6            breg_m2 the same with phi_est_method 2
  bM2     n 640, decodes in 6-7          bM2048  n 96; seeds 0, 1 decode in 7-8, seed 2 runs to 24 with SER 1
  bpa     n 295, decodes in 10-14        bsc     n 205, decodes in 7-10
  bhard   n 240, runs to 24, SER 0.05-0.31
M = 2 and M = 2048 are the ends of the section kernel's dispatch; bsc has phi
per row block; bhard and bM2048 seed 2 hold wrong decisions, sign errors and
no early stop.  Every section of every seed passed the generator's margin
check (largest |s| ahead of the runner-up and of zero by more than 1e-6), so
no seed index was moved."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
P, AWGN_VAR = 15.0, 1.0

# name, code_params (plus P, modulated, K = 2), decode_params, seeds
BPSK_CASES = [
    ("breg", {'R': 1.0, 'L': 64, 'M': 32}, {'t_max': 25}, 3),
    ("breg_m2", {'R': 1.0, 'L': 64, 'M': 32}, {'t_max': 25, 'phi_est_method': 2}, 3),
    ("bM2", {'R': 0.8, 'L': 256, 'M': 2}, {'t_max': 25}, 3),
    ("bM2048", {'R': 1.0, 'L': 8, 'M': 2048}, {'t_max': 25}, 3),
    ("bpa", {'R': 1.3, 'L': 64, 'M': 32, 'power_allocated': True, 'B': 4, 'R_PA_ratio': 1.0}, {'t_max': 30}, 3),
    ("bsc", {'R': 1.1, 'L': 32, 'M': 64, 'spatially_coupled': True, 'omega': 2, 'Lambda': 4}, {'t_max': 40}, 3),
    ("bhard", {'R': 1.6, 'L': 64, 'M': 32}, {'t_max': 25}, 3),
]


def code_params(cp):
    out = {'P': P, 'modulated': True, 'K': 2}
    out.update(cp)
    return out


def seed_of(si):
    return [7 * si + 1, 3000 + si]


def all_seeds():
    for name, cp, dp, ns in BPSK_CASES:
        for si in range(ns):
            yield name, code_params(cp), dict(dp), si


IDS = [f"{name}-s{si}" for name, _, _, si in all_seeds()]


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/bpsk_golden.npz as one name -> array mapping."""
    with np.load(os.path.join(HERE, "golden", "bpsk_golden.npz")) as z:
        return {k: z[k] for k in z.files}


def design(g, name, cp):
    """(W, L, M, n, order0, order1) of seed 0 of a golden case, orders as the reference drew them."""
    from ldpc_sparc_amd import sparc
    key = f"{name}_s0"
    cp = dict(cp)
    sparc.check_code_params(cp)
    tmp = cp.copy()
    tmp.update({'awgn_var': AWGN_VAR})
    W = sparc.create_base_matrix(**tmp)
    n = int(g[key + "_n"])
    L, M = cp['L'], cp['M']
    o0, o1 = g[key + "_order0"], g[key + "_order1"]
    if W.ndim == 0:
        return W, L, M, n, o0[0], o1[0]
    if W.ndim == 1:
        return W, L, M, n, o0, o1
    Lr, Lc = W.shape
    O0 = np.zeros((Lr, Lc, o0.shape[1]), np.uint32)
    O1 = np.zeros((Lr, Lc, o1.shape[1]), np.uint32)
    nz = [(r, c) for r in range(Lr) for c in range(Lc) if W[r, c] != 0]
    for t, (r, c) in enumerate(nz):
        O0[r, c] = o0[t]
        O1[r, c] = o1[t]
    return W, L, M, n, O0, O1


def words(loc, sym):
    """Section words (location << 1) | symbol."""
    return ((np.asarray(loc, dtype=np.int64) << 1) | np.asarray(sym, dtype=np.int64)).astype(np.int32)


def true_words(bits, M):
    """The transmitted words of a codeword's bits: the MSB-first value of each
    section's log2 M + 1 bits."""
    k = int(np.log2(M)) + 1
    return (np.asarray(bits).reshape(-1, k).astype(np.int64) @ (1 << np.arange(k)[::-1])).astype(np.int32)
