"""Golden complex / K-PSK SPARC cases (tests/golden/make_golden_csparc.py writes
their fixture) and the helpers the complex-SPARC tests share."""
import functools
import glob
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
P, AWGN_VAR = 15.0, 1.0

# name, code_params (plus P and complex), decode_params, seeds
CSPARC_CASES = [
    ("creg", {'R': 2.4, 'L': 64, 'M': 64}, {'t_max': 25}, 3),
    ("cpsk4", {'R': 2.4, 'L': 64, 'M': 32, 'modulated': True, 'K': 4}, {'t_max': 25}, 3),
    ("cpsk8", {'R': 2.0, 'L': 64, 'M': 16, 'modulated': True, 'K': 8}, {'t_max': 25}, 3),
    ("cpsk16", {'R': 2.0, 'L': 32, 'M': 16, 'modulated': True, 'K': 16}, {'t_max': 25}, 2),
    ("cpsk2m2", {'R': 2.0, 'L': 64, 'M': 32, 'modulated': True, 'K': 2}, {'t_max': 25, 'phi_est_method': 2}, 2),
    ("cpa4", {'R': 2.6, 'L': 64, 'M': 32, 'modulated': True, 'K': 4, 'power_allocated': True, 'B': 4,
              'R_PA_ratio': 1.0}, {'t_max': 30}, 2),
    ("csc4", {'R': 2.2, 'L': 32, 'M': 64, 'modulated': True, 'K': 4, 'spatially_coupled': True, 'omega': 2,
              'Lambda': 4}, {'t_max': 40}, 2),
    ("csc1", {'R': 2.2, 'L': 32, 'M': 64, 'spatially_coupled': True, 'omega': 2, 'Lambda': 4}, {'t_max': 40}, 2),
    # the reference notebook's geometry, w = 2^15
    ("cnb", {'R': 2.6, 'L': 2048, 'M': 8, 'modulated': True, 'K': 4}, {'t_max': 25}, 1),
]
EST_K = (1, 2, 4, 8)        # estimator vectors: L = 16, M = 32
EST_L, EST_M = 16, 32
PSK_K = (2, 4, 8, 16)       # psk_mod / psk_demod vectors


def code_params(cp):
    out = {'P': P, 'complex': True}
    out.update(cp)
    return out


def seed_of(si):
    return [7 * si + 1, 2000 + si]


def all_seeds():
    for name, cp, dp, ns in CSPARC_CASES:
        for si in range(ns):
            yield name, code_params(cp), dict(dp), si


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/csparc_golden.npz (or its _p<k> parts) as one name -> array mapping."""
    paths = sorted(glob.glob(os.path.join(HERE, "golden", "csparc_golden*.npz")))
    if not paths:
        raise FileNotFoundError("tests/golden/csparc_golden*.npz")
    out = {}
    for path in paths:
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def design(g, name, cp):
    """(W, L, M, n, order0, order1) of seed 0 of a golden case, orders as the reference drew them."""
    from ldpc_sparc_amd import sparc
    cp = dict(cp)
    sparc.check_code_params(cp)
    tmp = cp.copy()
    tmp.update({'awgn_var': AWGN_VAR})
    W = sparc.create_base_matrix(**tmp)
    key = f"{name}_s0"
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
