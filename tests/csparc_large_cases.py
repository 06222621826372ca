"""Golden complex SPARC cases with 2^17 to 2^20-point transforms
(tests/golden/make_golden_csparc_large.py writes their fixture,
tests/golden/csparc_large_golden.npz) and the helpers their tests share.

The fixture holds no orders (order1 alone is 2 MB at 2^19 entries): the tests
draw them with the package's own sparc_transforms(..., seed, True), which
tests/test_csparc_host.py pins to the reference's draws.
"""
import functools
import os

import numpy as np

from csparc_cases import AWGN_VAR, code_params, seed_of  # noqa: F401  (re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))

# name, code_params (plus P and complex), decode_params, seed indices (seed_of), log2 w
LARGE_CASES = [
    ("cbig17", {'R': 2.4, 'L': 512, 'M': 128, 'modulated': True, 'K': 4}, {'t_max': 25}, (0, 1), 17),
    ("cbig18sc", {'R': 2.0, 'L': 1024, 'M': 512, 'spatially_coupled': True, 'omega': 2, 'Lambda': 4}, {'t_max': 40},
     (0, 1), 18),
    ("cbig20", {'R': 2.4, 'L': 1024, 'M': 512}, {'t_max': 25}, (0, 1), 20),
]
CASES = {c[0]: c for c in LARGE_CASES}


def all_seeds(names=None):
    for name, cp, dp, seeds, _ in LARGE_CASES:
        if names is None or name in names:
            for si in seeds:
                yield name, code_params(cp), dict(dp), si


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(HERE, "golden", "csparc_large_golden.npz")) as z:
        return {k: z[k] for k in z.files}


def K_of(cp):
    return cp['K'] if cp.get('modulated') else 1


def base_matrix(cp):
    """(checked code_params, W) of a case."""
    from ldpc_sparc_amd import sparc
    cp = dict(cp)
    sparc.check_code_params(cp)
    tmp = cp.copy()
    tmp.update({'awgn_var': AWGN_VAR})
    return cp, sparc.create_base_matrix(**tmp)


def transforms(name, si):
    """(cp, W, n, Ab, Az) of a case-seed: the package's own order draw for seed_of(si)."""
    from ldpc_sparc_amd import sparc
    cp, W = base_matrix(code_params(CASES[name][1]))
    n = int(golden()[f"{name}_s{si}_n"])
    Ab, Az = sparc.sparc_transforms(W, cp['L'], cp['M'], n, seed_of(si), True)
    return cp, W, n, Ab, Az


def ref_orders(op, W):
    """The operator's orders in the layout tests/csparc_ref.py takes: per base-matrix entry."""
    if W.ndim == 0:
        return op.order0[0], op.order1[0]
    if W.ndim == 1:
        return op.order0, op.order1
    Lr, Lc = W.shape
    o0 = np.zeros((Lr, Lc, op.Mr), np.uint32)
    o1 = np.zeros((Lr, Lc, op.Mc), np.uint32)
    nz = [(r, c) for r in range(Lr) for c in range(Lc) if W[r, c] != 0]
    assert len(nz) == op.order0.shape[0]
    for t, (r, c) in enumerate(nz):
        o0[r, c], o1[r, c] = op.order0[t], op.order1[t]
    return o0, o1
