"""Pins tests/golden/csparc_large_golden.npz (the reference's runs at transform
sizes 2^17 to 2^20) to the package's host code at these sizes, without a GPU:
the package's own order draw, fed to the NumPy restatement of the design
operator (tests/csparc_ref.py), reproduces the reference's codeword."""
import numpy as np
import pytest

import csparc_ref
from csparc_large_cases import CASES, K_of, LARGE_CASES, golden, ref_orders, transforms
from ldpc_sparc_amd import sparc


@pytest.mark.parametrize("name", [c[0] for c in LARGE_CASES])
def test_fixture_matches_host_code(name):
    g, key = golden(), f"{name}_s0"
    cp, W, n, Ab, Az = transforms(name, 0)
    op = sparc.operator_of(Ab, Az)  # no plan is built: orders and sizes only
    L, M, K = cp['L'], cp['M'], K_of(cp)
    assert op.w == 2 ** CASES[name][4]
    o0, o1 = ref_orders(op, W)
    rAb, _ = csparc_ref.fft_operators(W, L, M, n, o0, o1)
    x = rAb(sparc.bin_arr_2_msg_vector(g[key + "_bits"], M, K).astype(complex))
    ref = g[key + "_x"]
    assert np.max(np.abs(x - ref)) / np.max(np.abs(ref)) < 1e-12
    assert g[key + "_x"].shape == (n,) and g[key + "_y"].shape == (n,)
    assert g[key + "_map"].shape == (L,) and g[key + "_map_sym"].shape == (L,)
