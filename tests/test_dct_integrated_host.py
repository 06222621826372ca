"""CPU tests behind the integrated AMP <-> BP decoders on the sub-sampled DCT
design (sg_amp_integrated_decode): they pin the yardstick the GPU tests of
test_dct_integrated_gpu.py use, on exactly the inputs of dct_integrated_cases.

  1. the explicit matrix of dct_integrated_cases equals the oracle's operators:
     Az(e_i) / snp is row i (every row of every case) and Ab(e_j) / snp column j
     (every column of the small cases, a sample of the large ones), to 1e-12;
  2. oracle/integrated_ref.decode on y and on nextafter(y, inf) gives the same
     bits and tau^2 within 1e-12 relative (measured: <= 2.2e-14), in every
     case and mode: the oracle is a 1e-9 yardstick on these inputs;
  3. the operating points: B, C and D decode to the transmitted bits in all
     four modes, A in naivepost and integ, E in none (every codeword of the
     batch of three);
  4. the public header declares both entry points and _native binds them.
"""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import dct_integrated_cases as dc
from oracle import integrated_ref, sparc_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_explicit_matrix_is_the_oracle_operator(name):
    c = dc.build(name)
    LM = c.L * c.M
    Ab, Az = sparc_ref.dct_operators(np.array(dc.P), c.L, c.M, c.n, c.order0, c.order1)
    for i in range(c.n):  # the adjoint gives whole rows: every entry of the matrix
        e = np.zeros(c.n)
        e[i] = 1.0
        assert np.max(np.abs(Az(e) / c.snp - c.A[i])) <= 1e-12, (name, i)
    cols = range(LM) if LM <= 2048 else np.random.default_rng(0).choice(LM, 48, replace=False)
    for j in cols:
        e = np.zeros(LM)
        e[j] = 1.0
        assert np.max(np.abs(Ab(e) / c.snp - c.A[:, j])) <= 1e-12, (name, j)
    # unit-norm columns on average, as N(0, 1/n) columns
    assert abs(np.mean(np.sum(c.A ** 2, axis=0)) - 1.0) < 0.05


@pytest.mark.parametrize("mode", dc.ORACLE_MODES)
@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_oracle_is_stable_under_one_ulp(oracle_built, name, mode):
    c = dc.build(name)
    bits, taus = dc.oracle(name, mode)
    y1 = np.nextafter(c.Y[0], np.inf)
    b1, t1 = integrated_ref.decode(mode, y1, c.A, dc.P, c.L, c.M, c.graph, c.N, c.K, dc.T_MAX)
    assert np.array_equal(np.asarray(b1, dtype=np.uint8), bits[0])
    rel = np.max(np.abs(np.asarray(t1) - taus[0]) / np.abs(taus[0]))
    print(f"{name} {mode}: tau^2 moves by {rel:.2e} relative under one ulp of y")
    assert rel < 1e-12


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_operating_points(oracle_built, name):
    c = dc.build(name)
    for mode in dc.ORACLE_MODES:
        bits, taus = dc.oracle(name, mode)
        assert taus.shape == (dc.B, dc.T_MAX) and np.all(np.isfinite(taus))
        errs = (bits != c.bits_in).sum(axis=1)
        print(f"{name} {mode}: bit errors per codeword {errs.tolist()} of {c.nblk * c.K}")
        if mode in dc.DECODES[name]:
            assert np.all(errs == 0), (name, mode, errs)
        if name == "E":
            assert np.all(errs > 0), (name, mode, errs)


def test_header_and_binding_have_the_entry_points():
    from ldpc_sparc_amd import _native
    src = open(os.path.join(REPO, "include", "ldpc_sparc_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    bound = {n: a for n, _, a in _native.SIGNATURES}
    for name, nargs in (("sg_amp_integrated_decode_device", 13), ("sg_amp_integrated_decode", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == nargs
        assert name in bound and len(bound[name]) == nargs
        assert hasattr(_native.lib(), name)
    assert _native.lib().sg_amp_integrated_decode.restype is ct.c_int
