"""The integrated AMP <-> BP decoders of both designs against the outputs recorded from the library before their
two host loops became one (integ_loop.hpp; tests/golden/integ_same_bits.npz, made by
tests/golden/make_golden_integ_same_bits.py): bits, tau^2 history and (DCT entry point) the final BP output equal
bit for bit, in every mode and both precisions.  Every reduction of these kernels is fixed-order, so equality is the
condition; there is no tolerance.  Cases and shapes: tests/integ_same_bits_cases.py.

The shared workspace (IntegWs) grow-only through one fresh plan: B = 1, 3, 1, 3; the two B = 3 results are equal
(and the recorded ones), as are the two B = 1 results.
"""
import os

import numpy as np
import pytest

import integ_same_bits_cases as sb

pytestmark = pytest.mark.gpu

CASES = [(d, m, p) for d in sb.DESIGNS for m in sb.MODES for p in sb.PRECISIONS if (d, m, p) not in sb.LEFT_OUT]


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", sb.FIXTURE)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def designs(integrated_golden, recorded):
    ds = sb.Designs(integrated_golden, recorded)
    yield ds
    ds.release()


def check(got, recorded, design, mode, prec):
    assert set(got) == ({"bits", "tau2"} if design == "dense" else {"bits", "app", "tau2"})
    for what, v in got.items():
        assert sb.same_bits(v, recorded[sb.key(design, mode, prec, what)]), (design, mode, prec, what)


@pytest.mark.parametrize("design,mode,prec", CASES)
def test_same_bits_as_before_the_one_loop(designs, recorded, design, mode, prec):
    check(designs.decode(design, mode, prec), recorded, design, mode, prec)


@pytest.mark.parametrize("prec", list(sb.PRECISIONS))
@pytest.mark.parametrize("design", sb.DESIGNS)
def test_workspace_regrow_through_one_plan(designs, recorded, design, prec):
    mode = "integrated_posteriors"
    designs.designs[design].release()  # a fresh plan: B = 1 carves the workspace, B = 3 releases and re-carves it
    one = designs.decode(design, mode, prec, 1)
    first = designs.decode(design, mode, prec, 3)
    one_again = designs.decode(design, mode, prec, 1)
    again = designs.decode(design, mode, prec, 3)
    for what in first:
        assert sb.same_bits(again[what], first[what]), what
        assert sb.same_bits(one_again[what], one[what]), what
        assert one[what].shape[0] * 3 == first[what].shape[0]
    check(first, recorded, design, mode, prec)
