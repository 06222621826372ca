"""Every soft-output entry point against the SHA-256 digests recorded from the library before its kernels were
rewritten on the shared bit-marginal core (csrc/section_bits.hpp; tests/golden/soft_output_same_bits.npz, made by
tests/golden/make_golden_soft_output_same_bits.py): the raw output buffers, guard tails included, equal bit for
bit.  Every reduction of these kernels is fixed-order, so equality is the condition; there is no tolerance.
Families, shapes and section range: tests/soft_output_same_bits_cases.py.
"""
import os

import numpy as np
import pytest

import soft_output_same_bits_cases as sb

pytestmark = pytest.mark.gpu

CASES = [c for c in sb.case_ids() if c not in {tuple(l[0]) for l in sb.LEFT_OUT}]


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", sb.FIXTURE)) as z:
        return {k: str(z[k]) for k in z.files}


@pytest.fixture(scope="module")
def runner():
    r = sb.Runner()
    yield r
    r.release()


def test_every_case_is_recorded_or_left_out_with_a_reason(recorded):
    """LEFT_OUT holds (case id, reason) pairs; the kernels are fixed-order, so the list is expected to be empty."""
    for left in sb.LEFT_OUT:
        assert len(left) == 2 and tuple(left[0]) in sb.case_ids() and str(left[1]).strip(), left
    have = {k.rsplit("_", 1)[0] for k in recorded}
    assert {"_".join(c) for c in CASES} <= have
    assert len(CASES) + len(sb.LEFT_OUT) == len(sb.case_ids())


@pytest.mark.parametrize("cid", CASES, ids=["-".join(c) for c in CASES])
def test_same_bits_as_before_the_shared_core(runner, recorded, cid):
    got = runner.run(cid)
    assert {sb.key(cid, k) for k in got} == {k for k in recorded if k.rsplit("_", 1)[0] == "_".join(cid)}
    for what, v in got.items():
        assert sb.sha256(v) == recorded[sb.key(cid, what)], (cid, what)
