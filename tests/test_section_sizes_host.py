"""The operating points of the section-size sweep, pinned with the oracle alone
(no GPU): tests/test_section_sizes_gpu.py means something only where these
hold.

- t_max = 3 leaves at least 100 bit probabilities inside (0.01, 0.99) at every
  geometry, so a wrong marginal moves a value far from 0 and 1;
- at M >= 128 at least 10 of them are marginals of the index bits >= 6 -- the
  bits that reg_llr_kernel takes from its per-lane partial sums and
  glue_llr_kernel from the later trips of its loop;
- at M >= 8 the oracle decodes every section and stops by itself before
  t_max = 25, so the comparison of the whole trajectory at 1e-9 is one of a
  contracting iteration (mixed stopping).  M = 2 and M = 4 stall and
  take part in the t_max = 3 leg only.

The floors are far below the oracle's own counts (printed; for the flat
geometries 171 .. 509 soft probabilities, 20 .. 60 of the last codeword's in
the high bits)."""
import pytest

import section_size_cases as ssc


@pytest.mark.parametrize("name", ssc.NAMES + ["m4096"])
def test_soft_point_is_soft(name):
    c = ssc.case(name)
    soft, hi, hi_last = c.soft_counts()
    print(f"{name}: L={c.L} M={c.M} n={c.n}: {soft} probabilities in (0.01, 0.99) at t_max={ssc.T_SOFT}, "
          f"{hi} in bits >= 6 ({hi_last} of the last codeword)")
    assert soft >= 100
    if c.M >= 128:
        assert hi >= 10
    if c.blocks:  # the power-allocated case has column blocks that differ: a tau per block, not one
        assert c.W.shape == (c.blocks,) and len(set(c.W.tolist())) >= 2, c.W


@pytest.mark.parametrize("name", ssc.CONVERGING + ["m4096"])
def test_full_decode_converges(name):
    c = ssc.case(name)
    o = c.oracle(ssc.T_FULL)
    errs = int((o["map"] != c.true).sum())
    print(f"{name}: t_final {o['t_final'].tolist()}, {errs} section errors at t_max={ssc.T_FULL}")
    assert errs == 0
    assert (o["t_final"] < ssc.T_FULL).all()


def test_stalled_sizes_are_left_out_for_a_reason():
    """M = 2 and M = 4 are kept out of the t_max = 25 leg because the oracle
    itself runs out of iterations there; if that changes, they belong in it."""
    for name in ("m2", "m4"):
        assert name not in ssc.CONVERGING
        assert ssc.case(name).oracle(ssc.T_FULL)["t_final"].max() == ssc.T_FULL - 1
