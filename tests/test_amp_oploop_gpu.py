"""The known-sections decode and the real K = 2 decode run one operator loop
(amp_oploop.hip, oploop_impl): one residual, control and init kernel, a
section kernel per family.  The merge changes no operand and no order of
operations, so both decodes are required to give the bits of the library that
had a loop and a kernel set per family: tests/golden/amp_oploop_golden.npz
holds the inputs and map, t_final, NMSE and psi recorded from that library
(`python tests/test_amp_oploop_gpu.py OUT.npz` records them with whichever
library is loaded).  The received words, known sets and true sections are read
from the file too, so that equality does not hang on the host's transform and
random number libraries; only the designs are rebuilt (integer orderings).

Every case is a batch of three with one noisy codeword, so that codewords
stop at different iterations; both precisions.

  known sections: "flat", "pa" and "m16" of test_amp_partial_gpu.py (codewords
  0, 2 and 6: none known, the protected ones with one wrong index, a random
  subset; codeword 6 at noise sigma 2.2, m16's with more noise added) and
  "m2", "m2048" of the section-size sweep with test_section_size_bounds' known
  sets, each with phi_est_method 1 and 2; "flat" with every section unknown
  and with every section known.
  K = 2: the seven cases of bpsk_cases.py on the design of seed 0 (W of ndim 0,
  1 and 2, M = 2 and M = 2048): the fixture's codeword and two more, the last
  at noise sigma 2.5.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "amp_oploop_golden.npz")
T_MAX, VAR = 25, 1.0
ROWS = [0, 2, 6]
PRECS = ["f64", "f32"]
OUTPUTS = ("map", "tf", "nmse", "psi")

# (case, phi_est_method) of the known-sections decode
KNOWN = [(name, phi) for name in ("flat", "pa", "m16", "m2", "m2048") for phi in (1, 2)]
KNOWN += [("flat_none", 1), ("flat_all", 1)]


def _bpsk_seed0():
    """name -> Seed of seed 0 (test_bpsk_gpu.py)."""
    import test_bpsk_gpu as bg
    from bpsk_cases import BPSK_CASES, code_params
    return {name: bg.seed_case(name, code_params(cp), dict(dp), 0) for name, cp, dp, _ in BPSK_CASES}


BPSK = ["breg", "breg_m2", "bM2", "bM2048", "bpa", "bsc", "bhard"]


def _prec(precision):
    from ldpc_sparc_amd import _native
    return _native.SG_F64 if precision == "f64" else _native.SG_F32


_ops = {}


def _known_op(name):
    """The GPU operator of a known-sections case (the designs of the modules named above, made once there)."""
    import section_size_cases as ssc
    import test_amp_partial_gpu as pg
    from ldpc_sparc_amd import sparc
    base = name.split("_")[0]
    if base in ("m2", "m2048"):
        if base not in _ops:
            s = ssc.case(base)
            _ops[base] = sparc.DesignOperator(s.W, s.L, s.M, s.n, s.o0, s.o1)
        return _ops[base]
    return pg.case(base).op


def _decode_known(data, name, phi, precision):
    from ldpc_sparc_amd import sparc
    return sparc.amp_decode_partial_batch(data[f"{name}_y"], _known_op(name), data[f"{name}_known"], VAR, T_MAX,
                                          phi_est_method=phi, true_idx=data[f"{name}_true"],
                                          precision=_prec(precision))


def _decode_bpsk(data, name, precision):
    from bpsk_cases import AWGN_VAR
    from ldpc_sparc_amd import sparc
    c = _bpsk_seed0()[name]
    return sparc.amp_decode_bpsk_batch(data[f"{name}_y"], c.op, AWGN_VAR, c.dp['t_max'], c.dp['rtol'],
                                       c.dp['phi_est_method'], data[f"{name}_true"], _prec(precision))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _require_equal(golden, key, got):
    for k, v in zip(OUTPUTS, got):
        g = golden[f"{key}_{k}"]
        assert g.dtype == v.dtype and g.shape == v.shape and np.array_equal(g, v), (key, k, int(np.sum(g != v)))


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name,phi", KNOWN, ids=[f"{n}-phi{p}" for n, p in KNOWN])
def test_known_sections_bits_of_the_library_before(golden, name, phi, precision):
    _require_equal(golden, f"{name}_p{phi}_{precision}", _decode_known(golden, name, phi, precision))


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", BPSK)
def test_bpsk_bits_of_the_library_before(golden, name, precision):
    _require_equal(golden, f"{name}_{precision}", _decode_bpsk(golden, name, precision))


def test_recorded_batches_stop_at_different_iterations(golden):
    """What the cases are for, read off the recording: the three codewords do not stop together, except at the
    rate at which AMP fails (bhard: none stops) and in the batch with nothing to decode (psi = 0 from the start,
    so it stops at the first comparison)."""
    for name, phi in KNOWN:
        if name != "flat_all":
            assert len(set(golden[f"{name}_p{phi}_f64_tf"].tolist())) >= 2, name
    assert np.all(golden["flat_all_p1_f64_nmse"][:, 1:] == 0) and np.all(golden["flat_all_p1_f64_tf"] == 2)
    for name in BPSK:
        if name != "bhard":
            assert len(set(golden[f"{name}_f64_tf"].tolist())) >= 2, name


# ---------------------------------------------------------------- recording

def _more_noise(Y, sigma, seed):
    """Y with N(0, sigma^2) added to its last codeword."""
    Y = np.array(Y, dtype=np.float64)
    Y[-1] += sigma * np.random.RandomState(seed).randn(Y.shape[1])
    return Y


def _known_inputs(name):
    """(Y [3, n], known [3, L], true [3, L]) of a known-sections case."""
    import amp_partial_ref as pr
    import section_size_cases as ssc
    import test_amp_partial_gpu as pg
    base = name.split("_")[0]
    if base in ("m2", "m2048"):
        s = ssc.case(base)
        known = pr.mixed_known(np.concatenate([s.true, s.true[2:]]), s.L // 2, s.M, 5)[[0, 1, 3]]
        return _more_noise(s.Y, 1.5, 17), known, s.true
    c = pg.case(base)
    Y, known, true = c.Y[ROWS], c.known[ROWS], c.true[ROWS]
    if base == "m16":  # (its batch is at sigma 1 throughout)
        Y = _more_noise(Y, 1.5, 17)
    if name == "flat_none":
        known = np.full_like(known, -1)
    if name == "flat_all":
        known = true
    return Y, known, true


def _bpsk_inputs(name):
    """(Y [3, n], true words [3, L]): the fixture's codeword of seed 0 and two drawn here, the last at sigma 2.5."""
    import test_bpsk_gpu as bg
    from ldpc_sparc_amd import _native
    c = _bpsk_seed0()[name]
    rng = np.random.RandomState(41)
    tw = np.concatenate([c.tw[None], rng.randint(0, 2 * c.M, (2, c.L))]).astype(np.int32)
    X = bg._encode_device(c.op, tw[1:], _native.SG_F64)
    Y = np.concatenate([c.y[None], X + np.array([1.0, 2.5])[:, None] * rng.randn(2, c.n)])
    return Y, tw


if __name__ == "__main__":  # record the inputs and the golden arrays with the loaded library
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    out = {}
    for name in sorted({n for n, _ in KNOWN}):
        Y, known, true = _known_inputs(name)
        out[f"{name}_y"], out[f"{name}_known"], out[f"{name}_true"] = Y, known.astype(np.int32), true.astype(np.int32)
    for name in BPSK:
        out[f"{name}_y"], out[f"{name}_true"] = _bpsk_inputs(name)
    runs = [(f"{n}_p{phi}_{pc}", _decode_known, (n, phi, pc)) for n, phi in KNOWN for pc in PRECS]
    runs += [(f"{n}_{pc}", _decode_bpsk, (n, pc)) for n in BPSK for pc in PRECS]
    for key, fn, args in runs:
        got = fn(out, *args)
        again = fn(out, *args)
        for a, b in zip(got, again):
            assert np.array_equal(a, b), key  # the recording library gives the same bits twice
        for k, v in zip(OUTPUTS, got):
            out[f"{key}_{k}"] = v
        errors = (got[0] != out[args[0] + "_true"]).sum(axis=1)
        print(key, "t_final", got[1].tolist(), "section errors", errors.tolist(), flush=True)
    np.savez_compressed(sys.argv[1], **out)
