"""Inputs and decode calls shared by tests/golden/make_golden_integ_same_bits.py (run once, on the library of the
commit before the integrated decoders became one loop) and tests/test_integrated_same_bits_gpu.py (which compares
the current library with what that run recorded, bit for bit).

Two designs, the smallest of the existing integrated suites:
  dense  integ0 of tests/golden/integrated_golden_p*.npz: L = 108, M = 64, n = 648, 802.11n r1/2 z = 27 (one block
         per codeword).  A is regenerated from the fixture's seed (35 MB, not committed; the new fixture holds its
         SHA-256), the three received words are y plus growing noise, as tests/test_plan_memory_gpu.py draws them.
  dct    case A of tests/dct_integrated_cases.py: L = 24, M = 64, n = 144, 802.16 r1/2 z = 3 (two blocks).
B = 3 codewords, t_max = 4 (iteration 0, two middle iterations, the final branch), 3 inner and 30 final BP
iterations, every mode, both precisions.  Outputs: the information bits, tau^2 of every iteration, and for the DCT
entry point the final BP output app.
"""
import hashlib

import numpy as np

import dct_integrated_cases as dc
from ldpc_sparc_amd import _native, sparc_new
from ldpc_sparc_amd.ldpc import code

B, T_MAX, BP_ITS, BP_ITS_FINAL = 3, 4, 3, 30
MODES = ("naive", "naive_posteriors", "integrated", "integrated_posteriors")
PRECISIONS = {"f64": _native.SG_F64, "f32": _native.SG_F32}
DESIGNS = ("dense", "dct")
FIXTURE = "integ_same_bits.npz"
# (design, mode, precision) that the pinned library did not reproduce on a second run, so not in the fixture: none
LEFT_OUT = ()


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dense_inputs(integrated_golden):
    """(A, L, M, P, Y [B, n]) of the dense design."""
    from test_oracle_pin import integrated_case
    y, A, L, M, P, _, _, _, _ = integrated_case(integrated_golden, "integ0")
    rng = np.random.default_rng(3)
    Y = np.stack([y + 0.1 * b * rng.standard_normal(y.size) for b in range(B)])
    return A, L, M, P, Y


class Designs:
    """The two designs on the GPU, their codes and received words; inputs from the fixture when it is given."""

    def __init__(self, integrated_golden, fixture=None):
        A, L, M, P, Y = dense_inputs(integrated_golden)
        c = dc.build("A")
        self.inputs = {"dense_A_sha256": np.array(sha256(A)), "dense_Y": Y, "dct_Y": np.array(c.Y),
                       "dct_order0": np.array(c.order0), "dct_order1": np.array(c.order1)}
        if fixture is not None:  # the regenerated design must be the recorded one; the received words are read
            assert str(fixture["dense_A_sha256"]) == sha256(A)
            assert np.array_equal(fixture["dct_order0"], c.order0) and np.array_equal(fixture["dct_order1"], c.order1)
            self.inputs["dense_Y"], self.inputs["dct_Y"] = fixture["dense_Y"], fixture["dct_Y"]
        self.case = c
        self.codes = {"dense": code('802.11n', '1/2', 27), "dct": c.code}
        self.designs = {"dense": sparc_new.DenseDesign(A, P, L, M), "dct": sparc_new.DctDesign(dc.operator(c))}

    def release(self):
        for d in self.designs.values():
            d.release()

    def decode(self, design, mode, prec, nB=B):
        """name -> array of the outputs of one decode of the first nB received words."""
        Y = self.inputs[design + "_Y"][:nB]
        if design == "dense":
            bits, tau2 = sparc_new.integrated_decode_batch(Y, self.designs["dense"], self.codes["dense"], mode, T_MAX,
                                                           BP_ITS, BP_ITS_FINAL, PRECISIONS[prec])
            return {"bits": bits, "tau2": tau2}
        c, dt = self.case, np.float64 if prec == "f64" else np.float32
        bits = np.zeros((nB, c.nblk * c.K), np.uint8)
        app, tau2 = np.zeros((nB * c.nblk, c.N), dt), np.zeros((nB, T_MAX))
        d_y = _native.DeviceBuffer.from_array(np.ascontiguousarray(Y, dtype=dt))
        d_bits, d_app, d_tau = (_native.DeviceBuffer.from_array(a) for a in (bits, app, tau2))
        _native.check(_native.lib().sg_amp_integrated_decode_device(
            self.designs["dct"].plan(PRECISIONS[prec]), c.code._device_graph(), _native.INTEGRATED_MODES[mode], c.K,
            d_y.ptr, nB, T_MAX, BP_ITS, BP_ITS_FINAL, d_bits.ptr, d_app.ptr, d_tau.ptr, None))
        _native.synchronize()
        return {"bits": d_bits.download(bits), "app": d_app.download(app), "tau2": d_tau.download(tau2)}


def key(design, mode, prec, what):
    return f"{design}_{mode}_{prec}_{what}"


def same_bits(a, b):
    """np.array_equal on the bit patterns (so that a NaN equals the same NaN)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
