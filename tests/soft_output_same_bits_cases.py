"""Inputs and calls shared by tests/golden/make_golden_soft_output_same_bits.py (run once, on the library of the
commit before the soft-output kernels were rewritten on csrc/section_bits.hpp) and
tests/test_soft_output_same_bits_gpu.py (which compares the current library with the SHA-256 digests that run
recorded of every raw output buffer).

Geometries: those of tests/section_size_cases.py at M = 2, 64, 128, 512, 1024, 2048 -- idle lanes, a full
VMAX = 1, the first high bit, a full VMAX = 8 and the VMAX = 32 instance at two sizes -- with their batch of B = 3
received words, decoded for T_SOFT = 3 iterations (the soft point of that sweep: posteriors that are not all hard).
The complex designs take the same (L, M, n) with complex orders and the real batch in both components.  The
integrated decodes are cases A, B, C of tests/dct_integrated_cases.py (VMAX 1, 8, 32).

Every device call asks for sections [1, L - 1) -- l0 > 0, a count that is no multiple of the four wavefronts of a
workgroup -- into rows PAD values longer than the range, in a buffer preset to GUARD: the digest is of the whole
buffer, and the tail is asserted untouched.  A case's outputs: name -> array.

    family   entry points                                       kernel
    reg      sg_amp_llr_device, sg_amp_llr (regular engine)     reg_llr_kernel<T, 1 | 8 | 32>
    gen      the same on a general-engine plan                  glue_llr_kernel<T>, round_p = 1
    glue     sg_beta_to_llr_device                              glue_llr_kernel<T>, round_p = 0
    bpsk     sg_amp_bpsk_llr_device, sg_amp_bpsk_llr            bpsk_llr_kernel<T, 1 | 8 | 32>
    camp     sg_camp_llr_device, sg_camp_llr, K = 1, 2, 4, 8    camp_llr_kernel, with tau
    psk      sg_section_llr_psk, K = 1, 2, 4, 8                 camp_llr_kernel, null tau
    idct     sg_amp_integrated_decode_device                    idct_section_kernel<T, 1 | 8 | 32> (vk0, llr, ua)
"""
import contextlib
import hashlib
import os

import numpy as np

import dct_integrated_cases as dc
import section_size_cases as ssc
from ldpc_sparc_amd import _native, sparc

B, T_SOFT = ssc.B, ssc.T_SOFT
SIZES = ("m2", "m64", "m128", "m512", "m1024", "m2048")
PRECISIONS = {"f64": _native.SG_F64, "f32": _native.SG_F32}
PSK_ORDERS = (1, 2, 4, 8)
CAMP_ALL_K = "m128"  # every K at this size, K = 4 at every size
IDCT = {"A": "integrated", "B": "integrated_posteriors", "C": "naive"}
IDCT_T_MAX, IDCT_BP_ITS, IDCT_BP_ITS_FINAL = 4, 3, 30
PAD, GUARD = 3, -777.0
PSK_L = 9
FIXTURE = "soft_output_same_bits.npz"
# (case id, reason) of every case that the pinned library did not reproduce on a second run, so not in the fixture: none
LEFT_OUT = ()


def case_ids():
    ids = [(f, m, p) for f in ("reg", "gen", "glue", "bpsk") for m in SIZES for p in PRECISIONS]
    ids += [("camp", m, f"k{k}") for m in SIZES for k in PSK_ORDERS if k == 4 or m == CAMP_ALL_K]
    ids += [("psk", m, f"k{k}") for m in SIZES for k in PSK_ORDERS]
    ids += [("idct", name, p) for name in IDCT for p in PRECISIONS]
    return ids


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def key(cid, what):
    return "_".join(cid) + "_" + what


@contextlib.contextmanager
def _engine(general):
    """SG_AMP_ENGINE=legacy while a plan is built selects the general engine."""
    old = os.environ.pop("SG_AMP_ENGINE", None)
    if general:
        os.environ["SG_AMP_ENGINE"] = "legacy"
    try:
        yield
    finally:
        os.environ.pop("SG_AMP_ENGINE", None)
        if old is not None:
            os.environ["SG_AMP_ENGINE"] = old


def _ranged(dtype, per, L, call):
    """{'p0': LLRs, 'p1': probabilities} of sections [1, L - 1) through a device entry point:
    call(l0, nl, ld, probs_only, d_llr) -> status; the whole [B, ld] buffers, guard tails included."""
    l0, nl = 1, L - 2
    assert nl % 4 != 0
    ld = nl * per + PAD
    out = {}
    for probs_only in (0, 1):
        buf = _native.DeviceBuffer.from_array(np.full((B, ld), GUARD, dtype))
        _native.check(call(l0, nl, ld, probs_only, buf.ptr))
        _native.synchronize()
        got = buf.download(np.empty((B, ld), dtype))
        assert np.all(got[:, nl * per:] == GUARD)
        out[f"p{probs_only}"] = got
    return out


class Runner:
    """Operators are built once per (family, size) and kept until release()."""

    def __init__(self):
        self.ops = {}

    def release(self):
        self.ops.clear()

    def _real_op(self, size, general):
        if (size, general) not in self.ops:
            c = ssc.case(size)
            op = sparc.DesignOperator(c.W, c.L, c.M, c.n, c.o0, c.o1)
            with _engine(general):
                for prec in PRECISIONS.values():
                    op.plan(prec)
            self.ops[size, general] = op
        return self.ops[size, general]

    def _complex_op(self, size):
        if (size, "c") not in self.ops:
            c = ssc.case(size)
            W = np.array(ssc.P)
            o0, o1 = sparc.generate_ordering(W, c.n, c.L * c.M, ssc.DESIGN_SEED, csparc=True)
            op = sparc.ComplexDesignOperator(W, c.L, c.M, c.n, o0, o1)
            op.soft_output(True)
            self.ops[size, "c"] = op
        return self.ops[size, "c"]

    def run(self, cid):
        return getattr(self, "_" + cid[0])(*cid[1:])

    def _amp_llr(self, size, prec, general):
        c, p = ssc.case(size), PRECISIONS[prec]
        op = self._real_op(size, general)
        lib = _native.lib()
        assert lib.sg_amp_plan_engine(op.plan(p), B) == (0 if general else 1)
        sparc.amp_decode_batch(c.Y, op, ssc.VAR, T_SOFT, rtol=1e-6, true_idx=c.true, precision=p)
        out = _ranged(np.float64 if prec == "f64" else np.float32, c.logM, c.L,
                      lambda l0, nl, ld, po, d: lib.sg_amp_llr_device(op.plan(p), B, l0, nl, ld, po, d, None))
        out["host"] = sparc.amp_llr(op, B, 1, c.L - 2, precision=p)
        return out

    def _reg(self, size, prec):
        return self._amp_llr(size, prec, False)

    def _gen(self, size, prec):
        return self._amp_llr(size, prec, True)

    def _glue(self, size, prec):
        """Section posteriors drawn once (a softmax of 3 N(0, 1) per section), scaled by sqrt(n P / L)."""
        c = ssc.case(size)
        dt = np.float64 if prec == "f64" else np.float32
        snp = float(np.sqrt(c.n * ssc.P / c.L))
        e = np.exp(3.0 * np.random.RandomState(c.M).randn(B, c.L, c.M))
        d_beta = _native.DeviceBuffer.from_array(np.ascontiguousarray((snp * e / e.sum(2, keepdims=True)).astype(dt)))
        lib = _native.lib()
        return _ranged(dt, c.logM, c.L, lambda l0, nl, ld, po, d: lib.sg_beta_to_llr_device(
            PRECISIONS[prec], d_beta.ptr, B, c.L, c.M, snp, l0, nl, ld, po, d, None))

    def _bpsk(self, size, prec):
        c, p = ssc.case(size), PRECISIONS[prec]
        op = self._real_op(size, False)
        op.soft_output(True, p)
        sparc.amp_decode_bpsk_batch(c.Y, op, ssc.VAR, T_SOFT, precision=p)
        lib = _native.lib()
        out = _ranged(np.float64 if prec == "f64" else np.float32, c.logM + 1, c.L,
                      lambda l0, nl, ld, po, d: lib.sg_amp_bpsk_llr_device(op.plan(p), B, l0, nl, ld, po, d, None))
        out["host"] = sparc.amp_llr_bpsk(op, B, 1, c.L - 2, precision=p)
        return out

    def _camp(self, size, k):
        c, K = ssc.case(size), int(k[1:])
        op = self._complex_op(size)
        Y = (c.Y + 1j * c.Y[::-1]) / np.sqrt(2)
        sparc.camp_decode_batch(Y, op, ssc.VAR, T_SOFT, K=K)
        cs = sparc._interleaved(sparc.psk_constel(K)) if K != 1 else None
        lib = _native.lib()
        out = _ranged(np.float64, sparc._section_bit_count(c.M, K), c.L,
                      lambda l0, nl, ld, po, d: lib.sg_camp_llr_device(op.plan(), B, K, _native.ptr(cs), l0, nl, ld, po,
                                                                       d, None))
        out["host"] = sparc.camp_llr(op, B, K, 1, c.L - 2)
        return out

    def _psk(self, size, k):
        """PSK_L sections of complex Gaussian x at growing scales, x given (tau = 2: no division moves it)."""
        M, K = ssc.GEOMETRIES[size][1], int(k[1:])
        rs = np.random.RandomState(1000 * M + K)
        x = (rs.randn(PSK_L, M) + 1j * rs.randn(PSK_L, M)) * (0.1 * 3.0 ** np.arange(PSK_L))[:, None]
        return {f"p{po}": sparc.section_llr_psk(x.reshape(-1), 2.0, M, K, probs_only=bool(po)) for po in (0, 1)}

    def _idct(self, name, prec):
        c, dt = dc.build(name), np.float64 if prec == "f64" else np.float32
        if ("idct", name) not in self.ops:
            self.ops["idct", name] = dc.operator(c)
        op = self.ops["idct", name]
        bits = np.zeros((B, c.nblk * c.K), np.uint8)
        app, tau2 = np.zeros((B * c.nblk, c.N), dt), np.zeros((B, IDCT_T_MAX))
        d_y = _native.DeviceBuffer.from_array(np.ascontiguousarray(c.Y, dtype=dt))
        d_bits, d_app, d_tau = (_native.DeviceBuffer.from_array(a) for a in (bits, app, tau2))
        _native.check(_native.lib().sg_amp_integrated_decode_device(
            op.plan(PRECISIONS[prec]), c.code._device_graph(), _native.INTEGRATED_MODES[IDCT[name]], c.K, d_y.ptr, B,
            IDCT_T_MAX, IDCT_BP_ITS, IDCT_BP_ITS_FINAL, d_bits.ptr, d_app.ptr, d_tau.ptr, None))
        _native.synchronize()
        return {"bits": d_bits.download(bits), "app": d_app.download(app), "tau2": d_tau.download(tau2)}
