"""Batched, device-resident concatenated SPARC + LDPC decoding (the hot loop of
sparc_sim_new.sparc_ldpc_sim with many codewords sharing one design).

Per batch: dense AMP (sparc_new.py:885-912) -> MAP bits of the
unprotected sections (:70-71) -> bit LLRs of the protected sections
(beta_estimate_to_bp_probs :1118-1138 and ldpc_bp's clip/log :1167-1169) ->
batched BP over every LDPC block (ldpc_bp :1176-1187, sumprod2, 200 iterations
by default) -> device-side error counts.  Nothing returns to the host but the
five counters.
"""
import ctypes as ct

import numpy as np

from . import _native
from .ldpc import code
from .sparc_new import DenseDesign


class ConcatPipeline:
    def __init__(self, L, M, n, P, L_unprotected, mults, ldpc=("802.11n", "1/2", 81), design_seed=0,
                 precision="f32", t_max=25, bp_dectype="sumprod2", bp_its=200, A=None):
        self._init_common(L, M, n, P, int(np.log2(M)), 0, L_unprotected, mults, ldpc, precision, t_max, bp_dectype,
                          bp_its)
        self.design = DenseDesign(A, P, L, M, n=n, seed=design_seed)
        self.plan = self.design.plan(self.prec)
        self.graph = self.c._device_graph()
        self.snp = float(np.sqrt(n * P / L))

    def _init_common(self, L, M, n, P, logM, logK, L_unprotected, mults, ldpc, precision, t_max, bp_dectype, bp_its):
        """What every pipeline holds whatever its design: the shape, the LDPC code, the precision and the
        iteration counts.  A section carries bits_per_section = logM + logK bits."""
        self.L, self.M, self.n, self.P = int(L), int(M), int(n), float(P)
        self.logM, self.bits_per_section = logM, logM + logK
        self.L_unp, self.mults = int(L_unprotected), int(mults)
        self.c = code(*ldpc)
        assert (self.L - self.L_unp) * self.bits_per_section == self.mults * self.c.N, \
            "protected sections must hold the blocks"
        self.prec = {"f64": _native.SG_F64, "f32": _native.SG_F32}[precision]
        self.dt = np.float64 if self.prec == _native.SG_F64 else np.float32
        self.t_max, self.bp_dectype, self.bp_its = int(t_max), bp_dectype, int(bp_its)
        self._cap = 0

    def _ensure(self, B):
        if B <= self._cap:
            return
        c, sz = self.c, np.dtype(self.dt).itemsize
        self.d_y = _native.DeviceBuffer(B * self.n * sz)
        self.d_x = _native.DeviceBuffer(B * self.n * sz)
        self.d_idx = _native.DeviceBuffer(B * self.L * 4)
        self.d_true = _native.DeviceBuffer(B * self.L * 4)
        self.d_llr = _native.DeviceBuffer(B * self.mults * c.N * sz)
        self.d_app = _native.DeviceBuffer(B * self.mults * c.N * sz)
        self.d_it = _native.DeviceBuffer(B * self.mults * 4)
        self.d_info = _native.DeviceBuffer(B * self.mults * c.K)
        self.d_unp = _native.DeviceBuffer(max(1, B * self.L_unp * self.bits_per_section))
        self.d_cw = _native.DeviceBuffer(B * self.mults * c.N)
        self.d_cnt = _native.DeviceBuffer(5 * 8)
        self._cap = B

    def _encode(self, B):
        """x = A beta0 [B, n] on the device for the section indices in d_true."""
        _native.check(_native.lib().sg_dense_encode_device(self.plan, self.d_true.ptr, B, self.d_x.ptr, None))

    def make_batch(self, B, awgn_var, rng):
        """Random user bits -> LDPC blocks -> section indices; x = A beta0 on
        the GPU; y = x + AWGN (host RNG).  Leaves y, the true indices and the
        information bits resident on the device.  A section's index is the
        MSB-first value of its bits_per_section bits (log2 M on the
        unmodulated designs)."""
        self._ensure(B)
        c, per = self.c, self.bits_per_section
        unp = rng.integers(0, 2, (B, self.L_unp * per))
        info = rng.integers(0, 2, (B * self.mults, c.K))
        cw = c.encode_batch(info).reshape(B, self.mults * c.N)
        bits = np.concatenate([unp, cw], axis=1).reshape(B, self.L, per)
        idx = (bits.astype(np.int64) @ (1 << np.arange(per)[::-1])).astype(np.int32)
        self.d_true.upload(idx)
        self.d_info.upload(info.reshape(B, -1).astype(np.uint8))
        self._encode(B)
        x = self.d_x.download(np.empty((B, self.n), self.dt))
        y = (x + np.sqrt(awgn_var) * rng.standard_normal(x.shape)).astype(self.dt)
        self.d_y.upload(y)
        self.B, self.awgn_var = B, float(awgn_var)
        return idx, info

    # distinct Philox keys of the parts of a device batch
    _SEED_INFO = 0x5DEECE66D

    def make_batch_device(self, B, awgn_var, seed, stream_id):
        """The same batch generated on the GPU (throughput mode, nothing from
        the host): Philox user bits of the unprotected sections and of the
        LDPC information words (sparc_new.py:15-51), the systematic LDPC
        encoder (ldpc.py:400-460) on the device, MSB-first bits -> section
        indices, x = A beta0, y = x + AWGN.  The draw of codeword b depends only
        on (seed, stream_id, b): a Monte-Carlo block keyed by (point, block) is
        the same whatever the rank count."""
        self._ensure(B)
        c, per, lib = self.c, self.bits_per_section, _native.lib()
        off = _native.offset
        nu = self.L_unp * per
        if nu:
            _native.check(lib.sg_rng_bits_device(seed, stream_id, B, nu, self.d_unp.ptr, None))
            _native.check(lib.sg_bits_to_sections_strided_device(self.d_unp.ptr, nu, B, self.L_unp, per,
                                                                 self.d_true.ptr, self.L, None))
        _native.check(lib.sg_rng_bits_device(seed ^ self._SEED_INFO, stream_id, B * self.mults, c.K, self.d_info.ptr,
                                             None))
        c.encode_device(self.d_info.ptr, B * self.mults, self.d_cw.ptr)
        _native.check(lib.sg_bits_to_sections_strided_device(self.d_cw.ptr, self.mults * c.N, B, self.L - self.L_unp,
                                                             per, off(self.d_true.ptr, 4 * self.L_unp), self.L, None))
        self._encode(B)
        _native.check(lib.sg_awgn_device(self.prec, seed, stream_id, self.d_x.ptr, B, self.n,
                                         float(np.sqrt(awgn_var)), self.d_y.ptr, None))
        self.B, self.awgn_var = B, float(awgn_var)

    def decode(self):
        """One batch: returns nothing; counters accumulate in d_cnt.  The stages below, of which a subclass
        overrides those that differ on its design or in its decoder."""
        self._amp()
        self._soft_output()
        self._bp()
        self._final_pass()
        self._count()

    def _amp(self):
        """AMP on d_y; the section decisions into d_idx."""
        lib, B = _native.lib(), self.B
        _native.check(lib.sg_dense_amp_device(self.plan, self.d_y.ptr, B, self.t_max, None, None, None))
        self._d_beta, d_s = ct.c_void_p(), ct.c_void_p()
        _native.check(lib.sg_dense_state_device(self.plan, ct.byref(self._d_beta), ct.byref(d_s)))
        _native.check(lib.sg_dense_map_device(self.plan, d_s, B, self.d_idx.ptr, None))

    def _soft_output(self):
        """The bit LLRs of the protected sections, from the state the AMP left, into d_llr."""
        _native.check(_native.lib().sg_beta_to_llr_device(
            self.prec, self._d_beta, self.B, self.L, self.M, self.snp, self.L_unp, self.L - self.L_unp,
            self.mults * self.c.N, 0, self.d_llr.ptr, None))

    def _bp(self):
        """BP over every LDPC block of the batch: d_llr -> d_app, d_it."""
        _native.check(_native.lib().sg_ldpc_decode_device(
            self.graph, _native.DECTYPES[self.bp_dectype], self.prec, self.d_llr.ptr, self.B * self.mults, self.bp_its,
            0.7, self.d_app.ptr, self.d_it.ptr, None))

    def _final_pass(self):
        """Nothing here; the three-stage decoders' AMP pass with the BP-decoded sections known."""

    def _known_sections(self):
        """d_known (a three-stage decoder's buffer): the hard decisions of every protected section whose LDPC
        blocks stopped on their syndrome, -1 elsewhere."""
        _native.check(_native.lib().sg_concat_known_sections_device(
            self.prec, self.d_app.ptr, self.d_it.ptr, self.bp_its, self.B, self.mults, self.c.N, self.L, self.L_unp,
            self.bits_per_section, self.d_known.ptr, None))

    def _count(self, d_idx=None):
        """d_cnt += the errors of the sections in d_idx (default: self.d_idx) and of the BP output in d_app."""
        c = self.c
        _native.check(_native.lib().sg_concat_count_errors_device(
            self.prec, (self.d_idx if d_idx is None else d_idx).ptr, self.d_true.ptr, self.B, self.L, self.L_unp,
            self.bits_per_section, self.d_app.ptr, self.d_info.ptr, self.mults, c.N, c.K, self.d_cnt.ptr, None))

    def reset_counts(self):
        self.d_cnt.zero()

    def counts(self):
        _native.synchronize()
        return self.d_cnt.download(np.zeros(5, np.int64))


class DctConcatPipeline(ConcatPipeline):
    """The same concatenated scheme on the sub-sampled DCT design (sparc.py
    :703-880) instead of the dense Gaussian matrix: statistically the same
    code, decoded by the DCT-design AMP engines.  Same methods, device buffers
    and counter layout as ConcatPipeline, so montecarlo.ConcatTrial takes it
    unchanged.

    `op` is a sparc.DesignOperator over (L, M, n): flat, power-allocated, or
    spatially coupled in double precision (the single-precision block engines
    give no soft output).  By default it is the flat design W = P with the
    orders sparc_transforms draws from `design_seed`.

    decode() per batch, nothing returning to the host but the five counters:
    sg_amp_decode_device (its map_idx gives the unprotected bits) ->
    sg_amp_llr_device over the protected sections (the bit LLRs from the
    engine's final s and tau) -> sg_ldpc_decode_device ->
    sg_concat_count_errors_device.

    The AMP here is the public decoder (sparc.py:883-999): known noise variance
    or the residual estimate (`phi_method` = phi_est_method 1 / 2) and early
    stopping at `rtol`, up to t_max - 1 iterations per codeword -- not the
    dense pipeline's fixed t_max iterations with the empirical tau^2
    (sparc_new.py:885-912).  Error rates of the two pipelines agree
    statistically, not codeword by codeword."""

    def __init__(self, L, M, n, P, L_unprotected, mults, ldpc=("802.11n", "1/2", 81), design_seed=0,
                 precision="f32", t_max=25, rtol=1e-6, phi_method=1, bp_dectype="sumprod2", bp_its=200, op=None):
        from . import sparc
        self._init_common(L, M, n, P, int(np.log2(M)), 0, L_unprotected, mults, ldpc, precision, t_max, bp_dectype,
                          bp_its)
        self.rtol, self.phi_method = float(rtol), int(phi_method)
        if op is None:
            W = np.array(float(P))
            o0, o1 = sparc.generate_ordering(W, self.n, self.L * self.M, design_seed)
            op = sparc.DesignOperator(W, self.L, self.M, self.n, o0, o1)
        if op.csparc or (op.L, op.M, op.n) != (self.L, self.M, self.n):
            raise ValueError(f"op must be a real DesignOperator with L = {self.L}, M = {self.M}, n = {self.n}")
        self.op = op
        self.plan = op.plan(self.prec)
        self.graph = self.c._device_graph()

    def _encode(self, B):
        _native.check(_native.lib().sg_amp_encode_device(self.plan, self.d_true.ptr, B, self.d_x.ptr, None))

    def _amp(self):
        _native.check(_native.lib().sg_amp_decode_device(
            self.plan, self.d_y.ptr, self.B, None, self.awgn_var, self.t_max, self.rtol, self.phi_method,
            self.d_idx.ptr, None, None, None, None))

    def _soft_output(self):
        _native.check(_native.lib().sg_amp_llr_device(self.plan, self.B, self.L_unp, self.L - self.L_unp,
                                                      self.mults * self.c.N, 0, self.d_llr.ptr, None))


class DctBpskConcatPipeline(DctConcatPipeline):
    """The concatenated scheme on a real K = 2 (BPSK) modulated SPARC with the
    sub-sampled DCT design: a section carries log2 M location bits, MSB first,
    and then one symbol bit (0: +1, 1: -1) -- the digits of its word
    (location << 1) | symbol (sparc.bpsk_words) -- so bits_per_section =
    log2 M + 1 stands where the unmodulated pipelines have logM, and d_true /
    d_idx hold words.  The last L - L_unprotected sections hold `mults` LDPC
    blocks.  Same methods, device buffers and counter layout as
    ConcatPipeline, so montecarlo.ConcatTrial takes it unchanged.

    `op` is a real sparc.DesignOperator over (L, M, n): flat, power-allocated
    or spatially coupled, either precision -- every plan
    sg_amp_decode_bpsk_device takes (M a power of two in [2, 2048]).  By
    default the flat design W = P with the orders drawn from `design_seed`.

    decode() per batch, nothing returning to the host but the five counters:
    sg_amp_decode_bpsk_device with soft output on (its map_word gives the
    unprotected bits) -> sg_amp_bpsk_llr_device over the protected sections
    (bit LLRs from the joint posterior over (location, sign) of the decoder's
    last s and tau) -> sg_ldpc_decode_device -> sg_concat_count_errors_device
    on the words.  The three-stage decoder with a final AMP pass is
    DctBpskConcat3Pipeline."""

    def __init__(self, L, M, n, P, L_unprotected, mults, ldpc=("802.11n", "1/2", 81), design_seed=0,
                 precision="f32", t_max=25, rtol=1e-6, phi_method=1, bp_dectype="sumprod2", bp_its=200, op=None):
        from . import sparc
        self.K = 2
        self._init_common(L, M, n, P, int(round(np.log2(int(M)))), 1, L_unprotected, mults, ldpc, precision, t_max,
                          bp_dectype, bp_its)
        self.rtol, self.phi_method = float(rtol), int(phi_method)
        if op is None:
            W = np.array(float(P))
            o0, o1 = sparc.generate_ordering(W, self.n, self.L * self.M, design_seed)
            op = sparc.DesignOperator(W, self.L, self.M, self.n, o0, o1)
        if op.csparc or (op.L, op.M, op.n) != (self.L, self.M, self.n):
            raise ValueError(f"op must be a real DesignOperator with L = {self.L}, M = {self.M}, n = {self.n}")
        self.op = op
        self.plan = op.plan(self.prec)
        op.soft_output(True, self.prec)
        self.graph = self.c._device_graph()

    def _encode(self, B):
        """x = A beta0 [B, n] on the device for the section words in d_true."""
        _native.check(_native.lib().sg_amp_encode_bpsk_device(self.plan, self.d_true.ptr, B, self.d_x.ptr, None))

    def _amp(self):
        _native.check(_native.lib().sg_amp_decode_bpsk_device(
            self.plan, self.d_y.ptr, self.B, None, self.awgn_var, self.t_max, self.rtol, self.phi_method,
            self.d_idx.ptr, None, None, None, None))

    def _soft_output(self):
        _native.check(_native.lib().sg_amp_bpsk_llr_device(self.plan, self.B, self.L_unp, self.L - self.L_unp,
                                                           self.mults * self.c.N, 0, self.d_llr.ptr, None))


class DctConcat3Pipeline(DctConcatPipeline):
    """The three-stage decoder AMP -> BP -> AMP of the concatenated scheme on
    the DCT design.  decode() runs DctConcatPipeline's AMP, soft output and BP,
    then turns the BP result into known sections
    (sg_concat_known_sections_device: the hard decisions of every protected
    section whose LDPC blocks stopped on their syndrome) and decodes the same
    received words again with them given (sg_amp_decode_partial_device, up to
    `final_t_max` - 1 iterations, default t_max): the unprotected sections
    then face the residual y - A beta_known at L_unprotected / L of the rate.
    Errors are counted with the second pass's map_idx for the unprotected
    sections and the same BP output for the protected bits.  Same methods,
    device buffers and counter layout as ConcatPipeline, so
    montecarlo.ConcatTrial takes it unchanged.  Flat and power-allocated
    designs (a spatially coupled `op` raises ValueError)."""

    def __init__(self, *args, final_t_max=None, **kw):
        super().__init__(*args, **kw)
        if self.op.W.ndim == 2:
            raise ValueError("the final AMP pass takes a flat or power-allocated design, not a spatially coupled one")
        self.final_t_max = self.t_max if final_t_max is None else int(final_t_max)

    def _ensure(self, B):
        if B <= self._cap:
            return
        super()._ensure(B)
        self.d_known = _native.DeviceBuffer(B * self.L * 4)

    def _final_pass(self):
        self._known_sections()
        _native.check(_native.lib().sg_amp_decode_partial_device(
            self.plan, self.d_y.ptr, self.B, self.d_known.ptr, None, self.awgn_var, self.final_t_max, self.rtol,
            self.phi_method, self.d_idx.ptr, None, None, None, None))


class DctBpskConcat3Pipeline(DctBpskConcatPipeline):
    """The three-stage decoder AMP -> BP -> AMP of the concatenated scheme on
    a real K = 2 SPARC.  decode() runs DctBpskConcatPipeline's AMP, soft output
    and BP, then turns the BP result into known section words
    (sg_concat_known_sections_device at log2 M + 1 bits per section: its
    output is the word (location << 1) | symbol, no unpack step) and decodes
    the same received words again with them given
    (sg_amp_decode_bpsk_partial_device, up to `final_t_max` - 1 iterations,
    default t_max): the unprotected sections then face the residual
    y - A beta_known at L_unprotected / L of the rate.  Errors are counted with
    the final pass's words for the unprotected sections and the same BP output
    for the protected bits.  Flat, power-allocated and spatially coupled
    designs in either precision.  Same methods, device buffers and counter
    layout as ConcatPipeline, so montecarlo.ConcatTrial takes it unchanged:
    campaigns run through ConcatTrial(DctBpskConcat3Pipeline(...)) with
    montecarlo.run_point.  concat_ber_sweep(design="dct", K=2,
    final_amp=True) still raises; wiring that switch is a follow-up that
    edits the one test pinning its text."""

    def __init__(self, *args, final_t_max=None, **kw):
        super().__init__(*args, **kw)
        self.final_t_max = self.t_max if final_t_max is None else int(final_t_max)

    def _ensure(self, B):
        if B <= self._cap:
            return
        super()._ensure(B)
        self.d_known = _native.DeviceBuffer(B * self.L * 4)

    def _final_pass(self):
        self._known_sections()
        _native.check(_native.lib().sg_amp_decode_bpsk_partial_device(
            self.plan, self.d_y.ptr, self.B, self.d_known.ptr, None, self.awgn_var, self.final_t_max, self.rtol,
            self.phi_method, self.d_idx.ptr, None, None, None, None))


class DctIntegratedPipeline(DctConcatPipeline):
    """The AMP <-> BP integrated decoders (sparc_new.py:257-282, :411-439, :472-502, :675-705) on the flat
    sub-sampled DCT design: `bp_its` BP iterations inside each of the t_max AMP iterations and a final
    `bp_its_final`-iteration decode (sg_amp_integrated_decode_device), counted on the device from its final BP
    output.  Every section is LDPC protected (L_unprotected = 0, ldpc_bp's assert :1171).  Same methods, device
    buffers and counter layout as ConcatPipeline, so montecarlo.ConcatTrial takes it unchanged."""

    def __init__(self, L, M, n, P, L_unprotected=0, mults=None, ldpc=("802.11n", "1/2", 81), design_seed=0,
                 precision="f32", t_max=25, mode="integrated", bp_its=6, bp_its_final=200, op=None):
        if L_unprotected != 0:
            raise ValueError("the integrated decoders protect every section: L_unprotected must be 0")
        if mode not in _native.INTEGRATED_MODES:
            raise ValueError(f"mode must be one of {sorted(_native.INTEGRATED_MODES)}")
        c = code(*ldpc)
        if mults is None:
            mults = int(L) * int(np.log2(M)) // c.N
        super().__init__(L, M, n, P, 0, mults, ldpc=ldpc, design_seed=design_seed, precision=precision, t_max=t_max,
                         bp_dectype="sumprod2", bp_its=bp_its_final, op=op)
        if self.op.W.ndim != 0:
            raise ValueError("the integrated decoders need a flat design (scalar W)")
        self.mode, self.bp_its_inner, self.bp_its_final = mode, int(bp_its), int(bp_its_final)

    def _ensure(self, B):
        if B <= self._cap:
            return
        super()._ensure(B)
        self.d_bits = _native.DeviceBuffer(B * self.mults * self.c.K)

    def decode(self):
        """One batch: returns nothing; counters accumulate in d_cnt."""
        lib, c, B = _native.lib(), self.c, self.B
        _native.check(lib.sg_amp_integrated_decode_device(
            self.plan, self.graph, _native.INTEGRATED_MODES[self.mode], c.K, self.d_y.ptr, B, self.t_max,
            self.bp_its_inner, self.bp_its_final, self.d_bits.ptr, self.d_app.ptr, None, None))
        # no unprotected section: the section-index arguments carry no bits (valid buffers all the same)
        self._count(self.d_true)


class CsparcConcatPipeline(ConcatPipeline):
    """The concatenated scheme on a complex SPARC with the sub-sampled FFT
    design (sparc.py:593-646), unmodulated (K = 1) or K-PSK modulated (K up to
    64): a section carries log2 M location bits and log2 K Gray-coded symbol
    bits, and the last L - L_unprotected sections hold `mults` LDPC blocks.
    Double precision only, like the rest of the complex surface.  Same
    methods and counter layout as ConcatPipeline, so montecarlo.ConcatTrial
    takes it unchanged; `bits_per_section` = log2 M + log2 K stands where the
    real pipelines have logM.

    `op` is a sparc.ComplexDesignOperator over (L, M, n); by default the flat
    design W = P with the orders generate_ordering(..., csparc=True) draws
    from `design_seed`.

    decode() per batch, nothing returning to the host but the five counters:
    sg_camp_decode_device with soft output on (MAP location and symbol of every
    section) -> sg_psk_pack_sections_device (the section's bits as one word) ->
    sg_camp_llr_device over the protected sections (bit LLRs from the joint
    posterior over (location, symbol) of the decoder's last s and tau) ->
    sg_ldpc_decode_device -> sg_concat_count_errors_device on the words."""

    def __init__(self, L, M, K, n, P, L_unprotected, mults, ldpc=("802.11n", "1/2", 81), design_seed=0,
                 precision="f64", t_max=25, rtol=1e-6, phi_method=1, bp_dectype="sumprod2", bp_its=200, op=None):
        from . import sparc
        if precision != "f64":
            raise NotImplementedError("complex SPARCs run in double precision only (precision='f64')")
        self.K = int(K)
        sparc._check_psk(self.K)
        self.logK = int(round(np.log2(self.K)))
        self._init_common(L, M, n, P, int(round(np.log2(int(M)))), self.logK, L_unprotected, mults, ldpc, precision,
                          t_max, bp_dectype, bp_its)
        self.rtol, self.phi_method = float(rtol), int(phi_method)
        if op is None:
            W = np.array(float(P))
            o0, o1 = sparc.generate_ordering(W, self.n, self.L * self.M, design_seed, csparc=True)
            op = sparc.ComplexDesignOperator(W, self.L, self.M, self.n, o0, o1)
        if not op.csparc or (op.L, op.M, op.n) != (self.L, self.M, self.n):
            raise ValueError(f"op must be a ComplexDesignOperator with L = {self.L}, M = {self.M}, n = {self.n}")
        self.op = op
        self.constel = sparc._interleaved(sparc.psk_constel(self.K)) if self.K != 1 else None
        self.plan = op.plan()
        op.soft_output(True)
        self.graph = self.c._device_graph()

    def _ensure(self, B):
        if B <= self._cap:
            return
        c, per = self.c, self.bits_per_section
        self.d_y = _native.DeviceBuffer(B * self.n * 16)
        self.d_x = _native.DeviceBuffer(B * self.n * 16)
        self.d_idx = _native.DeviceBuffer(B * self.L * 4)    # decoded section words
        self.d_true = _native.DeviceBuffer(B * self.L * 4)   # transmitted section words
        self.d_tidx = _native.DeviceBuffer(B * self.L * 4)   # transmitted location / constellation index
        self.d_tsym = _native.DeviceBuffer(B * self.L * 4)
        self.d_midx = _native.DeviceBuffer(B * self.L * 4)   # MAP location / constellation index
        self.d_msym = _native.DeviceBuffer(B * self.L * 4)
        self.d_llr = _native.DeviceBuffer(B * self.mults * c.N * 8)
        self.d_app = _native.DeviceBuffer(B * self.mults * c.N * 8)
        self.d_it = _native.DeviceBuffer(B * self.mults * 4)
        self.d_info = _native.DeviceBuffer(B * self.mults * c.K)
        self.d_unp = _native.DeviceBuffer(max(1, B * self.L_unp * per))
        self.d_cw = _native.DeviceBuffer(B * self.mults * c.N)
        self.d_cnt = _native.DeviceBuffer(5 * 8)
        self.d_tsym.zero()
        self._cap = B

    def _encode(self, B):
        """d_true (words) and x = A beta0 [B, n] from the (location, symbol) pairs in d_tidx / d_tsym."""
        lib = _native.lib()
        _native.check(lib.sg_psk_pack_sections_device(self.d_tidx.ptr, self.d_tsym.ptr, B, self.L, self.logK,
                                                      self.d_true.ptr, None))
        _native.check(lib.sg_camp_encode_device(self.plan, self.K, _native.ptr(self.constel), self.d_tidx.ptr,
                                                self.d_tsym.ptr, B, self.d_x.ptr, None))

    def make_batch(self, B, awgn_var, rng):
        """Random user bits -> LDPC blocks -> (location, symbol) per section
        (bin_arr_2_msg_vector, sparc.py:330-364); x = A beta0 on the GPU;
        y = x + CN(0, awgn_var) from the host RNG (real parts, then imaginary
        parts).  Leaves y, the true section words and the information bits on
        the device; returns (idx [B, L], sym [B, L], info [B * mults, K])."""
        from . import sparc
        self._ensure(B)
        c, logM, per = self.c, self.logM, self.bits_per_section
        unp = rng.integers(0, 2, (B, self.L_unp * per))
        info = rng.integers(0, 2, (B * self.mults, c.K))
        cw = c.encode_batch(info).reshape(B, self.mults * c.N)
        bits = np.concatenate([unp, cw], axis=1).reshape(B, self.L, per).astype(np.int64)
        idx = (bits[:, :, :logM] @ (1 << np.arange(logM)[::-1])).astype(np.int32)
        sym = np.zeros((B, self.L), dtype=np.int32)
        if self.logK:
            sym = sparc.gray2bin(bits[:, :, logM:] @ (1 << np.arange(self.logK)[::-1])).astype(np.int32)
        self.d_tidx.upload(idx)
        self.d_tsym.upload(sym)
        self.d_info.upload(info.reshape(B, -1).astype(np.uint8))
        self._encode(B)
        x = self.d_x.download(np.empty((B, self.n), np.complex128))
        sd = np.sqrt(awgn_var / 2)
        y = x + sd * rng.standard_normal(x.shape) + 1j * (sd * rng.standard_normal(x.shape))
        self.d_y.upload(y)
        self.B, self.awgn_var = B, float(awgn_var)
        return idx, sym, info

    def make_batch_device(self, B, awgn_var, seed, stream_id):
        """The same batch generated on the GPU: Philox user bits of the
        unprotected sections and of the LDPC information words, the device
        LDPC encoder, the strided PSK bit mapper, x = A beta0, complex AWGN of
        variance awgn_var (sqrt(awgn_var / 2) per real dimension).  The draw of
        codeword b depends only on (seed, stream_id, b)."""
        self._ensure(B)
        c, lib, per = self.c, _native.lib(), self.bits_per_section
        off = _native.offset
        nu = self.L_unp * per
        if nu:
            _native.check(lib.sg_rng_bits_device(seed, stream_id, B, nu, self.d_unp.ptr, None))
            _native.check(lib.sg_bits_to_psk_sections_strided_device(
                self.d_unp.ptr, nu, B, self.L_unp, self.logM, self.logK, self.d_tidx.ptr, self.d_tsym.ptr, self.L,
                None))
        _native.check(lib.sg_rng_bits_device(seed ^ self._SEED_INFO, stream_id, B * self.mults, c.K, self.d_info.ptr,
                                             None))
        c.encode_device(self.d_info.ptr, B * self.mults, self.d_cw.ptr)
        _native.check(lib.sg_bits_to_psk_sections_strided_device(
            self.d_cw.ptr, self.mults * c.N, B, self.L - self.L_unp, self.logM, self.logK,
            off(self.d_tidx.ptr, 4 * self.L_unp), off(self.d_tsym.ptr, 4 * self.L_unp), self.L, None))
        self._encode(B)
        _native.check(lib.sg_awgn_device(_native.SG_F64, seed, stream_id, self.d_x.ptr, B, 2 * self.n,
                                         float(np.sqrt(awgn_var / 2)), self.d_y.ptr, None))
        self.B, self.awgn_var = B, float(awgn_var)

    def _pack_map(self):
        """d_idx: the section words of the MAP (location, symbol) pairs in d_midx / d_msym."""
        _native.check(_native.lib().sg_psk_pack_sections_device(self.d_midx.ptr, self.d_msym.ptr, self.B, self.L,
                                                                self.logK, self.d_idx.ptr, None))

    def _amp(self):
        _native.check(_native.lib().sg_camp_decode_device(
            self.plan, self.d_y.ptr, self.B, self.K, _native.ptr(self.constel), None, None, self.awgn_var, self.t_max,
            self.rtol, self.phi_method, self.d_midx.ptr, self.d_msym.ptr, None, None, None, None))
        self._pack_map()

    def _soft_output(self):
        _native.check(_native.lib().sg_camp_llr_device(
            self.plan, self.B, self.K, _native.ptr(self.constel), self.L_unp, self.L - self.L_unp,
            self.mults * self.c.N, 0, self.d_llr.ptr, None))


class CsparcConcat3Pipeline(CsparcConcatPipeline):
    """The three-stage decoder AMP -> BP -> AMP of the concatenated scheme on
    the complex K-PSK design.  decode() runs CsparcConcatPipeline's AMP, soft
    output and BP, then turns the BP result into known section words
    (sg_concat_known_sections_device with bits_per_section: the hard decisions
    of every protected section whose LDPC blocks stopped on their syndrome),
    the words into (location, symbol) pairs (sg_psk_unpack_sections_device),
    and decodes the same received words again with them given
    (sg_camp_decode_partial_device, up to `final_t_max` - 1 iterations, default
    t_max): the unprotected sections then face the residual y - A beta_known
    at L_unprotected / L of the rate.  Errors are counted with the final pass's
    section words for the unprotected sections and the same BP output for the
    protected bits.  Flat, power-allocated and spatially coupled designs.  Same
    methods, device buffers and counter layout as ConcatPipeline, so
    montecarlo.ConcatTrial takes it unchanged."""

    def __init__(self, *args, final_t_max=None, **kw):
        super().__init__(*args, **kw)
        self.final_t_max = self.t_max if final_t_max is None else int(final_t_max)

    def _ensure(self, B):
        if B <= self._cap:
            return
        super()._ensure(B)
        self.d_known = _native.DeviceBuffer(B * self.L * 4)  # known section words; their (location, symbol)
        self.d_kidx = _native.DeviceBuffer(B * self.L * 4)
        self.d_ksym = _native.DeviceBuffer(B * self.L * 4)

    def _final_pass(self):
        lib, B = _native.lib(), self.B
        self._known_sections()
        _native.check(lib.sg_psk_unpack_sections_device(self.d_known.ptr, B, self.L, self.logK, self.d_kidx.ptr,
                                                        self.d_ksym.ptr, None))
        _native.check(lib.sg_camp_decode_partial_device(self.plan, self.d_y.ptr, B, self.K, _native.ptr(self.constel),
                                                        self.d_kidx.ptr, self.d_ksym.ptr, None, None, self.awgn_var,
                                                        self.final_t_max, self.rtol, self.phi_method, self.d_midx.ptr,
                                                        self.d_msym.ptr, None, None, None, None))
        self._pack_map()
