"""Monte-Carlo error-rate campaigns sharded over GPUs.

The reference parallelises only by launching independent processes with a
`sim_id` (ldpc_jossy/py/ldpc_awgn.py:125-131, ldpc_jossy/README.md:144-148).
Here one process per GPU runs a campaign together: every SNR point is split
into fixed blocks of codewords, block b being seeded by (seed, point, b) so
that the result does not depend on how many GPUs took part; each round the
blocks are dealt to ranks by contiguous ranges, and ONE all-reduce of an int64
counter vector (RCCL over xGMI between GPUs, or the host rendezvous group of
rendezvous.py for CPU tests) gives every
rank the global counts that drive the stopping rule.

Counters per point: [units, bit_errors, frame_errors, aux0, aux1] where aux
is decoder-specific (BP: executed iterations; AMP: section errors, AMP
iterations; concatenated: unprotected / protected bit errors).  A trial may
declare a longer vector with an `nc` attribute (CSparcTrial: 7).

Checkpoint/resume: with `checkpoint_dir`, the global counters
and next block of every point are written after each round; a restarted
campaign continues from there.
"""
import json
import os

import numpy as np

from . import _native

NC = 5


def shard_range(total, rank, world):
    """[start, end) of rank's share of `total` items (contiguous, balanced)."""
    return total * rank // world, total * (rank + 1) // world


class Aggregator:
    """Sum of int64 counter vectors over the ranks of a campaign: RCCL between
    GPUs (`comm`, a `_native.Comm`), or the host rendezvous group for CPU
    rehearsals (`group`, a `rendezvous.HostGroup`)."""

    def __init__(self, backend="none", comm=None, group=None):
        if backend not in ("none", "host", "rccl"):
            raise ValueError(f"Aggregator backend {backend!r}: one of none, host, rccl")
        if backend == "host" and group is None:
            raise ValueError("the host backend needs a rendezvous group")
        if backend == "rccl" and comm is None:
            raise ValueError("the rccl backend needs a communicator (_native.Comm)")
        self.backend = backend
        self.comm = comm
        self.group = group
        self._dbuf = None

    def allreduce(self, counts):
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        if self.backend == "none":
            return counts.copy()
        if self.backend == "host":
            return self.group.allreduce_sum_i64(counts)
        if self._dbuf is None or self._dbuf.nbytes < counts.nbytes:
            self._dbuf = _native.DeviceBuffer(counts.nbytes)
        self._dbuf.upload(counts)
        self.comm.allreduce_sum_i64(self._dbuf, counts.size)
        _native.synchronize()
        return self._dbuf.download(np.empty_like(counts))


def _ckpt_path(checkpoint_dir, tag, point):
    return os.path.join(checkpoint_dir, f"{tag}_pt{point}.json")


def _first_reaching(cum, need):
    """Index of the first entry of the running count `cum` that reaches
    `need`, or None."""
    hit = np.nonzero(cum >= need)[0]
    return int(hit[0]) if hit.size else None


# Campaign parameters added to the checkpoints after round 3, with the value
# an older checkpoint implies: such a checkpoint still resumes when the new
# run uses that value (concat_ber_sweep's min_errors None).
_LEGACY_PARAM_DEFAULTS = {"min_errors": None}


def run_point(trial, point, *, block, blocks_per_round, rank, world, agg, min_errors=None, max_units=None,
              checkpoint_dir=None, tag="campaign", params=None, max_rounds=None):
    """Run one point until `min_errors` frame errors or `max_units` units
    (globally).  trial(point, first_block, n_blocks, block) -> int64[NC]
    counters of the blocks [first_block, first_block + n_blocks); a trial
    with an `nc` attribute returns that many counters instead of NC, the first
    three with the same meaning.

    A trial with `per_unit = True` returns int64[n_blocks * block, NC] (one
    row per codeword, in block order) instead; the round's rows of every rank
    are then combined by the same single all-reduce (each rank fills its own
    rows of a zero matrix), and the point stops exactly at the codeword where
    the frame-error count reaches `min_errors` or the unit count reaches
    `max_units`, in block order -- the stopping rule of ldpc_awgn.sim
    (ldpc_awgn.py:86-105), whatever the number of ranks.

    `params` (campaign parameters) is stored in the checkpoint; resuming with
    different parameters raises ValueError instead of adding up counts of
    different experiments.  `max_rounds` ends this call after that many rounds
    without marking the point done (an interrupted run; the checkpoint lets a
    later call continue it)."""
    nc = int(getattr(trial, "nc", NC))
    total = np.zeros(nc, dtype=np.int64)
    next_block = 0
    done = False
    params = dict(params or {}, block=int(block))
    if checkpoint_dir:
        path = _ckpt_path(checkpoint_dir, tag, point)
        if os.path.exists(path):
            with open(path) as f:
                st = json.load(f)
            want = json.loads(json.dumps(params))
            for k, v in _LEGACY_PARAM_DEFAULTS.items():  # checkpoints written before the key existed
                if k not in st.get("params", {}) and want.get(k, v) == v:
                    want.pop(k, None)
            if st.get("params") != want:
                raise ValueError(f"checkpoint {path} was written with parameters {st.get('params')}, "
                                 f"not {params}: use another checkpoint_dir or tag")
            total = np.array(st["counts"], dtype=np.int64)
            next_block = int(st["next_block"])
            done = bool(st.get("done", False))
    per_unit = getattr(trial, "per_unit", False)
    rounds = 0
    while not done:
        if max_rounds is not None and rounds >= max_rounds:
            break
        rounds += 1
        if min_errors is not None and total[2] >= min_errors:
            break
        if max_units is not None and total[0] >= max_units:
            break
        nb = blocks_per_round
        if max_units is not None:
            nb = min(nb, -(-(max_units - int(total[0])) // block))
        a, b = shard_range(nb, rank, world)
        if per_unit:
            rows = np.zeros((nb * block, nc), dtype=np.int64)
            if b > a:
                rows[a * block:b * block] = trial(point, next_block + a, b - a, block)
            rows = agg.allreduce(rows.ravel()).reshape(nb * block, nc)  # the one collective per round
            cut = len(rows)
            if min_errors is not None:
                k = _first_reaching(total[2] + np.cumsum(rows[:, 2]), min_errors)
                if k is not None:
                    cut, done = min(cut, k + 1), True
            if max_units is not None and total[0] + cut >= max_units:
                cut, done = max_units - int(total[0]), True
            total = total + rows[:cut].sum(axis=0)
        else:
            local = trial(point, next_block + a, b - a, block) if b > a else np.zeros(nc, dtype=np.int64)
            total = total + agg.allreduce(local)  # the campaign's one collective per round
        next_block += nb
        if checkpoint_dir and rank == 0:
            os.makedirs(checkpoint_dir, exist_ok=True)
            tmp = _ckpt_path(checkpoint_dir, tag, point) + ".tmp"
            with open(tmp, "w") as f:
                json.dump({"counts": total.tolist(), "next_block": next_block, "done": done,
                           "params": params}, f)
            os.replace(tmp, _ckpt_path(checkpoint_dir, tag, point))
        if min_errors is None and max_units is None:
            break
    return total


# ------------------------------------------------------------------ LDPC over BPSK/AWGN


class LdpcTrial:
    """Random codewords over BPSK/AWGN at Es/N0 = snr dB (ldpc_awgn.py:39-56),
    decoded in batches on the GPU; counts over all N bits as the reference
    does (ldpc_awgn.py:97-104).  aux0 = sum of decode iteration counts."""

    def __init__(self, c, snrs, dectype="sumprod2", max_it=200, corr=0.7, precision="f32", seed=0, rng="host",
                 per_unit=False, schedule="flooding"):
        from .ldpc import _check_schedule
        self.c, self.snrs, self.dectype = c, list(snrs), dectype
        self.schedule = _check_schedule(schedule)  # 'layered': layers of c.z checks (ldpc.code.decode_batch)
        self.per_unit = bool(per_unit)  # per-codeword counter rows (exact stopping rule, run_point)
        self.max_it, self.corr, self.seed = int(max_it), float(corr), int(seed)
        self.prec = {"f64": _native.SG_F64, "f32": _native.SG_F32}[precision]
        if rng not in ("host", "device"):
            raise ValueError("rng must be 'host' (numpy, reproducible against the reference's generators) "
                             "or 'device' (Philox on the GPU, throughput mode)")
        self.rng = rng

    def _device_batch(self, point, first_block, n_blocks, block, sigma2):
        """Information bits, encoding, BPSK and noise on the GPU; Philox stream
        (point, block) so the draw does not depend on the rank or the batching."""
        c, lib, off = self.c, _native.lib(), _native.offset
        B = n_blocks * block
        es = 8 if self.prec == _native.SG_F64 else 4
        d_info = _native.DeviceBuffer(B * c.K)
        d_x = _native.DeviceBuffer(B * c.N)
        d_ch = _native.DeviceBuffer(B * c.N * es)
        for i, blk in enumerate(range(first_block, first_block + n_blocks)):
            sid = (int(point) << 32) | int(blk)
            o = i * block
            _native.check(lib.sg_rng_bits_device(self.seed, sid, block, c.K, off(d_info.ptr, o * c.K), None))
            c.encode_device(off(d_info.ptr, o * c.K), block, off(d_x.ptr, o * c.N))
            _native.check(lib.sg_bpsk_awgn_llr_device(self.prec, self.seed, sid, off(d_x.ptr, o * c.N), block, c.N,
                                                      sigma2, off(d_ch.ptr, o * c.N * es), None))
        return d_x, d_ch, B

    def __call__(self, point, first_block, n_blocks, block):
        c = self.c
        sigma2 = 1.0 / np.power(10, self.snrs[point] / 10.0)
        if self.rng == "device":
            d_x, d_ch, B = self._device_batch(point, first_block, n_blocks, block, sigma2)
            return self._decode_count(d_x, d_ch, B)
        X, LLR = [], []
        for blk in range(first_block, first_block + n_blocks):
            rng = np.random.default_rng([self.seed, point, blk])
            x = c.encode_batch(rng.integers(0, 2, (block, c.K)))
            y = (1.0 - 2.0 * x) + np.sqrt(sigma2) * rng.standard_normal(x.shape)
            X.append(x)
            LLR.append(2.0 / sigma2 * y)
        X = np.concatenate(X)
        LLR = np.concatenate(LLR)
        B = X.shape[0]
        dt = np.float64 if self.prec == _native.SG_F64 else np.float32
        d_ch = _native.DeviceBuffer.from_array(LLR.astype(dt))
        d_x = _native.DeviceBuffer.from_array(X.astype(np.uint8))
        return self._decode_count(d_x, d_ch, B)

    def _decode_count(self, d_x, d_ch, B):
        c, lib = self.c, _native.lib()
        dt = np.float64 if self.prec == _native.SG_F64 else np.float32
        g = c._device_graph()
        d_app = _native.DeviceBuffer(B * c.N * np.dtype(dt).itemsize)
        d_it = _native.DeviceBuffer(B * 4)
        if self.schedule == "layered":
            _native.check(lib.sg_ldpc_decode_layered_device(g, _native.DECTYPES[self.dectype], self.prec, int(c.z),
                                                            d_ch.ptr, B, self.max_it, self.corr, d_app.ptr, d_it.ptr,
                                                            None))
        else:
            _native.check(lib.sg_ldpc_decode_device(g, _native.DECTYPES[self.dectype], self.prec, d_ch.ptr, B,
                                                    self.max_it, self.corr, d_app.ptr, d_it.ptr, None))
        if self.per_unit:  # one row per codeword: [1, bit errors, frame error, iterations, 0]
            d_be = _native.DeviceBuffer(B * 4)
            _native.check(lib.sg_ldpc_codeword_errors_device(g, self.prec, d_app.ptr, d_x.ptr, B, d_be.ptr, None))
            _native.synchronize()
            be = d_be.download(np.zeros(B, np.int32)).astype(np.int64)
            it = d_it.download(np.zeros(B, np.int32)).astype(np.int64)
            return np.stack([np.ones(B, np.int64), be, (be > 0).astype(np.int64), it, np.zeros(B, np.int64)], 1)
        d_cnt = _native.DeviceBuffer(32)
        d_cnt.zero()
        _native.check(lib.sg_ldpc_count_errors_device(g, self.prec, d_app.ptr, d_x.ptr, d_it.ptr, B, c.K,
                                                      d_cnt.ptr, None))
        _native.synchronize()
        cnt = d_cnt.download(np.zeros(4, np.int64))
        return np.array([B, cnt[0], cnt[1], cnt[3], 0], dtype=np.int64)


class SparcTrial:
    """Regular SPARC with the sub-sampled DCT design over AWGN, generated and
    decoded on the GPU (throughput mode): Philox bits ->
    section indices -> x = A beta0 (sparc.py:17-53) -> y = x + N(0, awgn_var)
    (sparc_sim.py:179-204) -> AMP (sparc.py:883-999) -> errors.  Counters
    [codewords, bit errors, codeword errors, AMP iterations, section errors];
    the Philox stream of block b at point p is (p, b), so results do not
    depend on the rank count.  op: sparc.DesignOperator (shared design).

    K = 2: the real BPSK-modulated SPARC on the same design (csrc/amp_oploop.hip,
    the staged path): log2 M + 1 bits per section, the section word
    (location << 1) | symbol in the place of the index, so a section error is
    a wrong location or a wrong sign."""

    def __init__(self, op, awgn_vars, t_max=25, rtol=1e-6, phi_method=1, precision="f32", seed=0, K=1):
        if K not in (1, 2):
            raise ValueError("SparcTrial: K must be 1 (unmodulated) or 2 (BPSK modulated)")
        self.K = int(K)
        self.op, self.vars = op, list(awgn_vars)
        self.t_max, self.rtol, self.phi = int(t_max), float(rtol), int(phi_method)
        self.prec = {"f64": _native.SG_F64, "f32": _native.SG_F32}[precision]
        self.seed = int(seed)
        self.logM = int(np.log2(op.M)) + (1 if self.K == 2 else 0)  # bits per section

    def __call__(self, point, first_block, n_blocks, block):
        op, lib, off = self.op, _native.lib(), _native.offset
        L, n, logM = op.L, op.n, self.logM
        encode, decode = ((lib.sg_amp_encode_device, lib.sg_amp_decode_device) if self.K == 1 else
                          (lib.sg_amp_encode_bpsk_device, lib.sg_amp_decode_bpsk_device))
        es = 8 if self.prec == _native.SG_F64 else 4
        B = n_blocks * block
        plan = op.plan(self.prec)
        d_bits = _native.DeviceBuffer(B * L * logM)
        d_true = _native.DeviceBuffer(B * L * 4)
        d_x = _native.DeviceBuffer(B * n * es)
        d_y = _native.DeviceBuffer(B * n * es)
        sigma = float(np.sqrt(self.vars[point]))
        for i, blk in enumerate(range(first_block, first_block + n_blocks)):
            sid = (int(point) << 32) | int(blk)
            o = i * block
            _native.check(lib.sg_rng_bits_device(self.seed, sid, block, L * logM, off(d_bits.ptr, o * L * logM), None))
        _native.check(lib.sg_bits_to_sections_device(d_bits.ptr, B, L, logM, d_true.ptr, None))
        _native.check(encode(plan, d_true.ptr, B, d_x.ptr, None))
        for i, blk in enumerate(range(first_block, first_block + n_blocks)):
            sid = (int(point) << 32) | int(blk)
            o = i * block
            _native.check(lib.sg_awgn_device(self.prec, self.seed, sid, off(d_x.ptr, o * n * es), block, n, sigma,
                                             off(d_y.ptr, o * n * es), None))
        d_map = _native.DeviceBuffer(B * L * 4)
        d_tf = _native.DeviceBuffer(B * 4)
        d_cnt = _native.DeviceBuffer(4 * 8)
        d_cnt.zero()
        _native.check(decode(plan, d_y.ptr, B, d_true.ptr, float(self.vars[point]), self.t_max, self.rtol, self.phi,
                             d_map.ptr, d_tf.ptr, None, None, None))
        _native.check(lib.sg_amp_count_errors_device(d_map.ptr, d_true.ptr, d_tf.ptr, B, L, logM, d_cnt.ptr, None))
        cnt = d_cnt.download(np.zeros(4, np.int64))
        return np.array([B, cnt[1], cnt[2], cnt[3], cnt[0]], dtype=np.int64)


class CSparcTrial:
    """Complex SPARC with the sub-sampled FFT design, unmodulated (K = 1) or
    K-PSK modulated (K up to 64), over complex AWGN, generated and decoded on
    the GPU in double precision: Philox bits -> (location, constellation
    index) per section (sparc.py:330-364) -> x = A beta0 -> y = x + CN(0,
    awgn_var) (sparc_sim.py:179-204, complex branch) -> AMP (sparc.py:883-999)
    -> the error counts of calc_ber / calc_ler_ver.  Nothing crosses to the
    host between the generation and the counters.

    Counters (nc = 7): [codewords, bit errors, codeword errors, AMP
    iterations, section errors, location errors, value errors]; with
    `per_unit` one such row per codeword, in block order (run_point).  Block b
    of point p draws its bits and its noise from the Philox stream
    (p << 32) | b, one call per block, so results depend neither on the rank
    count nor on how blocks are batched.

    op: sparc.ComplexDesignOperator.  ONE design is shared by the whole
    campaign, as in SparcTrial; sparc_sim instead draws a new design from
    every seed, so a campaign estimates the error rate of a fixed design and
    sparc_sim runs average over designs too."""

    nc = 7

    def __init__(self, op, K, awgn_vars, t_max=25, rtol=1e-6, phi_method=1, seed=0, per_unit=False):
        from .sparc import _check_psk, _interleaved, psk_constel
        if not getattr(op, "csparc", False):
            raise ValueError("CSparcTrial needs a sparc.ComplexDesignOperator")
        self.op, self.K, self.vars = op, int(K), list(awgn_vars)
        _check_psk(self.K)
        self.t_max, self.rtol, self.phi = int(t_max), float(rtol), int(phi_method)
        self.seed, self.per_unit = int(seed), bool(per_unit)
        self.logM = int(round(np.log2(op.M)))
        self.logK = int(round(np.log2(self.K)))
        self.bits_per_codeword = op.L * (self.logM + self.logK)
        self.constel = _interleaved(psk_constel(self.K)) if self.K != 1 else None

    def generate(self, point, first_block, n_blocks, block):
        """Device buffers (d_true_idx int32 [B, L], d_true_sym int32 [B, L],
        d_y complex [B, n]) of the blocks [first_block, first_block + n_blocks),
        B = n_blocks * block."""
        op, lib, off = self.op, _native.lib(), _native.offset
        L, n, nbits = op.L, op.n, self.bits_per_codeword
        B = n_blocks * block
        plan = op.plan()
        d_bits = _native.DeviceBuffer(B * nbits)
        d_idx = _native.DeviceBuffer(B * L * 4)
        d_sym = _native.DeviceBuffer(B * L * 4)
        d_x = _native.DeviceBuffer(B * n * 16)
        d_y = _native.DeviceBuffer(B * n * 16)
        sids = [(int(point) << 32) | int(blk) for blk in range(first_block, first_block + n_blocks)]
        for i, sid in enumerate(sids):
            _native.check(lib.sg_rng_bits_device(self.seed, sid, block, nbits, off(d_bits.ptr, i * block * nbits), None))
        _native.check(lib.sg_bits_to_psk_sections_device(d_bits.ptr, B, L, self.logM, self.logK, d_idx.ptr, d_sym.ptr,
                                                         None))
        _native.check(lib.sg_camp_encode_device(plan, self.K, _native.ptr(self.constel), d_idx.ptr, d_sym.ptr, B,
                                                d_x.ptr, None))
        sigma = float(np.sqrt(self.vars[point] / 2))  # per real dimension
        for i, sid in enumerate(sids):
            o = i * block * n * 16
            _native.check(lib.sg_awgn_device(_native.SG_F64, self.seed, sid, off(d_x.ptr, o), block, 2 * n, sigma,
                                             off(d_y.ptr, o), None))
        return d_idx, d_sym, d_y

    def __call__(self, point, first_block, n_blocks, block):
        op, lib = self.op, _native.lib()
        L, B = op.L, n_blocks * block
        d_idx, d_sym, d_y = self.generate(point, first_block, n_blocks, block)
        d_map = _native.DeviceBuffer(B * L * 4)
        d_msym = _native.DeviceBuffer(B * L * 4)
        d_tf = _native.DeviceBuffer(B * 4)
        d_cnt = _native.DeviceBuffer(6 * 8)
        d_cnt.zero()
        d_rows = _native.DeviceBuffer(B * 4 * 4) if self.per_unit else None
        _native.check(lib.sg_camp_decode_device(op.plan(), d_y.ptr, B, self.K, _native.ptr(self.constel), d_idx.ptr,
                                                d_sym.ptr, float(self.vars[point]), self.t_max, self.rtol, self.phi,
                                                d_map.ptr, d_msym.ptr, d_tf.ptr, None, None, None))
        _native.check(lib.sg_camp_count_errors_device(d_map.ptr, d_msym.ptr, d_idx.ptr, d_sym.ptr, d_tf.ptr, B, L,
                                                      self.logM, self.logK, d_cnt.ptr,
                                                      d_rows.ptr if d_rows else None, None))
        if self.per_unit:  # one row per codeword
            r = d_rows.download(np.zeros((B, 4), np.int32)).astype(np.int64)
            tf = d_tf.download(np.zeros(B, np.int32)).astype(np.int64)
            return np.stack([np.ones(B, np.int64), r[:, 0], (r[:, 0] > 0).astype(np.int64), tf, r[:, 1], r[:, 2],
                             r[:, 3]], 1)
        cnt = d_cnt.download(np.zeros(6, np.int64))
        return np.array([B, cnt[3], cnt[4], cnt[5], cnt[0], cnt[1], cnt[2]], dtype=np.int64)


def csparc_ser_sweep(code_params, decode_params, awgn_vars, *, codewords, block=256, blocks_per_round=None, rank=0,
                     world=1, agg=None, design_seed=0, seed=0, min_errors=None, checkpoint_dir=None, max_rounds=None):
    """Error rates of a complex (K-PSK) SPARC against the noise variance:
    `codewords` per point of `awgn_vars`, sharded over the ranks, every point
    a run_point over CSparcTrial.  The design is built once, from
    `design_seed` (check_code_params, create_base_matrix at awgn_vars[0] --
    only a power allocation depends on the variance -- and
    sparc_transforms(..., csparc=True)), and shared by every point.  Returns
    one dict per point: awgn_var, codewords, ber (over L log2(K M) bits per
    codeword), cer, ser / ler / ver (section, location and value error rates
    over L sections per codeword; K = 1: ler = ser, ver = 0), t_final_mean and
    the raw `counts` (CSparcTrial's seven)."""
    from . import sparc
    cp, dp = dict(code_params), dict(decode_params)
    sparc.check_code_params(cp)
    sparc.check_decode_params(dp)
    if not cp['complex']:
        raise ValueError("csparc_ser_sweep runs complex SPARCs: code_params['complex'] must be True")
    if sparc._precision(dp) != _native.SG_F64:
        raise NotImplementedError("complex SPARCs run in double precision only ('precision': 'f64')")
    awgn_vars = [float(v) for v in awgn_vars]
    R, L, M = cp['R'], cp['L'], cp['M']
    K = cp['K'] if cp['modulated'] else 1
    sparc._check_psk(K)
    tmp = cp.copy()
    tmp.update({'awgn_var': awgn_vars[0]})
    W = sparc.create_base_matrix(**tmp)
    bit_len = int(round(L * np.log2(K * M)))
    n = int(round(bit_len / R))  # as sparc_encode (sparc.py:36-41)
    if W.ndim == 2:
        n = int(round(n / W.shape[0])) * W.shape[0]
    Ab, Az = sparc.sparc_transforms(W, L, M, n, design_seed, True)
    op = sparc.operator_of(Ab, Az)
    trial = CSparcTrial(op, K, awgn_vars, dp['t_max'], dp['rtol'], dp['phi_est_method'], seed)
    agg = agg or Aggregator()
    bpr = blocks_per_round or max(1, world)
    out = []
    for point, var in enumerate(awgn_vars):
        params = {"code_params": {k: cp[k] for k in sorted(cp)}, "awgn_var": var, "design_awgn_var": awgn_vars[0],
                  "t_max": dp['t_max'], "rtol": dp['rtol'], "phi_est_method": dp['phi_est_method'], "seed": seed,
                  "design_seed": design_seed, "codewords": codewords, "min_errors": min_errors}
        if min_errors is not None:  # the counters stop at round granularity (concat_ber_sweep)
            params["blocks_per_round"] = bpr
        tot = run_point(trial, point, block=block, blocks_per_round=bpr, rank=rank, world=world, agg=agg,
                        min_errors=min_errors, max_units=codewords, checkpoint_dir=checkpoint_dir,
                        tag=f"csparc_L{L}_M{M}_K{K}_n{n}", params=params, max_rounds=max_rounds)
        cw = int(tot[0])
        rate = (lambda c, per: float(c) / (cw * per)) if cw else (lambda c, per: None)
        out.append({"awgn_var": var, "codewords": cw, "ber": rate(tot[1], bit_len), "cer": rate(tot[2], 1),
                    "ser": rate(tot[4], L), "ler": rate(tot[5], L), "ver": rate(tot[6], L),
                    "t_final_mean": rate(tot[3], 1), "counts": [int(c) for c in tot]})
    return out


class ConcatTrial:
    """Concatenated SPARC + LDPC codewords (sparc_sim_new.sparc_ldpc_sim,
    sparc_new.py:15-82) at the points' AWGN variances,
    generated and decoded in batches by pipeline.ConcatPipeline (dense AMP ->
    glue -> batched BP -> device counters).  Block b of point p draws its user
    bits and noise from Philox keyed (seed, p << 32 | b) on the GPU (rng
    "device", with the LDPC encoder on the GPU too) or from
    default_rng([seed, p, b]) on the host (rng "host"), so results do not
    depend on the rank count.  Counters [codewords, user-bit errors, codeword errors,
    unprotected-bit errors, protected-bit errors]; per-block BERs of this
    rank are kept in block_ber[point].  With `granule` (a divisor of the
    block) a block is drawn and decoded as block / granule batches of that
    many codewords, batch g of the point keyed like block g above: the
    counters then do not depend on the block size either."""

    def __init__(self, pipe, awgn_vars, seed=0, rng="device", granule=None):
        self.pipe, self.vars, self.seed = pipe, list(awgn_vars), int(seed)
        self.granule = None if granule is None else int(granule)
        # bits of a section: log2 M, plus log2 K on a K-PSK pipeline (pipeline.CsparcConcatPipeline)
        self.user_bits = pipe.L_unp * getattr(pipe, "bits_per_section", pipe.logM) + pipe.mults * pipe.c.K
        self.block_ber = {}
        if rng not in ("host", "device"):
            raise ValueError("rng must be 'host' (numpy default_rng([seed, point, block])) or 'device' (Philox)")
        self.rng = rng

    def __call__(self, point, first_block, n_blocks, block):
        tot = np.zeros(NC, dtype=np.int64)
        size = self.granule or block
        if size <= 0 or block % size:
            raise ValueError(f"granule {size} must divide the block of {block} codewords")
        per = block // size
        for b in range(first_block, first_block + n_blocks):
            c = np.zeros(NC, dtype=np.int64)
            for g in range(b * per, (b + 1) * per):  # (no granule: the block itself, g = b)
                if self.rng == "device":  # throughput mode: no host encode or host RNG in the loop
                    self.pipe.make_batch_device(size, self.vars[point], self.seed, (int(point) << 32) | int(g))
                else:
                    self.pipe.make_batch(size, self.vars[point], np.random.default_rng([self.seed, int(point), int(g)]))
                self.pipe.reset_counts()
                self.pipe.decode()
                c += self.pipe.counts()
            tot += c
            self.block_ber.setdefault(point, []).append(float(c[1]) / (c[0] * self.user_bits))
        return tot


def concat_checkpoint_tag(L, M, n, design="dense", K=1):
    """Checkpoint tag of a concat_ber_sweep: concat_L.. (dense), concat_dct_L.. (DCT design),
    concat_dct3_L.. (DCT design with the final AMP pass, design "dct3"),
    concat_fft_L.._M.._K.. (complex FFT design with K-PSK; K = 1 unmodulated),
    concat_fft3_L.._M.._K.. (the same with the final AMP pass, design "fft3"),
    concat_dct_k2_L.. (DCT design with real K = 2 modulated sections, design "dct_k2")."""
    if design in ("fft", "fft3"):
        return f"concat_{design}_L{L}_M{M}_K{K}_n{n}"
    return f"concat_L{L}_M{M}_n{n}" if design == "dense" else f"concat_{design}_L{L}_M{M}_n{n}"


def concat_ber_sweep(L, M, n, P, L_unprotected, mults, ebn0_db, *, codewords, block=256, blocks_per_round=None,
                     rank=0, world=1, agg=None, design_seed=0, seed=0, t_max=25, bp_its=200, precision="f32",
                     ldpc=("802.11n", "1/2", 81), min_errors=None, checkpoint_dir=None, npz_file=None, rng="device",
                     trial=None, max_rounds=None, on_point=None, design="dense", K=1, granule=None, final_amp=False,
                     final_t_max=None):
    """BER / FER of concatenated SPARC + LDPC against Eb/N0 (the experiment of
    ldpc_sparc/performance_plots_general.py:100-138 for the plain concatenated
    decoder), `codewords` per point sharded over the ranks.  Eb/N0 to noise as
    the bench: awgn_var = P / (2 R_overall 10^(Eb/N0 / 10)), R_overall = user
    bits / n.  Returns one dict per point; rank 0 writes `npz_file` in the
    layout of performance_plots_general.py:138 (ber_store_averages, _max,
    _min over the blocks rank 0 decoded, and snr_store = Eb/N0 in dB), plus a
    `complete` flag per point; a sweep that `max_rounds` interrupted writes
    `<npz_file>.partial.npz` instead, so it never overwrites a final file.
    `trial(point, first_block, n_blocks, block)` (counters as ConcatTrial's)
    replaces the GPU pipeline (CPU rehearsals: tools/c5_sweep.py --rehearsal); `max_rounds`
    interrupts every point after that many rounds (run_point); `on_point(dict)`
    is called with each point's result as soon as it is done.  `design`:
    "dense" is the reference's Gaussian matrix (pipeline.ConcatPipeline), "dct"
    the sub-sampled DCT design drawn from `design_seed`, decoded by the public
    AMP with early stopping (pipeline.DctConcatPipeline).  A DCT sweep keeps
    its checkpoints under its own tag and parameters, so neither kind resumes
    the other.  "fft" is the complex sub-sampled FFT design with K-PSK
    modulated sections (`K` = 1: unmodulated; pipeline.CsparcConcatPipeline,
    double precision only: precision="f32" raises NotImplementedError): a
    section carries log2 M + log2 K bits, and the n channel uses are complex.
    For complex noise of variance awgn_var per sample N0 = awgn_var, so there
    Eb/N0 = P / (R_overall awgn_var), awgn_var = P / (R_overall 10^(Eb/N0 / 10))
    with R_overall = user bits / n; the real sweeps keep their factor 2
    (N0 = 2 awgn_var).  Its checkpoints carry the design name and K in tag and
    parameters, so a resumed real or dense sweep never reads them.  `granule`
    (ConcatTrial) fixes the size of the batches a block is drawn in, which
    makes the counters independent of `block`; it then is part of the
    checkpointed parameters.  `final_amp` (with design="dct" or "fft"; off by
    default) runs the three-stage decoder AMP -> BP -> AMP with the BP-decoded
    sections known (pipeline.DctConcat3Pipeline or CsparcConcat3Pipeline, its
    last pass up to `final_t_max` - 1 iterations, default t_max); its
    checkpoints live under concat_dct3_L.. / concat_fft3_L.._M.._K.. with
    "design": "dct3" / "fft3" and final_t_max in the parameters, so a two-stage
    sweep never resumes them.  design="dct" with K=2 is the real K = 2 (BPSK)
    modulated SPARC on the DCT design (pipeline.DctBpskConcatPipeline, either
    precision): a section carries log2 M + 1 bits, the noise is real (the
    factor 2 stays), and its checkpoints live under concat_dct_k2_L.. with
    "design": "dct_k2" and "K": 2.  Known sections are not built for K = 2,
    so final_amp=True raises ValueError there."""
    from .ldpc import code
    if design not in ("dense", "dct", "fft"):
        raise ValueError(f"design must be 'dense', 'dct' or 'fft', not {design!r}")
    if final_amp and design == "dense":
        raise ValueError("final_amp needs the DCT or FFT design: design='dct' or 'fft'")
    ftm = int(t_max if final_t_max is None else final_t_max)
    K = int(K)
    bpsk = design == "dct" and K == 2  # real K = 2 modulated sections on the DCT design
    if design != "fft" and K != 1 and not bpsk:
        raise ValueError("K-PSK modulation needs the complex design: design='fft' (design='dct' takes K = 1 or the "
                         "real K = 2)")
    if bpsk and final_amp:
        raise ValueError("final_amp with K = 2 on the DCT design: known sections for K = 2 are not built")
    # what names the campaign in checkpoint tag and parameters
    key = "dct_k2" if bpsk else design + "3" if final_amp else design
    agg = agg or Aggregator()
    logM = int(np.log2(M))
    per = logM + (int(round(np.log2(K))) if design == "fft" or bpsk else 0)
    user_bits = L_unprotected * per + mults * code(*ldpc).K
    r_overall = user_bits / n
    if design == "fft":  # complex samples: N0 = awgn_var
        vars_ = [P / (r_overall * 10 ** (e / 10)) for e in ebn0_db]
    else:
        vars_ = [P / (2 * r_overall * 10 ** (e / 10)) for e in ebn0_db]
    if trial is None:
        from .pipeline import (ConcatPipeline, CsparcConcat3Pipeline, CsparcConcatPipeline, DctBpskConcatPipeline,
                               DctConcat3Pipeline, DctConcatPipeline)
        if design == "fft" and final_amp:
            pipe = CsparcConcat3Pipeline(L, M, K, n, P, L_unprotected, mults, ldpc=ldpc, design_seed=design_seed,
                                         precision=precision, t_max=t_max, bp_its=bp_its, final_t_max=ftm)
        elif design == "fft":
            pipe = CsparcConcatPipeline(L, M, K, n, P, L_unprotected, mults, ldpc=ldpc, design_seed=design_seed,
                                        precision=precision, t_max=t_max, bp_its=bp_its)
        elif final_amp:
            pipe = DctConcat3Pipeline(L, M, n, P, L_unprotected, mults, ldpc=ldpc, design_seed=design_seed,
                                      precision=precision, t_max=t_max, bp_its=bp_its, final_t_max=ftm)
        else:
            make = DctBpskConcatPipeline if bpsk else DctConcatPipeline if design == "dct" else ConcatPipeline
            pipe = make(L, M, n, P, L_unprotected, mults, ldpc=ldpc, design_seed=design_seed, precision=precision,
                        t_max=t_max, bp_its=bp_its)
        trial = ConcatTrial(pipe, vars_, seed, rng, granule)
        assert trial.user_bits == user_bits
    bpr = blocks_per_round or max(1, world)
    out = []
    for point, e in enumerate(ebn0_db):
        params = {"P": P, "L_unprotected": L_unprotected, "mults": mults, "ebn0_db": float(e),
                  "seed": seed, "design_seed": design_seed, "t_max": t_max, "bp_its": bp_its,
                  "precision": precision, "ldpc": list(ldpc), "codewords": codewords, "rng": rng,
                  "min_errors": min_errors}
        if min_errors is not None:
            # the counters stop at round granularity, so with an error target
            # the round size is part of the experiment (without one the point
            # ends at `codewords`, a multiple of the block, at any round size)
            params["blocks_per_round"] = bpr
        if design != "dense":  # (dense sweeps keep the parameters their checkpoints were written with)
            params["design"] = key
        if final_amp:
            params["final_t_max"] = ftm
        if design == "fft" or bpsk:
            params["K"] = K
        if granule is not None:
            params["granule"] = int(granule)
        tot = run_point(trial, point, block=block, blocks_per_round=bpr, rank=rank, world=world, agg=agg,
                        min_errors=min_errors, max_units=codewords, checkpoint_dir=checkpoint_dir,
                        tag=concat_checkpoint_tag(L, M, n, key, K), params=params, max_rounds=max_rounds)
        out.append({"ebn0_db": float(e), "awgn_var": vars_[point], "codewords": int(tot[0]),
                    "ber": float(tot[1]) / (tot[0] * user_bits) if tot[0] else None,
                    "fer": float(tot[2]) / tot[0] if tot[0] else None,
                    "unprotected_bit_errors": int(tot[3]), "protected_bit_errors": int(tot[4]),
                    "R_overall": r_overall,
                    # False when max_rounds interrupted the point before its target
                    "complete": bool(tot[0] >= codewords or (min_errors is not None and tot[2] >= min_errors))})
        if on_point is not None:
            on_point(out[-1])
    if npz_file and rank == 0:
        complete = np.array([o["complete"] for o in out])
        if not complete.all():  # an interrupted sweep never overwrites a final file
            npz_file = (npz_file[:-4] if npz_file.endswith(".npz") else npz_file) + ".partial.npz"
        avg = np.array([[o["ber"] for o in out]], dtype=float)
        bb = [getattr(trial, "block_ber", {}).get(p, [np.nan]) for p in range(len(ebn0_db))]
        np.savez(npz_file, ber_store_averages=avg, ber_store_max=np.array([[np.max(b) for b in bb]]),
                 ber_store_min=np.array([[np.min(b) for b in bb]]), snr_store=np.asarray(ebn0_db, dtype=float),
                 complete=complete)
    return out


def ldpc_awgn_campaign(standard, rate, z, ptype="A", *, rank=0, world=1, agg=None, N_MEASUREMENTS=24,
                       C_AWGN_OFFSET=1.0, P_STEP=100.0, MIN_ERRORS=100, MAX_BLOCKS=400000, block=256,
                       blocks_per_round=16, dectype="sumprod2", max_it=200, precision="f32", seed=0,
                       results_file=None, checkpoint_dir=None, trial=None, schedule="flooding"):
    """The BER/FER campaign of ldpc_awgn.sim (ldpc_awgn.py:60-114) on the GPU(s):
    same starting SNR, stopping rule (each point ends at the codeword whose
    frame error is the MIN_ERRORS-th, or at MAX_BLOCKS codewords, counted in
    block order whatever the rank count) and SNR-step heuristic; returns and
    (rank 0) appends the result tuples (standard, rate, z, ptype, SNR, nblocks,
    nblockerrors, nblocks*K, nbiterrors, nit_total) -- the 11-field form that
    results2csv.c parses (results2csv.c:47-48).  `trial` replaces the GPU
    trial (tests).  schedule='layered' decodes on the layered schedule and
    keeps its checkpoints under a tag and parameters of their own, so a
    flooding checkpoint is never resumed as layered or the reverse."""
    from .ldpc import code
    Rv = {"1/2": .5, "2/3": 0.6667, "3/4": 0.75, "5/6": 0.83333}
    if rate not in Rv:
        raise NameError("Rate unsupported")
    agg = agg or Aggregator()
    c = code(standard, rate, z, ptype)
    snr = 10.0 * np.log10(np.power(2, Rv[rate]) - 1.0) + C_AWGN_OFFSET
    res = []
    from .ldpc import _check_schedule
    layered = _check_schedule(schedule) == "layered"
    trial = trial or LdpcTrial(c, [], dectype, max_it, 0.7, precision, seed, per_unit=True, schedule=schedule)
    for point in range(N_MEASUREMENTS):
        trial.snrs.append(snr)
        params = {"seed": seed, "dectype": dectype, "max_it": max_it, "precision": precision, "snr": float(snr),
                  "min_errors": MIN_ERRORS, "max_blocks": MAX_BLOCKS}
        if layered:  # (flooding checkpoints keep the tag and parameters they have always had)
            params["schedule"] = schedule
        tot = run_point(trial, point, block=block, blocks_per_round=blocks_per_round, rank=rank, world=world,
                        agg=agg, min_errors=MIN_ERRORS, max_units=MAX_BLOCKS, checkpoint_dir=checkpoint_dir,
                        tag=f"ldpc_{standard}_{rate.replace('/', '')}_{z}_{ptype}" + ("_layered" if layered else ""),
                        params=params)
        nblocks = int(tot[0])
        out = (standard, rate, z, ptype, snr, nblocks, int(tot[2]), nblocks * c.K, int(tot[1]), int(tot[3]))
        res.append(out)
        if results_file and rank == 0:
            with open(results_file, "a") as f:
                f.write(str(out) + "\n")
        snr += np.sqrt(P_STEP / nblocks)
    return res


def results_to_csv(lines):
    """The conversion of results2csv.c:47-72 (standard code, rate, type, z, SNR,
    nblocks, nblockerrors, nbits, nbiterrors, nit) for result tuples."""
    out = []
    for (std, rate, z, ptype, snr, nb, nbe, nbits, nber, nit) in lines:
        num, den = (int(v) for v in rate.split("/"))
        out.append(f"{'16' if std[5] == '6' else '11'}, {num / den:g}, {0 if ptype == 'A' else 1}, {z}, "
                   f"{snr:g}, {nb}, {nbe}, {nbits}, {nber}, {nit}")
    return out
