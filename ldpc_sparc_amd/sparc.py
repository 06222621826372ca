"""Sparse regression codes (SPARCs) with a GPU AMP decoder.

Drop-in for sparc_public/sparc.py (Kuan Hsieh's SPARC library as vendored in
SophieLangdon27/LDPC_SPARC): same function names, argument meaning, dict
mutation and return values.  The AMP loop (sparc_amp, sparc.py:883-999) and
the design operators returned by sparc_transforms (sparc.py:703-880) run on
the MI355X through libldpc_sparc_amd (include/ldpc_sparc_amd.h); the code
parameter handling, bit <-> message-vector formats, base matrices and the
random orderings are host-side and follow the reference exactly.

Engine knobs (not in the reference, ignored by it): decode_params may carry
'precision' ('f64' default, the reference's arithmetic; 'f32' the throughput
path).

Complex SPARCs (the sub-sampled FFT design, sub_fft sparc.py:593-646) and
K-PSK modulated complex SPARCs (K up to 64) run on the complex engine
(csrc/amp_cfft.hip) in double precision only: 'precision': 'f32' with a
complex design raises NotImplementedError.  Also out of scope, raising
NotImplementedError: K > 64.

Real K=2 (BPSK) modulated SPARCs -- the DCT design with section entries +1 or
-1 -- decode on the GPU in either precision (csrc/amp_oploop.hip, flat,
power-allocated and spatially coupled designs): amp_decode_bpsk_batch, and
montecarlo.SparcTrial(..., K=2) for campaigns.  Through the drop-in functions
(sparc_encode, sparc_amp, sparc_decode, sparc_sim.sparc_sim) the family is
opt-in: they refuse it with NotImplementedError until enable_real_psk() has
been called once, the one line a reference script needs added.
Soft output of the complex engine: ComplexDesignOperator.soft_output() then
camp_llr (bit LLRs of location and K-PSK symbol bits); section_llr_psk is the
stand-alone function.  Monte-Carlo campaigns of complex SPARCs that stay on the GPU are
montecarlo.CSparcTrial / csparc_ser_sweep; state evolution, K-PSK included, is
sparc_se.py.
"""
import ctypes as ct
from copy import copy

import numpy as np

from . import _native

# ------------------------------------------------------------------ helpers


def is_power_of_2(x):
    return (x > 0) and ((x & (x - 1)) == 0)


def _precision(decode_params):
    p = (decode_params or {}).get('precision', 'f64')
    if p not in ('f64', 'f32'):
        raise ValueError("decode_params['precision'] must be 'f64' or 'f32'")
    return _native.SG_F64 if p == 'f64' else _native.SG_F32


# ------------------------------------------------------------------ encode / decode


def sparc_encode(code_params, awgn_var, rand_seed):
    """Bits -> message vector -> codeword x = A beta0 (sparc.py:17-53).
    Mutates code_params (check_code_params, then adds 'n' and 'R_actual')."""
    check_code_params(code_params)
    R, L, M = map(code_params.get, ['R', 'L', 'M'])
    K = code_params['K'] if code_params['modulated'] else 1
    _check_family(K, code_params['complex'])

    bit_len = int(round(L * np.log2(K * M)))
    bits_in = rnd_bin_arr(bit_len, rand_seed)
    beta0 = bin_arr_2_msg_vector(bits_in, M, K)

    tmp = code_params.copy()
    tmp.update({'awgn_var': awgn_var})
    W = create_base_matrix(**tmp)

    n = int(round(bit_len / R))
    if W.ndim == 2:
        Lr, _ = W.shape
        Mr = int(round(n / Lr))
        n = Mr * Lr
    R_actual = bit_len / n
    code_params.update({'n': n, 'R_actual': R_actual})

    Ab, Az = sparc_transforms(W, L, M, n, rand_seed, code_params['complex'])
    x = Ab(beta0)
    return bits_in, beta0, x, Ab, Az


def sparc_decode(y, code_params, decode_params, awgn_var, rand_seed, beta0, Ab=None, Az=None):
    """AMP decode + hard decision + bits (sparc.py:55-74)."""
    check_decode_params(decode_params)
    beta, t_final, nmse, psi = sparc_amp(y, code_params, decode_params, awgn_var, rand_seed, beta0,
                                         Ab, Az)
    expect_err = psi.mean() >= 0.001
    K = code_params['K'] if code_params['modulated'] else 1
    bits_out = msg_vector_2_bin_arr(beta, code_params['M'], K)
    return bits_out, beta, t_final, nmse, expect_err


# ------------------------------------------------------------------ parameter checks


def check_code_params(code_params):
    """Validate and rewrite code_params in place (sparc.py:77-149)."""
    out = {}

    def take(keys):
        if all(k in code_params for k in keys):
            for k in keys:
                out[k] = copy(code_params[k])
        else:
            raise Exception('Need code parameters {}.'.format(keys))

    for flag in ('complex', 'modulated', 'power_allocated', 'spatially_coupled'):
        if flag not in code_params:
            code_params[flag] = False
        else:
            assert type(code_params[flag]) == bool, "'{}' must be boolean".format(flag)
        out[flag] = copy(code_params[flag])

    take(['P', 'R', 'L', 'M'])
    P, R, L, M = map(code_params.get, ['P', 'R', 'L', 'M'])
    assert (type(P) == float or type(P) == np.float64) and P > 0
    assert (type(R) == float or type(R) == np.float64) and R > 0
    assert type(L) == int and L > 0
    assert type(M) == int and M > 0 and is_power_of_2(M)

    if code_params['modulated']:
        take(['K'])
        K = code_params['K']
        assert type(K) == int and K > 1 and is_power_of_2(K)
        if not code_params['complex']:
            assert K == 2, 'Real-modulated SPARCs requires K=2'

    if code_params['power_allocated']:
        take(['B', 'R_PA_ratio'])
        B, R_PA_ratio = map(code_params.get, ['B', 'R_PA_ratio'])
        assert type(B) == int and B > 1
        assert L % B == 0, 'B must divide L'
        assert type(R_PA_ratio) == float or type(R_PA_ratio) == np.float64
        assert R_PA_ratio >= 0

    if code_params['spatially_coupled']:
        take(['omega', 'Lambda'])
        omega, Lambda = map(code_params.get, ['omega', 'Lambda'])
        assert type(omega) == int and omega > 1
        assert type(Lambda) == int and Lambda >= (2 * omega - 1)
        assert L % Lambda == 0, 'Lambda must divide L'

    if code_params['power_allocated'] and code_params['spatially_coupled']:
        assert L % (Lambda * B) == 0, 'Lambda*B must divide L'

    code_params.clear()
    code_params.update(dict(out))


def check_decode_params(decode_params):
    """Validate decode_params and fill defaults in place (sparc.py:151-170)."""
    if 't_max' not in decode_params:
        raise Exception('Need decode parameters {}.'.format(['t_max']))
    for key, val in {'rtol': 1e-6, 'phi_est_method': 1}.items():
        if key not in decode_params:
            decode_params[key] = val
    t_max, rtol, phi_est_method = map(decode_params.get, ['t_max', 'rtol', 'phi_est_method'])
    assert type(t_max) == int and t_max > 1
    assert type(rtol) == float and 0 < rtol < 1
    assert phi_est_method == 1 or phi_est_method == 2


# ------------------------------------------------------------------ bits and message vectors


def rnd_bin_arr(k, rand_seed):
    """k random bits from RandomState(rand_seed) (sparc.py:174-180)."""
    assert type(k) == int
    return np.random.RandomState(rand_seed).randint(2, size=k, dtype='bool')


def bin_arr_2_int(bin_array):
    """MSB-first bits -> integer (sparc.py:182-189)."""
    assert bin_array.dtype == 'bool'
    k = bin_array.size
    assert 0 < k < 64
    return bin_array.dot(1 << np.arange(k)[::-1])


def int_2_bin_arr(integer, arr_length):
    """Integer -> MSB-first bits of length arr_length (sparc.py:191-197, with the
    numpy-1.26 semantics the reference pins)."""
    assert integer >= 0
    return ((int(integer) >> np.arange(arr_length)[::-1]) & 1).astype(bool)


def _bits_to_indices(bin_arr, logM):
    w = 1 << np.arange(logM)[::-1]
    return bin_arr.reshape(-1, logM).astype(np.int64) @ w


def _indices_to_bits(idx, logM):
    return ((np.asarray(idx, dtype=np.int64)[:, None] >> np.arange(logM)[::-1]) & 1).astype(bool).ravel()


def bin2gray(num):
    """Binary code -> Gray code (sparc.py:206-211)."""
    return num ^ (num >> 1)


def gray2bin(num):
    """Gray code -> binary code (sparc.py:214-223); integers or integer arrays."""
    mask = num >> 1
    while np.any(mask != 0):
        num = num ^ mask
        mask = mask >> 1
    return num


def psk_constel(K):
    """K-PSK constellation (sparc.py:225-239): real for K=2, the exact
    {1, 1j, -1, -1j} for K=4, cos + 1j sin of 2 pi k / K otherwise."""
    assert type(K) == int and K > 1 and is_power_of_2(K)
    if K == 2:
        return np.array([1, -1])
    if K == 4:
        return np.array([1 + 0j, 0 + 1j, -1 + 0j, 0 - 1j])
    theta = 2 * np.pi * np.arange(K) / K
    return np.cos(theta) + 1J * np.sin(theta)


def _psk_indices(bin_arr, logK):
    """Constellation index of every group of logK MSB-first Gray-coded bits."""
    return gray2bin(_bits_to_indices(bin_arr, logK))


def psk_mod(bin_arr, K):
    """Gray-coded K-PSK modulation of L*log2(K) bits (sparc.py:241-269): a
    single symbol (0-d) for one group of bits, else an array of L symbols."""
    assert type(K) == int and K > 1 and is_power_of_2(K)
    assert bin_arr.dtype == 'bool'
    c = psk_constel(K)
    logK = int(round(np.log2(K)))
    assert bin_arr.size % logK == 0
    idx = _psk_indices(bin_arr, logK)
    return c[idx[0]] if idx.size == 1 else c[idx]


def _psk_symbol_indices(symbols, K):
    """Index of each symbol in the K-PSK constellation (exact match, as the
    reference's np.argwhere(c == symbol))."""
    c = psk_constel(K)
    sym = np.asarray(symbols).reshape(-1)
    hit = sym[:, None] == c[None, :]
    if not np.all(hit.any(axis=1)):
        raise IndexError("symbol is not a point of the {}-PSK constellation".format(K))
    return hit.argmax(axis=1)


def psk_demod(symbols, K):
    """Gray-coded K-PSK demodulation (sparc.py:271-299): L symbols -> L*log2(K) bits."""
    assert type(K) == int and K > 1 and is_power_of_2(K)
    logK = int(round(np.log2(K)))
    return _indices_to_bits(bin2gray(_psk_symbol_indices(symbols, K)), logK)


def _sym_values(K, sym_idx):
    """Message-vector values of constellation indices (1 for K=1)."""
    if K == 1:
        return np.ones(np.shape(sym_idx))
    return psk_constel(K)[sym_idx]


def _msg_vector_from_indices(idx, sym_idx, M, K):
    """Message vector with value c[sym_idx[l]] at entry idx[l] of section l:
    real for K in {1, 2}, complex128 otherwise (sparc.py:351-354)."""
    L = len(idx)
    mv = np.zeros((L, M)) if K in (1, 2) else np.zeros((L, M), dtype=complex)
    mv[np.arange(L), idx] = _sym_values(K, sym_idx)
    return mv.ravel()


def _msg_vector_indices(msg_vector, M, K):
    """(locations, constellation indices) of a message vector with exactly one
    nonzero per section."""
    L = msg_vector.size // M
    mr = msg_vector.reshape(L, M)
    rows, cols = np.nonzero(mr)
    assert np.array_equal(rows, np.arange(L))
    if K == 1:
        return cols, np.zeros(L, dtype=np.int64)
    return cols, _psk_symbol_indices(mr[rows, cols], K)


def rnd_msg_vector(L, M, rand_seed, K=1):
    """Random message vector, K-PSK modulated for K>1 (sparc.py:303-328)."""
    rng = np.random.RandomState(rand_seed)
    assert type(M) == int and M > 0 and is_power_of_2(M)
    idxs = rng.randint(0, M, L)
    syms = rng.randint(0, K, L) if K != 1 else np.zeros(L, dtype=np.int64)
    return _msg_vector_from_indices(idxs, syms, M, K)


def _section_bits(bin_arr, M, K):
    """Bits [L, logM + logK] of a bit array: location bits first (sparc.py:339-349)."""
    assert type(M) == int and M > 0 and is_power_of_2(M)
    logM = int(round(np.log2(M)))
    logK = 0
    if K != 1:
        assert type(K) == int and K > 1 and is_power_of_2(K)
        logK = int(round(np.log2(K)))
    assert bin_arr.size % (logM + logK) == 0
    return np.asarray(bin_arr, dtype=bool).reshape(-1, logM + logK), logM, logK


def bin_arr_2_msg_vector(bin_arr, M, K=1):
    """Bits -> message vector (sparc.py:330-364): per section log2 M MSB-first
    location bits, then log2 K Gray-coded K-PSK bits for K>1.  Real for
    K in {1, 2}, complex128 otherwise."""
    sec, logM, logK = _section_bits(bin_arr, M, K)
    L = sec.shape[0]
    idx = _bits_to_indices(np.ascontiguousarray(sec[:, :logM]), logM) if logM else np.zeros(L, dtype=np.int64)
    sym = _psk_indices(np.ascontiguousarray(sec[:, logM:]), logK) if K != 1 else np.zeros(L, dtype=np.int64)
    return _msg_vector_from_indices(idx, sym, M, K)


def msg_vector_2_bin_arr(msg_vector, M, K=1):
    """Message vector -> bits (sparc.py:366-400), the inverse of bin_arr_2_msg_vector."""
    assert type(msg_vector) == np.ndarray
    assert type(M) == int and M > 0 and is_power_of_2(M)
    assert msg_vector.size % M == 0
    logM = int(round(np.log2(M)))
    L = msg_vector.size // M
    if K != 1:
        assert type(K) == int and K > 1 and is_power_of_2(K)
    cols, sym = _msg_vector_indices(msg_vector, M, K)
    bits = _indices_to_bits(cols, logM).reshape(L, logM)
    if K != 1:
        logK = int(round(np.log2(K)))
        bits = np.concatenate([bits, _indices_to_bits(bin2gray(sym), logK).reshape(L, logK)], axis=1)
    return bits.ravel()


MAX_PSK = 64  # largest constellation of the GPU engine


def _check_psk(K):
    if K != 1:
        assert type(K) == int and K > 1 and is_power_of_2(K)
        if K > MAX_PSK:
            raise NotImplementedError("K-PSK with K > {} is not part of the GPU engine".format(MAX_PSK))


_real_psk = False  # enable_real_psk


def enable_real_psk(on=True):
    """Switch the drop-in functions' real K=2 modulated path (sparc_encode,
    sparc_amp, sparc_decode, sparc_sim.sparc_sim) on or off; off is the
    default.  Returns the previous setting; calling it again with the same
    value changes nothing.  amp_decode_bpsk_batch and
    montecarlo.SparcTrial(K=2) need no switch."""
    global _real_psk
    prev, _real_psk = _real_psk, bool(on)
    return prev


def _check_family(K, csparc):
    """Complex designs carry any K up to MAX_PSK; real designs K=1, and K=2
    after enable_real_psk()."""
    _check_psk(K)
    if K != 1 and not csparc:
        assert K == 2, 'Real-modulated SPARCs requires K=2'
        if not _real_psk:
            raise NotImplementedError("real K=2 modulated SPARCs are opt-in for the drop-in functions: call "
                                      "ldpc_sparc_amd.sparc.enable_real_psk() once before (amp_decode_bpsk_batch and "
                                      "montecarlo.SparcTrial(K=2) need no switch)")


def _interleaved(a):
    """complex128 array -> contiguous float64 view [..., 2]."""
    return np.ascontiguousarray(a, dtype=np.complex128).view(np.float64)


def msg_vector_mmse_estimator(s, tau, M, K=1):
    """MMSE estimate of the message vector from s = beta + sqrt(tau) noise
    (sparc.py:402-465), evaluated on the GPU in double precision with a
    per-section maximum (the reference's global maximum in float128 is the
    same function).  K=1: softmax; K>1: the K-PSK estimators.  Real output for
    K in {1, 2}, complex otherwise.  For complex s the noise variance per real
    dimension is tau/2; unlike the reference (sparc.py:417-418, `tau /= 2` on
    the caller's array) the caller's tau is left unchanged."""
    assert type(s) == np.ndarray
    assert s.size % M == 0
    _check_psk(K)
    if K != 1 or np.iscomplexobj(s):
        _native.require_gpu()
        cplx = np.iscomplexobj(s)
        t = np.asarray(tau, dtype=np.float64) / 2 if cplx else np.asarray(tau, dtype=np.float64)
        if K <= 2 or not cplx:
            x = np.ascontiguousarray(s.real / t, dtype=np.float64)
            xc = 0
        else:
            x = _interleaved(s.real / t + 1j * (s.imag / t))
            xc = 1
        out = np.empty(s.size, dtype=np.complex128)
        c = _interleaved(psk_constel(K)) if K != 1 else None
        _native.check(_native.lib().sg_section_mmse_psk(_native.ptr(x), s.size // M, M, K, _native.ptr(c), xc,
                                                        _native.ptr(out)))
        return out.real.copy() if K in (1, 2) else out
    _native.require_gpu()
    x = np.ascontiguousarray(s.real / tau, dtype=np.float64)
    out = np.empty_like(x)
    _native.check(_native.lib().sg_section_softmax(_native.ptr(x), x.size // M, M, 1.0,
                                                   _native.ptr(out)))
    return out


def _section_bit_count(M, K):
    return int(round(np.log2(M))) + (int(round(np.log2(K))) if K != 1 else 0)


def section_llr_psk(s, tau, M, K=1, probs_only=False):
    """Soft bits of the message vector behind s = beta + sqrt(tau) noise: per
    section the log2 M MSB-first location bits, then the log2 K Gray-coded
    K-PSK bits (the bit order of msg_vector_2_bin_arr), as the marginals of
    the joint posterior over (location, symbol) that msg_vector_mmse_estimator
    averages.  Returns float64 [L * (log2 M + log2 K)]: the LLRs
    log p - log(1 - p) of p = P(bit = 0) clipped to [1e-15, 1 - 1e-15]
    (ldpc_bp, sparc_new.py:1167-1169), or with probs_only the unclipped p.
    s and tau as msg_vector_mmse_estimator (the caller's tau is left
    unchanged); M a power of two in [2, 2048].  Evaluated on the GPU."""
    assert type(s) == np.ndarray
    assert s.size % M == 0
    _check_psk(K)
    _native.require_gpu()
    cplx = np.iscomplexobj(s)
    t = np.asarray(tau, dtype=np.float64) / 2 if cplx else np.asarray(tau, dtype=np.float64)
    if K <= 2 or not cplx:
        x = np.ascontiguousarray(s.real / t, dtype=np.float64)
        xc = 0
    else:
        x = _interleaved(s.real / t + 1j * (s.imag / t))
        xc = 1
    L = s.size // M
    out = np.empty(L * _section_bit_count(M, K))
    c = _interleaved(psk_constel(K)) if K != 1 else None
    _native.check(_native.lib().sg_section_llr_psk(_native.ptr(x), L, M, K, _native.ptr(c), xc,
                                                   int(bool(probs_only)), _native.ptr(out)))
    return out


def msg_vector_map_estimator(s, M, K=1):
    """MAP estimate per section (sparc.py:467-512) on the GPU: the location
    (and for K>1 the K-PSK symbol) closest to s; first maximum wins."""
    assert type(s) == np.ndarray
    assert s.size % M == 0
    _check_psk(K)
    _native.require_gpu()
    L = s.size // M
    if K != 1:
        cplx = np.iscomplexobj(s)
        sv = _interleaved(s) if cplx else np.ascontiguousarray(s, dtype=np.float64)
        idx = np.empty(L, dtype=np.int32)
        sym = np.empty(L, dtype=np.int32)
        _native.check(_native.lib().sg_section_map_psk(_native.ptr(sv), L, M, K,
                                                       _native.ptr(_interleaved(psk_constel(K))), int(cplx),
                                                       _native.ptr(idx), _native.ptr(sym)))
        return _msg_vector_from_indices(idx, sym, M, K)
    x = np.ascontiguousarray(s.real, dtype=np.float64)
    idx = np.empty(L, dtype=np.int32)
    _native.check(_native.lib().sg_section_argmax(_native.ptr(x), L, M, _native.ptr(idx)))
    beta = np.zeros((L, M))
    beta[np.arange(L), idx] = 1
    return beta.ravel()


# ------------------------------------------------------------------ base matrices


def pa_iterative(P, sigmaSqr, B, R_PA):
    """Iterative power allocation from asymptotic SE (sparc.py:516-533)."""
    Q = np.zeros(B)
    for b in range(B):
        phi = sigmaSqr + P - Q.mean()
        p_block = 2 * np.log(2) * R_PA * phi
        p_spread = (B * P - Q.sum()) / (B - b)
        if p_block > p_spread:
            Q[b:b + 1] = p_block
        else:
            Q[b:] = p_spread
            break
    Q /= Q.mean() / P
    return Q


def sc_basic(Q, omega, Lambda):
    """(omega, Lambda) spatially coupled base matrix (sparc.py:535-568)."""
    assert type(Q) == np.ndarray
    Lr = Lambda + omega - 1
    if Q.ndim == 0:
        W = np.zeros((Lr, Lambda))
        for c in range(Lambda):
            W[c:c + omega, c] = Q * Lr / omega
    elif Q.ndim == 1:
        B = Q.size
        W = np.zeros((Lr, Lambda * B))
        for c in range(Lambda):
            for r in range(c, c + omega):
                W[r, c * B:(c + 1) * B] = Q * Lr / omega
    else:
        raise Exception('Something wrong with Q')
    assert np.isclose(W.mean(), np.mean(Q)), "Average base matrix values must equal P"
    return W


def create_base_matrix(P, power_allocated=False, spatially_coupled=False, **kwargs):
    """Base entry / vector / matrix W (sparc.py:570-589)."""
    if not power_allocated:
        Q = np.array(P)
    else:
        awgn_var, B, R, R_PA_ratio = map(kwargs.get, ['awgn_var', 'B', 'R', 'R_PA_ratio'])
        Q = pa_iterative(P, awgn_var, B, R * R_PA_ratio)
    if not spatially_coupled:
        return Q
    omega, Lambda = map(kwargs.get, ['omega', 'Lambda'])
    return sc_basic(Q, omega, Lambda)


# ------------------------------------------------------------------ design operator


def transform_size(Mr, Mc, csparc=False):
    """w = 2^ceil(log2(max(Mr+1, Mc+1))) (sparc.py:673,744); complex designs
    also avoid bin w/2: max(Mr+2, Mc+2) (sparc.py:618,748)."""
    d = 2 if csparc else 1
    return 2 ** int(np.ceil(np.log2(max(Mr + d, Mc + d))))


def generate_ordering(W, Mr, Mc, rand_seed, csparc=False):
    """Row/column sub-sampling orders (sparc.py:735-775): one RandomState, the
    same two index arrays re-shuffled cumulatively for every block (row-major
    over the nonzero entries of W).  Real designs draw from 1..w-1; complex
    designs (csparc) from 0..w-1 without 0 and w/2 (sparc.py:747-750)."""
    shape = W.shape
    order0 = np.zeros(shape + (Mr,), dtype=np.uint32)
    order1 = np.zeros(shape + (Mc,), dtype=np.uint32)
    w = transform_size(Mr, Mc, csparc)
    if not csparc:
        rows = np.arange(1, w, dtype=np.uint32)
        cols = np.arange(1, w, dtype=np.uint32)
    else:
        rows = np.delete(np.arange(w, dtype=np.uint32), [0, w // 2])
        cols = np.delete(np.arange(w, dtype=np.uint32), [0, w // 2])
    rng = np.random.RandomState(rand_seed)
    if W.ndim == 0:
        rng.shuffle(rows)
        rng.shuffle(cols)
        return rows[:Mr], cols[:Mc]
    blocks = [(b,) for b in range(shape[0])] if W.ndim == 1 else \
        [(r, c) for r in range(shape[0]) for c in range(shape[1]) if W[r, c] != 0]
    if W.ndim > 2:
        raise Exception("Something is wrong with the ordering")
    for blk in blocks:
        rng.shuffle(rows)
        rng.shuffle(cols)
        order0[blk] = rows[:Mr]
        order1[blk] = cols[:Mc]
    return order0, order1


class DesignOperator:
    """A sub-sampled DCT design matrix A (n x LM) on the GPU.

    Holds the base matrix and orders; `Ab(x)` = A x and `Az(y)` = A^T y are the
    callables sparc_transforms returns (sparc.py:786-875).  Plans (device
    tables) are built lazily per precision and reused by the AMP decoder."""

    csparc = False

    def __init__(self, W, L, M, n, order0, order1):
        self.W = np.array(W, dtype=np.float64)
        self.L, self.M, self.n = int(L), int(M), int(n)
        self.LM = self.L * self.M
        nd = self.W.ndim
        self.Lr = self.W.shape[0] if nd == 2 else 1
        self.Lc = self.W.shape[-1] if nd >= 1 else 1
        self.Mr = self.n // self.Lr if nd == 2 else self.n
        self.Mc = self.LM // self.Lc
        if nd == 0:
            o0, o1 = [np.asarray(order0)], [np.asarray(order1)]
        elif nd == 1:
            o0 = [order0[b] for b in range(self.Lc)]
            o1 = [order1[b] for b in range(self.Lc)]
        else:
            nz = [(r, c) for r in range(self.Lr) for c in range(self.Lc) if self.W[r, c] != 0]
            o0 = [order0[r, c] for r, c in nz]
            o1 = [order1[r, c] for r, c in nz]
        self.order0 = np.ascontiguousarray(np.stack(o0), dtype=np.uint32)
        self.order1 = np.ascontiguousarray(np.stack(o1), dtype=np.uint32)
        self.w = transform_size(self.Mr, self.Mc, self.csparc)
        self._plans = {}

    def plan(self, precision=_native.SG_F64):
        if precision not in self._plans:
            _native.require_gpu()
            h = ct.c_void_p()
            Wf = np.ascontiguousarray(self.W.reshape(-1), dtype=np.float64)
            _native.check(_native.lib().sg_amp_plan_create(
                self.W.ndim, _native.ptr(Wf), self.Lr, self.Lc, self.L, self.M, self.n,
                _native.ptr(self.order0), _native.ptr(self.order1), precision, ct.byref(h)))
            self._plans[precision] = h
        return self._plans[precision]

    def soft_output(self, on=True, precision=_native.SG_F64):
        """Make the following amp_decode_bpsk_batch calls through this
        operator at `precision` keep their last effective observation s for
        amp_llr_bpsk (sg_amp_bpsk_soft_output): L M reals per codeword of the
        batch, nothing while off (the default).  The unmodulated decoders
        need no switch (amp_llr)."""
        _native.check(_native.lib().sg_amp_bpsk_soft_output(self.plan(precision), int(bool(on))))

    def __del__(self):
        for h in getattr(self, "_plans", {}).values():
            try:
                _native.lib().sg_amp_plan_destroy(h)
            except Exception:
                pass

    def apply(self, x, transpose, precision=_native.SG_F64):
        x = np.ascontiguousarray(x, dtype=np.float64)
        batched = x.ndim == 2
        X = x if batched else x[None, :]
        B = X.shape[0]
        out = np.empty((B, self.LM if transpose else self.n))
        _native.check(_native.lib().sg_amp_apply(self.plan(precision), int(transpose), _native.ptr(X),
                                                 B, _native.ptr(out)))
        return out if batched else out[0]

    def Ab(self, x):
        assert np.asarray(x).shape[-1] == self.LM
        return self.apply(x, False)

    def Az(self, y):
        assert np.asarray(y).shape[-1] == self.n
        return self.apply(y, True)


class ComplexDesignOperator(DesignOperator):
    """A sub-sampled FFT design matrix A (n x LM, complex) on the GPU: the
    csparc=True operators of sparc_transforms (sparc.py:593-646, 786-875).
    `Ab(x)` = A x and `Az(y)` = A^H y take and return complex128; double
    precision only."""

    csparc = True

    def plan(self, precision=_native.SG_F64):
        if precision != _native.SG_F64:
            raise NotImplementedError("complex SPARCs run in double precision only ('precision': 'f64')")
        if precision not in self._plans:
            _native.require_gpu()
            h = ct.c_void_p()
            Wf = np.ascontiguousarray(self.W.reshape(-1), dtype=np.float64)
            _native.check(_native.lib().sg_camp_plan_create(
                self.W.ndim, _native.ptr(Wf), self.Lr, self.Lc, self.L, self.M, self.n,
                _native.ptr(self.order0), _native.ptr(self.order1), ct.byref(h)))
            self._plans[precision] = h
        return self._plans[precision]

    def soft_output(self, on=True):
        """Make the following decodes through this operator keep their last
        effective observation s for camp_llr (sg_camp_soft_output): 16 L M
        bytes per codeword of the batch, nothing while off (the default)."""
        _native.check(_native.lib().sg_camp_soft_output(self.plan(), int(bool(on))))

    def __del__(self):
        for h in getattr(self, "_plans", {}).values():
            try:
                _native.lib().sg_camp_plan_destroy(h)
            except Exception:
                pass

    def apply(self, x, transpose, precision=_native.SG_F64):
        x = np.ascontiguousarray(x, dtype=np.complex128)
        batched = x.ndim == 2
        X = x if batched else x[None, :]
        B = X.shape[0]
        out = np.empty((B, self.LM if transpose else self.n), dtype=np.complex128)
        _native.check(_native.lib().sg_camp_apply(self.plan(precision), int(transpose), _native.ptr(X), B,
                                                  _native.ptr(out)))
        return out if batched else out[0]


def sparc_transforms(W, L, M, n, rand_seed, csparc=False):
    """Ab(x) = A x and Az(y) = A^T y (A^H y for csparc) for the design given by
    (W, seed) (sparc.py:703-880), evaluated on the GPU."""
    assert type(W) == np.ndarray
    assert type(L) == int and type(M) == int and type(n) == int
    assert L > 0 and M > 0 and n > 0
    if W.ndim == 0:
        Mr, Mc = n, L * M
    elif W.ndim == 1:
        assert L % W.size == 0
        Mr, Mc = n, L * M // W.size
    elif W.ndim == 2:
        Lr, Lc = W.shape
        assert L % Lc == 0
        assert n % Lr == 0
        Mr, Mc = n // Lr, L * M // Lc
    else:
        raise Exception('Something wrong with base matrix input W')
    order0, order1 = generate_ordering(W, Mr, Mc, rand_seed, csparc)
    op = (ComplexDesignOperator if csparc else DesignOperator)(W, L, M, n, order0, order1)
    return op.Ab, op.Az


def operator_of(Ab, Az):
    """The DesignOperator (or ComplexDesignOperator) behind Ab/Az callables from
    sparc_transforms, or None."""
    a, b = getattr(Ab, "__self__", None), getattr(Az, "__self__", None)
    if isinstance(a, DesignOperator) and a is b:
        return a
    return None


# ------------------------------------------------------------------ AMP


def _received_words(Y, op, dtype):
    """Y as a contiguous [B, n] array of dtype; returns (Y, B)."""
    Y = np.ascontiguousarray(Y, dtype=dtype)
    if Y.ndim != 2 or Y.shape[1] != op.n:
        raise ValueError(f"received words must have shape [B, {op.n}]")
    return Y, Y.shape[0]


def _known_sections(a, name, B, op):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.shape != (B, op.L):
        raise ValueError(f"{name} must have shape [{B}, {op.L}]")
    return a


def _true_sections(a, B, op):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(B, op.L)


def _decode_outputs(B, op, t_max):
    """(map_idx [B, L], t_final [B], nmse [B, t_max, Lc], psi [B, Lc]) for a decoder to fill."""
    return (np.empty((B, op.L), dtype=np.int32), np.empty(B, dtype=np.int32), np.empty((B, t_max, op.Lc)),
            np.empty((B, op.Lc)))


def amp_decode_batch(Y, op, awgn_var, t_max, rtol=1e-6, phi_est_method=1, true_idx=None,
                     precision=_native.SG_F64):
    """Batched AMP on the GPU for codewords sharing one design.

    Y [B, n] received words; true_idx [B, L] transmitted section indices (for
    NMSE) or None.  Returns (map_idx [B, L], t_final [B], nmse [B, t_max, Lc],
    psi [B, Lc])."""
    Y, B = _received_words(Y, op, np.float64)
    ti = None if true_idx is None else _true_sections(true_idx, B, op)
    map_idx, t_final, nmse, psi = _decode_outputs(B, op, t_max)
    _native.check(_native.lib().sg_amp_decode(
        op.plan(precision), _native.ptr(Y), B, _native.ptr(ti), float(awgn_var), int(t_max),
        float(rtol), int(phi_est_method), _native.ptr(map_idx), _native.ptr(t_final),
        _native.ptr(nmse), _native.ptr(psi)))
    return map_idx, t_final, nmse, psi


def amp_decode_partial_batch(Y, op, known_idx, awgn_var, t_max, rtol=1e-6, phi_est_method=1, true_idx=None,
                             precision=_native.SG_F64):
    """amp_decode_batch with some sections of each codeword given: known_idx
    [B, L] holds a section's index in [0, M), or -1 for a section to decode
    (the set is per codeword).  A known section's estimate is the one-hot of
    its index from the start, the residual starts at y - A beta_known, and the
    state evolution starts at the share of unknown sections; map_idx reports
    the known index there.  With every entry -1 this is amp_decode_batch.
    Flat and power-allocated designs, M <= 2048.  Same returns: (map_idx
    [B, L], t_final [B], nmse [B, t_max, Lc], psi [B, Lc])."""
    if op.csparc:
        raise NotImplementedError("AMP with known sections is implemented for real (DCT design) SPARCs only")
    Y, B = _received_words(Y, op, np.float64)
    known = _known_sections(known_idx, "known_idx", B, op)
    ti = None if true_idx is None else _true_sections(true_idx, B, op)
    map_idx, t_final, nmse, psi = _decode_outputs(B, op, t_max)
    _native.check(_native.lib().sg_amp_decode_partial(
        op.plan(precision), _native.ptr(Y), B, _native.ptr(known), _native.ptr(ti), float(awgn_var), int(t_max),
        float(rtol), int(phi_est_method), _native.ptr(map_idx), _native.ptr(t_final), _native.ptr(nmse),
        _native.ptr(psi)))
    return map_idx, t_final, nmse, psi


def bpsk_words(loc, sym):
    """Section words (location << 1) | symbol of a real K=2 SPARC, int32: the
    MSB-first digits of a word are the section's log2 M location bits and its
    symbol bit (0: +1, 1: -1) in the order of bin_arr_2_msg_vector."""
    return ((np.asarray(loc, dtype=np.int64) << 1) | np.asarray(sym, dtype=np.int64)).astype(np.int32)


def amp_decode_bpsk_batch(Y, op, awgn_var, t_max, rtol=1e-6, phi_est_method=1, true_word=None,
                          precision=_native.SG_F64):
    """amp_decode_batch for real K=2 (BPSK) modulated SPARCs: the section's
    non-zero entry is +1 or -1.  A section is reported and supplied as one
    word (bpsk_words): true_word [B, L] the transmitted words (for NMSE) or
    None.  Flat, power-allocated and spatially coupled DCT designs, M a power
    of two in [2, 2048], either precision.  Returns (map_word [B, L], t_final
    [B], nmse [B, t_max, Lc], psi [B, Lc])."""
    if op.csparc:
        raise ValueError("amp_decode_bpsk_batch needs a real DesignOperator (complex designs: camp_decode_batch "
                         "with K=2)")
    Y, B = _received_words(Y, op, np.float64)
    tw = None if true_word is None else _true_sections(true_word, B, op)
    map_word, t_final, nmse, psi = _decode_outputs(B, op, t_max)
    _native.check(_native.lib().sg_amp_decode_bpsk(
        op.plan(precision), _native.ptr(Y), B, _native.ptr(tw), float(awgn_var), int(t_max),
        float(rtol), int(phi_est_method), _native.ptr(map_word), _native.ptr(t_final),
        _native.ptr(nmse), _native.ptr(psi)))
    return map_word, t_final, nmse, psi


def amp_decode_bpsk_partial_batch(Y, op, known_word, awgn_var, t_max, rtol=1e-6, phi_est_method=1, true_word=None,
                                  precision=_native.SG_F64):
    """amp_decode_bpsk_batch with some sections of each codeword given:
    known_word [B, L] holds a section's word (bpsk_words) in [0, 2M), or -1
    for a section to decode (the set is per codeword).  A known section's
    estimate is the +-1 one-hot of its word from the start, the residual
    starts at y - A beta_known, and the state evolution starts at the share of
    unknown sections; map_word reports the known word there.  With every entry
    -1 this is amp_decode_bpsk_batch, bit for bit.  Flat, power-allocated and
    spatially coupled DCT designs, M a power of two in [2, 2048], either
    precision.  It keeps no soft output: amp_llr_bpsk refuses after it.  Same
    returns: (map_word [B, L], t_final [B], nmse [B, t_max, Lc], psi [B, Lc])."""
    if op.csparc:
        raise ValueError("amp_decode_bpsk_partial_batch needs a real DesignOperator (complex designs: "
                         "camp_decode_partial_batch with K=2)")
    Y, B = _received_words(Y, op, np.float64)
    known = _known_sections(known_word, "known_word", B, op)
    tw = None if true_word is None else _true_sections(true_word, B, op)
    map_word, t_final, nmse, psi = _decode_outputs(B, op, t_max)
    _native.check(_native.lib().sg_amp_decode_bpsk_partial(
        op.plan(precision), _native.ptr(Y), B, _native.ptr(known), _native.ptr(tw), float(awgn_var), int(t_max),
        float(rtol), int(phi_est_method), _native.ptr(map_word), _native.ptr(t_final), _native.ptr(nmse),
        _native.ptr(psi)))
    return map_word, t_final, nmse, psi


def amp_llr(op, B, l0, nl, probs_only=False, precision=_native.SG_F64):
    """Soft output of the last amp_decode_batch of B codewords through `op` at
    this precision: for sections [l0, l0 + nl), the LLRs log p - log(1 - p) of
    the section bits (MSB first), p = P(bit = 0) under the decoder's final
    beta clipped to [1e-15, 1 - 1e-15] (beta_estimate_to_bp_probs and ldpc_bp's
    clip, sparc_new.py:1118-1138, 1167-1169), or with probs_only the unclipped
    p.  Returns float64 [B, nl * log2 M] (computed in the plan's precision)."""
    if op.csparc:
        raise NotImplementedError("soft output is implemented for real (DCT design) SPARCs only")
    logM = int(np.log2(op.M))
    out = np.empty((int(B), int(nl) * logM))
    _native.check(_native.lib().sg_amp_llr(op.plan(precision), int(B), int(l0), int(nl), int(bool(probs_only)),
                                           _native.ptr(out)))
    return out


def amp_llr_bpsk(op, B, l0, nl, probs_only=False, precision=_native.SG_F64):
    """Soft output of the last amp_decode_bpsk_batch of B codewords through
    `op` at this precision, decoded after op.soft_output(True, precision): for
    sections [l0, l0 + nl) the LLRs log p - log(1 - p) of the section's
    log2 M location bits, MSB first, and then of its symbol bit (0: +1) -- the
    digits of its word (bpsk_words) -- with p = P(bit = 0) under the joint
    posterior over (location, sign) whose mean is the K=2 denoiser, from each
    codeword's last effective observation s and its tau (a codeword that
    stopped early: those of its last iteration), clipped to
    [1e-15, 1 - 1e-15]; with probs_only the unclipped p.  Returns float64
    [B, nl * (log2 M + 1)] (computed in the plan's precision)."""
    if op.csparc:
        raise ValueError("amp_llr_bpsk needs a real DesignOperator (complex designs: camp_llr with K=2)")
    per = int(np.log2(op.M)) + 1
    out = np.empty((int(B), int(nl) * per))
    _native.check(_native.lib().sg_amp_bpsk_llr(op.plan(precision), int(B), int(l0), int(nl), int(bool(probs_only)),
                                                _native.ptr(out)))
    return out


def _camp_decode(Y, op, known, awgn_var, t_max, rtol, phi_est_method, K, true_idx, true_sym):
    """camp_decode_batch (known None) and camp_decode_partial_batch (known = (known_idx, known_sym)) after their
    own refusals."""
    Y, B = _received_words(Y, op, np.complex128)
    if known is not None:
        ki = _known_sections(known[0], "known_idx", B, op)
        ks = _known_sections(known[1], "known_sym", B, op) if K != 1 else None
    ti = None if true_idx is None else _true_sections(true_idx, B, op)
    ts = _true_sections(true_sym, B, op) if ti is not None and K != 1 else None
    map_idx, t_final, nmse, psi = _decode_outputs(B, op, t_max)
    map_sym = np.zeros((B, op.L), dtype=np.int32)
    c = _interleaved(psk_constel(K)) if K != 1 else None
    head = (op.plan(), _native.ptr(Y), B, int(K), _native.ptr(c))
    tail = (_native.ptr(ti), _native.ptr(ts), float(awgn_var), int(t_max), float(rtol), int(phi_est_method),
            _native.ptr(map_idx), _native.ptr(map_sym), _native.ptr(t_final), _native.ptr(nmse), _native.ptr(psi))
    if known is None:
        _native.check(_native.lib().sg_camp_decode(*head, *tail))
    else:
        _native.check(_native.lib().sg_camp_decode_partial(*head, _native.ptr(ki), _native.ptr(ks), *tail))
    return map_idx, map_sym, t_final, nmse, psi


def camp_decode_batch(Y, op, awgn_var, t_max, rtol=1e-6, phi_est_method=1, K=1, true_idx=None, true_sym=None):
    """Batched AMP on the GPU for complex codewords sharing one complex design.

    Y [B, n] complex received words; K the PSK order (1: unmodulated);
    true_idx / true_sym [B, L] transmitted locations and constellation indices
    (for NMSE) or None.  Returns (map_idx [B, L], map_sym [B, L], t_final [B],
    nmse [B, t_max, Lc], psi [B, Lc])."""
    _check_psk(K)
    return _camp_decode(Y, op, None, awgn_var, t_max, rtol, phi_est_method, K, true_idx, true_sym)


def camp_decode_partial_batch(Y, op, known_idx, known_sym, awgn_var, t_max, rtol=1e-6, phi_est_method=1, K=1,
                              true_idx=None, true_sym=None):
    """camp_decode_batch with some sections of each codeword given: known_idx
    [B, L] holds a section's location in [0, M), or -1 for a section to decode,
    and known_sym [B, L] its constellation index in [0, K) (ignored, and may be
    None, for K = 1); the set is per codeword.  A known section's estimate is
    the one-hot c[sym] at idx from the start, the residual starts at
    y - A beta_known, and the state evolution starts at the share of unknown
    sections; map_idx / map_sym report the known pair there.  With every entry
    -1 this is camp_decode_batch.  Flat, power-allocated and spatially coupled
    designs.  Same returns: (map_idx [B, L], map_sym [B, L], t_final [B], nmse
    [B, t_max, Lc], psi [B, Lc])."""
    if not op.csparc:
        raise ValueError("camp_decode_partial_batch needs a ComplexDesignOperator (real designs: "
                         "amp_decode_partial_batch)")
    _check_psk(K)
    return _camp_decode(Y, op, (known_idx, known_sym), awgn_var, t_max, rtol, phi_est_method, K, true_idx, true_sym)


def camp_llr(op, B, K, l0, nl, probs_only=False):
    """Soft output of the last camp_decode_batch of B codewords at PSK order K
    through the complex operator `op`, decoded after op.soft_output(): for
    sections [l0, l0 + nl) the bits of section_llr_psk -- log2 M location
    bits, then log2 K symbol bits -- from each codeword's last effective
    observation s and its tau (a codeword that stopped early: those of its
    last iteration).  Returns float64 [B, nl * (log2 M + log2 K)]."""
    if not op.csparc:
        raise ValueError("camp_llr needs a ComplexDesignOperator (real designs: amp_llr)")
    _check_psk(K)
    out = np.empty((int(B), int(nl) * _section_bit_count(op.M, K)))
    c = _interleaved(psk_constel(K)) if K != 1 else None
    _native.check(_native.lib().sg_camp_llr(op.plan(), int(B), int(K), _native.ptr(c), int(l0), int(nl),
                                            int(bool(probs_only)), _native.ptr(out)))
    return out


def _sparc_amp_complex(y, op, W, L, M, K, decode_params, awgn_var, beta0):
    """sparc_amp for a complex design: beta real for K in {1, 2}, complex for
    K >= 4 (sparc.py:914, 480-483)."""
    if _precision(decode_params) != _native.SG_F64:
        raise NotImplementedError("complex SPARCs run in double precision only: "
                                  "decode_params['precision'] must be 'f64'")
    t_max, rtol, phi_est_method = map(decode_params.get, ['t_max', 'rtol', 'phi_est_method'])
    true_idx = true_sym = None
    if beta0 is not None:
        ti, ts = _msg_vector_indices(np.asarray(beta0), M, K)
        true_idx, true_sym = ti[None, :], ts[None, :]
    map_idx, map_sym, t_final, nmse, psi = camp_decode_batch(np.asarray(y)[None, :], op, awgn_var, t_max, rtol,
                                                             phi_est_method, K, true_idx, true_sym)
    beta = _msg_vector_from_indices(map_idx[0], map_sym[0], M, K)
    if W.ndim == 0:
        return beta, int(t_final[0]), nmse[0, :, 0].copy(), np.float64(psi[0, 0])
    return beta, int(t_final[0]), nmse[0].copy(), psi[0].copy()


def sparc_amp(y, code_params, decode_params, awgn_var, rand_seed, beta0, Ab=None, Az=None):
    """AMP decoder (sparc.py:883-999) on the GPU.  Returns (beta_MAP, t_final,
    nmse, psi) with the reference's shapes: nmse (t_max,) for a regular
    design, (t_max, Lc) otherwise; psi a scalar or (Lc,).  Complex designs
    (code_params['complex'], optionally K-PSK modulated) run on the complex
    engine in double precision; real K=2 modulated codes (after
    enable_real_psk()) return beta with entries +1 / -1."""
    P, R, L, M, n = map(code_params.get, ['P', 'R', 'L', 'M', 'n'])
    K = code_params['K'] if code_params['modulated'] else 1
    _check_family(K, code_params.get('complex', False))
    tmp = code_params.copy()
    tmp.update({'awgn_var': awgn_var})
    W = create_base_matrix(**tmp)
    assert 0 <= W.ndim <= 2
    t_max, rtol, phi_est_method = map(decode_params.get, ['t_max', 'rtol', 'phi_est_method'])
    assert phi_est_method == 1 or phi_est_method == 2

    if Ab is None or Az is None:
        Ab, Az = sparc_transforms(W, L, M, n, rand_seed, code_params['complex'])
    op = operator_of(Ab, Az)
    if op is None:
        raise NotImplementedError("sparc_amp runs fused on the GPU and needs the Ab/Az returned "
                                  "by ldpc_sparc_amd.sparc.sparc_transforms")
    if op.csparc != bool(code_params.get('complex', False)):
        raise ValueError("Ab/Az do not match code_params['complex']")
    if op.csparc:
        return _sparc_amp_complex(y, op, W, L, M, K, decode_params, awgn_var, beta0)
    if K == 2:
        true_word = None
        if beta0 is not None:
            true_word = bpsk_words(*_msg_vector_indices(np.asarray(beta0), M, K))[None, :]
        map_word, t_final, nmse, psi = amp_decode_bpsk_batch(np.asarray(y)[None, :], op, awgn_var, t_max, rtol,
                                                             phi_est_method, true_word, _precision(decode_params))
        beta = _msg_vector_from_indices(map_word[0] >> 1, map_word[0] & 1, M, K)
        if W.ndim == 0:
            return beta, int(t_final[0]), nmse[0, :, 0].copy(), np.float64(psi[0, 0])
        return beta, int(t_final[0]), nmse[0].copy(), psi[0].copy()
    true_idx = None
    if beta0 is not None:
        b0 = np.asarray(beta0).reshape(L, M)
        true_idx = np.argmax(b0 != 0, axis=1).astype(np.int32)[None, :]
    map_idx, t_final, nmse, psi = amp_decode_batch(np.asarray(y)[None, :], op, awgn_var, t_max,
                                                   rtol, phi_est_method, true_idx,
                                                   _precision(decode_params))
    beta = np.zeros((L, M))
    beta[np.arange(L), map_idx[0]] = 1
    if W.ndim == 0:
        return beta.ravel(), int(t_final[0]), nmse[0, :, 0].copy(), np.float64(psi[0, 0])
    return beta.ravel(), int(t_final[0]), nmse[0].copy(), psi[0].copy()


def test_bin_arr_msg_vector(k=1024 * 9, M=2 ** 9):
    """Round trip bits -> beta -> bits (sparc.py:1003-1008)."""
    seed = list(np.random.randint(2 ** 32 - 1, size=2))
    bin_array = rnd_bin_arr(k, seed)
    msg_vector = bin_arr_2_msg_vector(bin_array, M)
    assert np.array_equal(bin_array, msg_vector_2_bin_arr(msg_vector, M))
