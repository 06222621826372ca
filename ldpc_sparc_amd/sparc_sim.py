"""End-to-end SPARC simulation over AWGN (drop-in for sparc_public/sparc_sim.py).

sparc_sim(code_params, decode_params, awgn_var, rand_seed) returns the
reference's result dict (sparc_sim.py:8-58); the decoder runs on the GPU.
Complex SPARCs, unmodulated or K-PSK modulated (K up to 64), run on the
complex engine in double precision; modulated codes add the location / value
error statistics of calc_ler_ver.  Real K=2 (BPSK) modulated SPARCs run on
the DCT design after sparc.enable_real_psk() (opt-in: refused with
NotImplementedError before), in either precision.  Out of scope
(NotImplementedError): single precision for complex SPARCs, and K > 64.  An
error-rate curve of a complex SPARC is
montecarlo.csparc_ser_sweep (one shared design, generated, decoded and counted
on the GPU); its state-evolution prediction is sparc_se.sparc_se.
"""
import numpy as np

from .sparc import sparc_decode, sparc_encode


def sparc_sim(code_params, decode_params, awgn_var, rand_seed=None):
    """Encode, AWGN channel, AMP decode and error statistics (sparc_sim.py:8-58)."""
    bits_i, beta0, x, Ab, Az = sparc_encode(code_params, awgn_var, rand_seed)
    y = awgn_channel(x, awgn_var, rand_seed)
    bits_o, beta, T, nmse, expect = sparc_decode(y, code_params, decode_params, awgn_var, rand_seed,
                                                 beta0, Ab, Az)
    ber = calc_ber(bits_i, bits_o)
    cer = 1.0 * (ber > 0)
    detect = 1.0 * (not (ber > 0) ^ expect)
    results = {'ber': ber, 'cer': cer, 't_final': T, 'nmse': nmse, 'detect': detect}
    if not code_params['modulated']:
        ser, loc_of_sec_errs, num_of_sec_errs = calc_ser(beta0, beta, code_params['L'])
        results.update({'ser': ser, 'loc_of_sec_errs': loc_of_sec_errs,
                        'num_of_sec_errs': num_of_sec_errs})
    else:
        err_rates, loc_of_errs, num_of_errs = calc_ler_ver(beta0, beta, code_params['L'], code_params['K'])
        ler, ver, ser = err_rates
        loc_of_loc_errs, loc_of_val_errs, loc_of_sec_errs = loc_of_errs
        num_of_loc_errs, num_of_val_errs, num_of_sec_errs = num_of_errs
        results.update({'ser': ser, 'ler': ler, 'ver': ver,
                        'loc_of_sec_errs': loc_of_sec_errs,
                        'loc_of_loc_errs': loc_of_loc_errs,
                        'loc_of_val_errs': loc_of_val_errs,
                        'num_of_sec_errs': num_of_sec_errs,
                        'num_of_loc_errs': num_of_loc_errs,
                        'num_of_val_errs': num_of_val_errs})
    return results


def calc_ber(true_bin_array, est_bin_array):
    """Fraction of differing bits (sparc_sim.py:62-70)."""
    assert true_bin_array.dtype == 'bool'
    assert est_bin_array.dtype == 'bool'
    k = true_bin_array.size
    assert k == est_bin_array.size
    return np.count_nonzero(np.bitwise_xor(true_bin_array, est_bin_array)) / k


def calc_ser(beta0, beta, L):
    """Section error rate, error locations and count (sparc_sim.py:72-98)."""
    assert beta.size == beta0.size, 'beta and beta0 are of different size'
    assert beta.dtype == beta0.dtype, 'beta and beta0 are of different type'
    assert type(L) == int and L > 0
    assert beta.size % L == 0
    M = beta.size // L
    err = np.any(beta.reshape(L, M) != beta0.reshape(L, M), axis=1)
    num = int(np.count_nonzero(err))
    return num / L, np.flatnonzero(err), num


def calc_ler_ver(beta0, beta, L, K):
    """Location, value and section error rates of a modulated message vector
    (sparc_sim.py:100-175): ((ler, ver, ser), (loc_of_loc_errs, loc_of_val_errs,
    loc_of_sec_errs), (num_of_loc_errs, num_of_val_errs, num_of_sec_errs))."""
    assert beta.size == beta0.size, 'beta and beta0 are of different size'
    assert beta.dtype == beta0.dtype, 'beta and beta0 are of different type'
    assert type(L) == int and L > 0
    assert beta.size % L == 0
    M = beta.size // L
    b0, b = beta0.reshape(L, M), beta.reshape(L, M)
    r0, c0 = np.nonzero(b0)
    r1, c1 = np.nonzero(b)
    assert np.array_equal(r0, np.arange(L))  # exactly one nonzero per section
    assert np.array_equal(r1, np.arange(L))
    loc_err = c0 != c1
    val_err = b0[r0, c0] != b[r1, c1]
    sec_err = np.logical_or(loc_err, val_err)
    nums = tuple(int(np.count_nonzero(e)) for e in (loc_err, val_err, sec_err))
    return (tuple(k / L for k in nums),
            tuple(np.flatnonzero(e) for e in (loc_err, val_err, sec_err)), nums)


def awgn_channel(input_array, awgn_var, rand_seed):
    """y = x + N(0, awgn_var) from RandomState(rand_seed) (sparc_sim.py:179-204, real case)."""
    assert input_array.ndim == 1, 'input array must be one-dimensional'
    assert awgn_var >= 0
    rng = np.random.RandomState(rand_seed)
    n = input_array.size
    if input_array.dtype == np.float64:
        return input_array + np.sqrt(awgn_var) * rng.randn(n)
    if input_array.dtype == np.complex128:
        return input_array + np.sqrt(awgn_var / 2) * (rng.randn(n) + 1j * rng.randn(n))
    raise Exception("Unknown input type '{}'".format(input_array.dtype))
