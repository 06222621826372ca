"""The yardstick of the K = 2 decoder's soft output (sg_amp_bpsk_llr*,
amp_bpsk_llr.hip) and of the concatenated real K = 2 SPARC + LDPC decoder
(pipeline.DctBpskConcatPipeline), in NumPy; what it computes shares no code
with ldpc_sparc_amd (the designs and batches of the shared cases at the end are
drawn with the package's generators, as the other tests draw theirs).

A section of a real K = 2 modulated SPARC carries log2 M MSB-first location
bits and then one symbol bit (0: +1, 1: -1): the digits of its word
(location << 1) | symbol.  Given the effective observation s = beta0 + N(0, tau)
the posterior over (location j, symbol c = +-1) is p(j, c) ~ exp(c x_j) with
x = s / tau -- the weights whose mean is the K = 2 denoiser
(amp_bpsk_ref.mmse_bpsk, sparc.py:433-441) -- and P(bit = 0) is its sum over
the (j, c) whose bit is clear, here by brute force over every (j, c)
(csparc_concat_ref.bit_probs with K = 2 on real x).  The AMP loop is
amp_bpsk_ref.amp_bpsk operation for operation, returning what the soft output
needs: the last s and tau.  Then dct_concat_ref.llr_of_probs and
oracle.bp.decode("sumprod2")."""
import numpy as np

import amp_bpsk_ref as br
import csparc_concat_ref as cref
from csparc_concat_ref import counters, word_bits  # noqa: F401  (the K-PSK yardstick's, unchanged)
from dct_concat_ref import llr_of_probs


def amp_bpsk_soft(y, W, L, M, n, awgn_var, t_max, Ab, Az, rtol=1e-6, phi_method=1):
    """amp_bpsk_ref.amp_bpsk, returning a dict: s and tau_use (per entry) of
    the last executed iteration, the MAP words of that s, t_final, psi."""
    W = np.asarray(W, dtype=float)
    beta = np.zeros(L * M)
    z = y
    atol = 2 * np.finfo(np.float64).resolution
    Lc = W.shape[-1] if W.ndim >= 1 else 1
    Mc = L * M // Lc
    if W.ndim == 2:
        Lr = W.shape[0]
        Mr = n // Lr
    gamma = W if W.ndim == 0 else np.dot(W, np.ones(Lc)) / Lc
    psi = phi = None
    for t in range(t_max - 1):
        if t > 0:
            psi_prev = np.copy(psi)
            phi_prev = np.copy(phi)
            gamma = W * psi if W.ndim == 0 else np.dot(W, psi) / Lc
            b = gamma / phi_prev
            z = y - Ab(beta) + (b * z if W.ndim != 2 else b.repeat(Mr) * z)
        if phi_method == 1:
            phi = awgn_var + gamma
        else:
            phi = (np.abs(z) ** 2).mean() if W.ndim != 2 else (np.abs(z) ** 2).reshape(Lr, -1).mean(axis=1)
        if W.ndim == 0:
            tau_use, phi_use = np.full(L * M, (L * phi / n) / W), phi
        elif W.ndim == 1:
            tau_use, phi_use = ((L * phi / n) / W).repeat(Mc), phi
        else:
            tau_use, phi_use = ((L / Mr) / np.dot(W.T, 1 / phi)).repeat(Mc), phi.repeat(Mr)
        s = beta + tau_use * Az(z / phi_use)
        beta = br.mmse_bpsk(s, tau_use, M)
        if W.ndim == 0:
            psi = 1 - (np.abs(beta) ** 2).sum() / L
        else:
            psi = 1 - (np.abs(beta) ** 2).reshape(Lc, -1).sum(axis=1) / (L / Lc)
        if t > 0 and np.allclose(psi, psi_prev, rtol, atol=atol):
            break
    return {"s": s, "tau_use": tau_use, "words": br.map_words(s, M), "t_final": t + 1, "psi": psi}


def posterior_mean(x, M):
    """sum_c c p(j, c) [L M] of x = s / tau: the K = 2 denoiser, from the enumerated posterior."""
    p = cref.joint_posterior(x, M, 2)
    return (p[:, :, 0] - p[:, :, 1]).reshape(-1)


def bit_probs(x, M):
    """P(bit = 0) [L, log2 M + 1] of x = s / tau (real), by enumeration of every (j, c)."""
    return cref.bit_probs(np.asarray(x, dtype=np.float64), M, 2)


def soft_probs(st, M):
    """P(bit = 0) [L, log2 M + 1] of an amp_bpsk_soft result."""
    return bit_probs(st["s"] / st["tau_use"], M)


def decode_user_bits(st, L, M, L_unp, c, bp_its=200):
    """(user bits, BP iteration counts, protected LLRs) of one codeword: the
    MAP bits of the unprotected sections, then the systematic hard decisions
    of sumprod2 on every LDPC block of the protected sections."""
    from oracle import bp
    per = int(round(np.log2(M))) + 1
    unp = word_bits(st["words"][:L_unp], per)
    llr = llr_of_probs(soft_probs(st, M)[L_unp:].reshape(-1)).reshape(-1, c.N)
    out, its = [unp], []
    for blk in llr:
        app, it = bp.decode("sumprod2", blk, c.vdeg, c.cdeg, c.intrlv, bp_its)
        out.append((app[:c.K] < 0).astype(np.int64))
        its.append(int(it))
    return np.concatenate(out), its, llr.reshape(-1)


def user_bits_truth(words_b, info_b, L_unp, per):
    return np.concatenate([word_bits(words_b[:L_unp], per), np.asarray(info_b).reshape(-1)])


def flat_design(L, M, n, P, seed):
    """(W, order0, order1) of the flat design as the package draws it from a seed."""
    from ldpc_sparc_amd import sparc
    W = np.array(float(P))
    o0, o1 = sparc.generate_ordering(W, n, L * M, seed)
    return W, o0, o1


# ---- shapes and operating points shared by tests/test_bpsk_concat_host.py and tests/test_bpsk_concat_gpu.py

P, LDPC = 15.0, ("802.11n", "1/2", 27)
# (L, M, L_unp, mults, n, awgn_var): flat P = 15, design_seed 0, eight codewords from default_rng(1)
POINTS = {"A": (144, 32, 36, 1, 864, 4.0), "B": (108, 128, 27, 1, 864, 4.0)}
PIPE_B = 8

# section sizes: name -> (L, M); flat, R = 1 (n = L (log2 M + 1)), B = 3, t_max = 3
SIZES = {"m2": (64, 2), "m64": (32, 64), "m128": (32, 128), "m512": (16, 512), "m1024": (8, 1024), "m2048": (8, 2048)}
SIZE_B, SIZE_TMAX = 3, 3


def golden_batch(g, name, cp, ops):
    """The three seeds' transmitted words of a golden case (tests/bpsk_cases.py) as one batch on seed 0's design,
    the received words regenerated from the CPU operators at awgn_var = 1: (Y [3, n], words [3, L])."""
    from bpsk_cases import true_words
    M = cp['M']
    tw = np.stack([true_words(g[f"{name}_s{si}_bits"], M) for si in range(3)])
    rng = np.random.RandomState(17)
    Y = np.stack([ops[0](br.beta_of_words(w, M)) for w in tw]) + rng.randn(3, int(g[f"{name}_s0_n"]))
    return Y, tw


def size_case(name):
    """(W, L, M, n, o0, o1, words [B, L], Y [B, n]) of a section-size case (CPU operators for x)."""
    from oracle import sparc_ref
    if name == "pa256":  # four column blocks, each with its own tau
        from ldpc_sparc_amd import sparc
        L, M = 32, 256
        n = L * 9
        W = sparc.create_base_matrix(P, power_allocated=True, awgn_var=1.0, B=4, R=1.0, R_PA_ratio=1.0)
        o0, o1 = sparc.generate_ordering(W, n, L * M // 4, 5)
    else:
        L, M = SIZES[name]
        n = L * (int(np.log2(M)) + 1)
        W, o0, o1 = flat_design(L, M, n, P, 5)
    Ab, Az = sparc_ref.dct_operators(W, L, M, n, o0, o1)
    rng = np.random.RandomState(100 + M)
    words = rng.randint(0, 2 * M, (SIZE_B, L)).astype(np.int32)
    Y = np.stack([Ab(br.beta_of_words(w, M)) for w in words]) + rng.randn(SIZE_B, n)
    return W, L, M, n, o0, o1, words, Y, (Ab, Az)


def point_batch(name):
    """The host batch of an operating point, as pipeline.make_batch draws it
    from default_rng(1): (words [B, L], info [B * mults, K], noise [B, n])."""
    from ldpc_sparc_amd.ldpc import code
    L, M, Lu, mults, n, var = POINTS[name]
    c = code(*LDPC)
    per = int(np.log2(M)) + 1
    rng = np.random.default_rng(1)
    unp = rng.integers(0, 2, (PIPE_B, Lu * per))
    info = rng.integers(0, 2, (PIPE_B * mults, c.K))
    cw = c.encode_batch(info).reshape(PIPE_B, mults * c.N)
    bits = np.concatenate([unp, cw], axis=1).reshape(PIPE_B, L, per)
    words = (bits.astype(np.int64) @ (1 << np.arange(per)[::-1])).astype(np.int32)
    noise = np.sqrt(var) * rng.standard_normal((PIPE_B, n))
    return words, info, noise
