"""The yardstick of the complex engine's soft output and of the concatenated
K-PSK SPARC + LDPC decoder, in NumPy; it shares no code with ldpc_sparc_amd.

A section of a K-PSK modulated complex SPARC carries log2 M MSB-first location
bits, then log2 K Gray-coded symbol bits (msg_vector_2_bin_arr,
sparc.py:366-400).  Given the effective observation s = beta0 + CN(0, tau) the
posterior over (location j, symbol k) is p(j, k) ~ exp(Re(x_j conj c_k)) with
x = s / (tau / 2) -- the weights msg_vector_mmse_estimator (sparc.py:402-465)
averages c_k with -- and P(bit = 0) is its sum over the (j, k) whose bit is
clear.  Here that is done by brute force over every (j, k).  The AMP loop is
that of tests/csparc_ref.py, returning what the soft output needs: the last s
and tau.  Then dct_concat_ref.llr_of_probs and oracle.bp.decode("sumprod2")."""
import numpy as np

import csparc_ref
from dct_concat_ref import llr_of_probs


def constel(K):
    return np.array([1.0 + 0j]) if K == 1 else np.asarray(csparc_ref.constel(K), dtype=complex)


def bits_of(M, K):
    logM, logK = int(round(np.log2(M))), int(round(np.log2(K)))
    return logM, logK


def section_words(idx, sym, K):
    """idx << log2 K | gray(sym): the section's bits as one integer."""
    logK = int(round(np.log2(K)))
    sym = np.asarray(sym, dtype=np.int64)
    return (np.asarray(idx, dtype=np.int64) << logK) | (sym ^ (sym >> 1))


def word_bits(words, nbits):
    """MSB-first bits [len(words) * nbits] of the section words."""
    return ((np.asarray(words, dtype=np.int64)[..., None] >> np.arange(nbits)[::-1]) & 1).reshape(-1)


def joint_posterior(x, M, K):
    """p [L, M, K] over (location, symbol) of x = s / (tau / 2), complex [L M]."""
    c = constel(K)
    X = np.asarray(x, dtype=complex).reshape(-1, M)
    arg = X.real[:, :, None] * c.real[None, None, :] + X.imag[:, :, None] * c.imag[None, None, :]
    w = np.exp(arg - arg.max(axis=(1, 2), keepdims=True))
    return w / w.sum(axis=(1, 2), keepdims=True)


def bit_probs(x, M, K):
    """P(bit = 0) [L, log2 M + log2 K] by enumeration of every (j, k)."""
    logM, logK = bits_of(M, K)
    p = joint_posterior(x, M, K)
    L = p.shape[0]
    out = np.zeros((L, logM + logK))
    for j in range(M):
        for k in range(K):
            word = (j << logK) | (k ^ (k >> 1))
            for pos in range(logM + logK):
                if ((word >> (logM + logK - 1 - pos)) & 1) == 0:
                    out[:, pos] += p[:, j, k]
    return out


def x_of(s, tau_use):
    """s / (tau / 2); tau_use scalar or per entry."""
    t = np.asarray(tau_use, dtype=np.float64) / 2
    return s.real / t + 1j * (s.imag / t)


def amp_soft(y, W, L, M, n, K, Ab, Az, awgn_var, t_max, rtol=1e-6, phi_est_method=1):
    """The AMP loop of csparc_ref.amp.  Returns a dict: s and tau_use of the
    last executed iteration, the MAP (idx, sym) of that s, t_final, and
    `margin`: over the stopping tests taken, the smallest factor by which
    |psi - psi_prev| stayed away from its threshold (above it where the loop
    went on, below it where it stopped)."""
    W = np.asarray(W, dtype=np.float64)
    atol = 2e-15
    Lc = W.shape[-1] if W.ndim >= 1 else 1
    Mc = L * M // Lc
    if W.ndim == 2:
        Lr = W.shape[0]
        Mr = n // Lr
    beta = np.zeros(L * M, dtype=complex)
    z = y
    gamma = W if W.ndim == 0 else np.dot(W, np.ones(Lc)) / Lc
    margin = np.inf
    for t in range(t_max - 1):
        if t > 0:
            psi_prev, phi_prev = np.copy(psi), np.copy(phi)
            gamma = W * psi if W.ndim == 0 else np.dot(W, psi) / Lc
            b = gamma / phi_prev
            z = y - Ab(beta) + (b * z if W.ndim != 2 else b.repeat(Mr) * z)
        if phi_est_method == 1:
            phi = awgn_var + gamma
        elif W.ndim != 2:
            phi = (np.abs(z) ** 2).mean()
        else:
            phi = (np.abs(z) ** 2).reshape(Lr, -1).mean(axis=1)
        if W.ndim == 0:
            tau_use, phi_use = (L * phi / n) / W, phi
        elif W.ndim == 1:
            tau_use, phi_use = ((L * phi / n) / W).repeat(Mc), phi
        else:
            tau_use, phi_use = ((L / Mr) / np.dot(W.T, 1 / phi)).repeat(Mc), phi.repeat(Mr)
        s = beta + tau_use * Az(z / phi_use)
        beta = csparc_ref.mmse(s, tau_use, M, K).astype(complex)
        if W.ndim == 0:
            psi = 1 - (np.abs(beta) ** 2).sum() / L
        else:
            psi = 1 - (np.abs(beta) ** 2).reshape(Lc, -1).sum(axis=1) / (L / Lc)
        if t > 0:
            diff = np.atleast_1d(np.abs(psi - psi_prev))
            thr = np.atleast_1d(atol + rtol * np.abs(psi_prev))
            stop = bool(np.all(diff <= thr))
            with np.errstate(divide="ignore"):
                margin = min(margin, float(np.min(thr / diff)) if stop else float(np.max(diff / thr)))
            if stop:
                break
    idx, sym = csparc_ref.map_indices(s, M, K)
    return {"s": s, "tau_use": tau_use, "idx": np.asarray(idx), "sym": np.asarray(sym), "t_final": t + 1,
            "margin": margin}


def soft_probs(st, M, K):
    """P(bit = 0) [L, log2 M + log2 K] of an amp_soft result."""
    return bit_probs(x_of(st["s"], st["tau_use"]), M, K)


def decode_user_bits(st, L, M, K, L_unp, c, bp_its=200):
    """User bits of one codeword and the BP iteration counts: the MAP bits of
    the unprotected sections, then the systematic hard decisions of sumprod2
    on every LDPC block of the protected sections."""
    from oracle import bp
    logM, logK = bits_of(M, K)
    per = logM + logK
    unp = word_bits(section_words(st["idx"][:L_unp], st["sym"][:L_unp], K), per)
    llr = llr_of_probs(soft_probs(st, M, K)[L_unp:].reshape(-1)).reshape(-1, c.N)
    out, its = [unp], []
    for blk in llr:
        app, it = bp.decode("sumprod2", blk, c.vdeg, c.cdeg, c.intrlv, bp_its)
        out.append((app[:c.K] < 0).astype(np.int64))
        its.append(int(it))
    return np.concatenate(out), its


def counters(user_bits, truth, n_unp):
    """The five counters of ConcatPipeline over [B, user bits] decisions."""
    err = np.asarray(user_bits) != np.asarray(truth)
    per_cw = err.sum(axis=1)
    return np.array([err.shape[0], err.sum(), (per_cw > 0).sum(), err[:, :n_unp].sum(), err[:, n_unp:].sum()],
                    dtype=np.int64)
