"""The yardstick of the real K = 2 (BPSK) modulated AMP decode
(sg_amp_decode_bpsk*, amp_oploop.hip): a NumPy restatement per codeword on
oracle.sparc_ref's DCT operators.

amp_bpsk is oracle.sparc_ref.amp (sparc.py:883-999) operation for operation,
with the K = 2 denoiser (sparc.py:433-441, exp in longdouble, the global shift
by max |x|) in the place of the softmax and the K = 2 decision (sparc.py:488-492)
at the end.  Sections are words (location << 1) | symbol, symbol 0 for +1."""
import numpy as np

from oracle import sparc_ref


def mmse_bpsk(s, tau, M):
    """sparc.py:433-441 and 463."""
    x = s / tau
    x_max = np.abs(x).max()
    tmp1 = np.exp(x - x_max, dtype=np.longdouble)
    tmp2 = np.exp(-x - x_max, dtype=np.longdouble)
    top = tmp1 - tmp2
    bot = (tmp1 + tmp2).reshape(-1, M).sum(axis=1).repeat(M)
    return (top / bot).astype(np.float64)


def map_words(s, M):
    """sparc.py:488-492 as words: the first maximum of |s|, symbol 1 where s there is negative."""
    s2 = s.reshape(-1, M)
    idx = np.abs(s2).argmax(axis=1)
    return ((idx << 1) | (s2[np.arange(s2.shape[0]), idx] < 0)).astype(np.int32)


def beta_of_words(words, M):
    words = np.asarray(words)
    beta = np.zeros((words.size, M))
    beta[np.arange(words.size), words >> 1] = 1 - 2 * (words & 1)
    return beta.ravel()


def amp_bpsk(y, W, L, M, n, awgn_var, t_max, Ab, Az, beta0, rtol=1e-6, phi_method=1):
    """Returns (map_word [L], t_final, nmse, psi) -- t_final, nmse, psi as sparc_ref.amp."""
    W = np.asarray(W, dtype=float)
    beta = np.zeros(L * M)
    z = y
    atol = 2 * np.finfo(np.float64).resolution
    if W.ndim == 0:
        gamma = W
        nmse = np.ones(t_max)
    else:
        if W.ndim == 2:
            Lr = W.shape[0]
            Mr = n // Lr
        Lc = W.shape[-1]
        Mc = L * M // Lc
        gamma = np.dot(W, np.ones(Lc)) / Lc
        nmse = np.ones((t_max, Lc))
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
            tau = (L * phi / n) / W
            tau_use, phi_use = tau, phi
        elif W.ndim == 1:
            tau = (L * phi / n) / W
            tau_use, phi_use = tau.repeat(Mc), phi
        else:
            tau = (L / Mr) / np.dot(W.T, 1 / phi)
            tau_use, phi_use = tau.repeat(Mc), phi.repeat(Mr)
        s = beta + tau_use * Az(z / phi_use)
        beta = mmse_bpsk(s, tau_use, M)
        if W.ndim == 0:
            psi = 1 - (np.abs(beta) ** 2).sum() / L
            nmse[t + 1] = (np.abs(beta - beta0) ** 2).sum() / L
        else:
            psi = 1 - (np.abs(beta) ** 2).reshape(Lc, -1).sum(axis=1) / (L / Lc)
            nmse[t + 1] = (np.abs(beta - beta0) ** 2).reshape(Lc, -1).sum(axis=1) / (L / Lc)
        if t > 0 and np.allclose(psi, psi_prev, rtol, atol=atol):
            nmse[t:] = nmse[t]
            break
    return map_words(s, M), t + 1, nmse, psi


def operators(W, L, M, n, o0, o1):
    return sparc_ref.dct_operators(W, L, M, n, o0, o1)


def decode_batch(Y, W, L, M, n, awgn_var, t_max, Ab, Az, true_word, rtol=1e-6, phi_method=1):
    """amp_bpsk per codeword in the shapes of sparc.amp_decode_bpsk_batch: (map_word [B, L], t_final [B], nmse
    [B, t_max, Lc], psi [B, Lc])."""
    res = [amp_bpsk(Y[b], W, L, M, n, awgn_var, t_max, Ab, Az, beta_of_words(true_word[b], M), rtol, phi_method)
           for b in range(len(Y))]
    return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32),
            np.stack([np.asarray(r[2]).reshape(t_max, -1) for r in res]),
            np.stack([np.atleast_1d(r[3]) for r in res]))
