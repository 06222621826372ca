"""From-scratch NumPy restatement of the complex SPARC design operator and AMP
decoder (sparc.py:593-646, 703-880, 883-999 with csparc=True): scatter,
np.fft.fft, gather; float64 denoisers with a per-section maximum.  The
yardstick of the complex engine's operator tests and the CPU baseline of
tools/csparc_time.py.  It shares no code with ldpc_sparc_amd."""
import numpy as np


def _blocks(W, order0, order1):
    """[(r, c, scale, o0, o1)] of the nonzero blocks in row-major order."""
    W = np.asarray(W, dtype=np.float64)
    if W.ndim == 0:
        return [(0, 0, float(W), np.asarray(order0), np.asarray(order1))]
    if W.ndim == 1:
        return [(0, c, float(W[c]), order0[c], order1[c]) for c in range(W.size)]
    return [(r, c, float(W[r, c]), order0[r, c], order1[r, c])
            for r in range(W.shape[0]) for c in range(W.shape[1]) if W[r, c] != 0]


def fft_operators(W, L, M, n, order0, order1):
    """Ab(x) = A x (complex [n]) and Az(y) = A^H y (complex [L M])."""
    W = np.asarray(W, dtype=np.float64)
    Lr = W.shape[0] if W.ndim == 2 else 1
    Lc = W.shape[-1] if W.ndim >= 1 else 1
    Mr, Mc = n // Lr, L * M // Lc
    w = 2 ** int(np.ceil(np.log2(max(Mr + 2, Mc + 2))))
    blocks = _blocks(W, order0, order1)

    def Ab(x):
        out = np.zeros(n, dtype=complex)
        for r, c, wv, o0, o1 in blocks:
            ext = np.zeros(w, dtype=complex)
            ext[o1] = x[c * Mc:(c + 1) * Mc]
            out[r * Mr:(r + 1) * Mr] += np.sqrt(wv / L) * np.fft.fft(ext)[o0]
        return out

    def Az(y):
        out = np.zeros(L * M, dtype=complex)
        for r, c, wv, o0, o1 in blocks:
            ext = np.zeros(w, dtype=complex)
            ext[o0] = y[r * Mr:(r + 1) * Mr]
            out[c * Mc:(c + 1) * Mc] += np.sqrt(wv / L) * np.fft.fft(ext.conj()).conj()[o1]
        return out

    return Ab, Az


def constel(K):
    if K == 2:
        return np.array([1.0, -1.0])
    if K == 4:
        return np.array([1, 1j, -1, -1j])
    th = 2 * np.pi * np.arange(K) / K
    return np.cos(th) + 1j * np.sin(th)


def mmse(s, tau, M, K):
    """K-PSK MMSE estimate of complex s (tau per entry or scalar, not yet halved)."""
    t = np.asarray(tau, dtype=np.float64) / 2
    S = s.reshape(-1, M)
    if K == 1:
        x = (s.real / t).reshape(-1, M)
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True)).ravel()
    if K == 2:
        x = (s.real / t).reshape(-1, M)
        m = np.abs(x).max(axis=1, keepdims=True)
        a, b = np.exp(x - m), np.exp(-x - m)
        return ((a - b) / (a + b).sum(axis=1, keepdims=True)).ravel()
    if K == 4:
        x, y = (s.real / t).reshape(-1, M), (s.imag / t).reshape(-1, M)
        m = np.maximum(np.abs(x), np.abs(y)).max(axis=1, keepdims=True)
        a, b, c, d = np.exp(x - m), np.exp(-x - m), np.exp(y - m), np.exp(-y - m)
        return (((a - b) + 1j * (c - d)) / ((a + b) + (c + d)).sum(axis=1, keepdims=True)).ravel()
    c = constel(K)
    X = ((s / t).reshape(-1, M)[:, :, None] * c.conj()[None, None, :]).real
    e = np.exp(X - X.max(axis=(1, 2), keepdims=True))
    return ((e @ c) / e.sum(axis=(1, 2))[:, None]).ravel()


def map_indices(s, M, K):
    """(locations, constellation indices) of the MAP estimate of s."""
    S = s.reshape(-1, M)
    L = S.shape[0]
    if K == 1:
        return S.real.argmax(axis=1), np.zeros(L, dtype=int)
    if K == 2:
        idx = np.abs(S.real).argmax(axis=1)
        return idx, (S.real[np.arange(L), idx] < 0).astype(int)
    if K == 4:
        idx = np.maximum(np.abs(S.real), np.abs(S.imag)).argmax(axis=1)
        k = np.rint(K * np.angle(S[np.arange(L), idx]) / (2 * np.pi)).astype(int)
        return idx, k % K
    c = constel(K)
    T = (S.conj()[:, :, None] * c[None, None, :]).real.reshape(L, -1)
    flat = T.argmax(axis=1)
    return flat // K, flat % K


def amp(y, W, L, M, n, K, Ab, Az, awgn_var, t_max, rtol=1e-6, phi_est_method=1, beta0=None):
    """AMP decode of one complex codeword; returns (map_idx, map_sym, t_final, nmse, psi)."""
    W = np.asarray(W, dtype=np.float64)
    atol = 2e-15
    Lc = W.shape[-1] if W.ndim >= 1 else 1
    Mc = L * M // Lc
    if W.ndim == 2:
        Lr = W.shape[0]
        Mr = n // Lr
    beta = np.zeros(L * M, dtype=complex)
    z = y
    if W.ndim == 0:
        gamma = W
        nmse = np.ones(t_max)
    else:
        gamma = np.dot(W, np.ones(Lc)) / Lc
        nmse = np.ones((t_max, Lc))
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
        beta = mmse(s, tau_use, M, K).astype(complex)
        if W.ndim == 0:
            psi = 1 - (np.abs(beta) ** 2).sum() / L
            if beta0 is not None:
                nmse[t + 1] = (np.abs(beta - beta0) ** 2).sum() / L
        else:
            psi = 1 - (np.abs(beta) ** 2).reshape(Lc, -1).sum(axis=1) / (L / Lc)
            if beta0 is not None:
                nmse[t + 1] = (np.abs(beta - beta0) ** 2).reshape(Lc, -1).sum(axis=1) / (L / Lc)
        if t > 0 and np.allclose(psi, psi_prev, rtol, atol=atol):
            nmse[t:] = nmse[t]
            break
    idx, sym = map_indices(s, M, K)
    return idx, sym, t + 1, nmse, psi
