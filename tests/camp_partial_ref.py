"""The yardstick of the complex AMP decode with known sections
(sg_camp_decode_partial*) and of the three-stage concatenated K-PSK decoder
AMP -> BP -> AMP (pipeline.CsparcConcat3Pipeline): NumPy restatements per
codeword on csparc_ref's FFT operators and estimators, and the geometry and
operating point the tests share.  The reference project has no such decoder.

amp_partial is csparc_ref.amp (sparc.py:883-999, W of ndim 0, 1 or 2) with two
differences: the denoiser of a known section returns the one-hot c[sym] at its
location, and the start is beta0 = the known one-hots, z0 = y - Ab(beta0), with
psi0_c the share of unknown sections of column block c in the place of 1
(gamma0 = W psi0, or dot(W, psi0) / Lc).  With no known section every operation
is csparc_ref.amp's, in its order.

unpack_words inverts csparc_concat_ref.section_words; three_stage composes
csparc_concat_ref's AMP -> LLR -> BP with amp_partial_ref.known_sections (at
logM = the bits of a section) and both."""
import numpy as np

import amp_partial_ref
import csparc_concat_ref as cref
import csparc_ref
from dct_concat_ref import llr_of_probs

# ---- the geometry: 36 unprotected + 108 protected sections of M = 16 locations and K = 4 symbols (6 bits); the
# protected ones hold one 802.11n r1/2 z = 27 block (648 bits).  n complex channel uses.
GEOM = dict(L=144, M=16, K=4, n=432, P=15.0, L_unp=36, mults=1, ldpc=("802.11n", "1/2", 27))
# ---- the operating point of the value test (chosen on the CPU, tests/test_camp_partial_host.py): flat design of
# seed DESIGN_SEED, a batch of B_POINT codewords drawn as CsparcConcatPipeline.make_batch draws them from
# default_rng(BATCH_SEED), noise variance VAR (known to the decoder), t_max = 25, 200 BP iterations
DESIGN_SEED, BATCH_SEED, B_POINT, VAR = 2, 11, 8, 4.0

_point = {}


def gray2bin(g):
    g = np.array(g, dtype=np.int64)
    m = g >> 1
    while np.any(m):
        g ^= m
        m >>= 1
    return g


def unpack_words(words, K):
    """(idx, sym) of section words idx << log2 K | gray(sym); a word < 0 gives (-1, 0)."""
    w = np.asarray(words, dtype=np.int64)
    logK = int(round(np.log2(K)))
    neg = w < 0
    idx = np.where(neg, -1, w >> logK)
    sym = np.where(neg, 0, gray2bin(np.where(neg, 0, w) & (K - 1)))
    return idx.astype(np.int32), sym.astype(np.int32)


def one_hots(idx, sym, M, K):
    """beta [B, L M] complex with c[sym] at idx of every section."""
    idx, sym = np.atleast_2d(idx), np.atleast_2d(sym)
    B, L = idx.shape
    beta = np.zeros((B, L * M), dtype=complex)
    beta[np.arange(B)[:, None], np.arange(L) * M + idx] = cref.constel(K)[sym]
    return beta


def amp_partial(y, W, L, M, n, K, Ab, Az, awgn_var, t_max, beta0, known_idx, known_sym, rtol=1e-6, phi_est_method=1):
    """known_idx [L]: location in [0, M) or -1; known_sym [L]: constellation
    index (None for K = 1).  Returns (map_idx, map_sym, t_final, nmse, psi) as
    csparc_ref.amp."""
    W = np.asarray(W, dtype=np.float64)
    atol = 2e-15
    Lc = W.shape[-1] if W.ndim >= 1 else 1
    Mc = L * M // Lc
    if W.ndim == 2:
        Lr = W.shape[0]
        Mr = n // Lr
    known_idx = np.asarray(known_idx)
    kn = np.flatnonzero((known_idx >= 0) & (known_idx < M))
    ksym = np.zeros(L, dtype=int) if K == 1 else np.asarray(known_sym) % K
    one_hot = np.zeros((L, M), dtype=complex)
    one_hot[kn, known_idx[kn]] = cref.constel(K)[ksym[kn]]
    unknown = np.ones(L)
    unknown[kn] = 0
    beta = one_hot.ravel().copy()
    z = y - Ab(beta)
    if W.ndim == 0:
        psi = unknown.sum() / L
        gamma = W * psi
        nmse = np.ones(t_max)
    else:
        psi = unknown.reshape(Lc, -1).sum(axis=1) / (L / Lc)
        gamma = np.dot(W, psi) / Lc
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
        beta = csparc_ref.mmse(s, tau_use, M, K).astype(complex).reshape(L, M)
        beta[kn] = one_hot[kn]
        beta = beta.ravel()
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
    idx, sym = csparc_ref.map_indices(s, M, K)
    idx, sym = np.array(idx), np.array(sym)
    idx[kn], sym[kn] = known_idx[kn], ksym[kn]
    return idx, sym, t + 1, nmse, psi


def three_stage(y, W, L, M, n, K, Ab, Az, awgn_var, t_max, beta0, L_unp, c, bp_its=200, final_t_max=None, rtol=1e-6,
                phi_est_method=1):
    """One codeword through AMP -> BP -> AMP with the converged blocks' sections
    known.  Returns dict(idx2, sym2 first-pass MAP, idx3, sym3 final-pass MAP,
    app [mults, N], it [mults], known_idx, known_sym [L])."""
    from oracle import bp
    per = sum(cref.bits_of(M, K))
    st = cref.amp_soft(y, W, L, M, n, K, Ab, Az, awgn_var, t_max, rtol, phi_est_method)
    llr = llr_of_probs(cref.soft_probs(st, M, K)[L_unp:].reshape(-1)).reshape(-1, c.N)
    res = [bp.decode("sumprod2", blk, c.vdeg, c.cdeg, c.intrlv, bp_its) for blk in llr]
    app, it = np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32)
    words = amp_partial_ref.known_sections(app, it, bp_its, 1, app.shape[0], L, L_unp, per)[0]
    kidx, ksym = unpack_words(words, K)
    i3, s3 = amp_partial(y, W, L, M, n, K, Ab, Az, awgn_var, t_max if final_t_max is None else final_t_max, beta0,
                         kidx, ksym, rtol, phi_est_method)[:2]
    return dict(idx2=st["idx"], sym2=st["sym"], idx3=i3, sym3=s3, app=app, it=it, known_idx=kidx, known_sym=ksym)


def user_bits(idx, sym, app, L_unp, M, K, c):
    """User bits of one codeword: the bits of the unprotected sections' (idx,
    sym), then the systematic hard decisions of every BP block."""
    per = sum(cref.bits_of(M, K))
    unp = cref.word_bits(cref.section_words(idx[:L_unp], sym[:L_unp], K), per)
    return np.concatenate([unp, (app[:, :c.K] < 0).astype(np.int64).reshape(-1)])


def draw(c, L, M, K, L_unp, mults, B, rng):
    """CsparcConcatPipeline.make_batch's draws of user bits: (idx [B, L], sym [B, L], info [B * mults, K])."""
    logM, logK = cref.bits_of(M, K)
    per = logM + logK
    unp = rng.integers(0, 2, (B, L_unp * per))
    info = rng.integers(0, 2, (B * mults, c.K))
    cw = c.encode_batch(info).reshape(B, mults * c.N)
    bits = np.concatenate([unp, cw], axis=1).reshape(B, L, per).astype(np.int64)
    idx = (bits[:, :, :logM] @ (1 << np.arange(logM)[::-1])).astype(np.int32)
    sym = np.zeros((B, L), dtype=np.int32)
    if logK:
        sym = gray2bin(bits[:, :, logM:] @ (1 << np.arange(logK)[::-1])).astype(np.int32)
    return idx, sym, info


def point():
    """The operating point's design and batch, made once: dict(W, o0, o1, Ab, Az,
    c, idx, sym [B, L], info [B, K], beta0 [B, LM], Y [B, n])."""
    if not _point:
        from ldpc_sparc_amd import sparc
        from ldpc_sparc_amd.ldpc import code
        g = GEOM
        L, M, K, n = g["L"], g["M"], g["K"], g["n"]
        c = code(*g["ldpc"])
        W = np.array(g["P"])
        o0, o1 = sparc.generate_ordering(W, n, L * M, DESIGN_SEED, csparc=True)
        Ab, Az = csparc_ref.fft_operators(W, L, M, n, o0, o1)
        rng = np.random.default_rng(BATCH_SEED)
        idx, sym, info = draw(c, L, M, K, g["L_unp"], g["mults"], B_POINT, rng)
        beta0 = one_hots(idx, sym, M, K)
        x = np.stack([Ab(b0).reshape(n) for b0 in beta0])
        sd = np.sqrt(VAR / 2)
        Y = x + sd * rng.standard_normal(x.shape) + 1j * (sd * rng.standard_normal(x.shape))
        _point.update(W=W, o0=o0, o1=o1, Ab=Ab, Az=Az, c=c, idx=idx, sym=sym, info=info, beta0=beta0, Y=Y)
    return _point


def mixed_known(true_idx, true_sym, L_unp, M, K, seed):
    """A known set per codeword of a batch [B, L] (B >= 5): codeword 0 none known;
    1 every protected section known; 2 the same with one wrong location; 3 the
    same with one wrong symbol (K = 1: another wrong location); the others a
    random subset of all sections, another one per codeword.  Returns
    (known_idx, known_sym)."""
    rng = np.random.RandomState(seed)
    B, L = true_idx.shape
    kidx = np.full((B, L), -1, dtype=np.int32)
    ksym = np.zeros((B, L), dtype=np.int32)
    for b in (1, 2, 3):
        kidx[b, L_unp:], ksym[b, L_unp:] = true_idx[b, L_unp:], true_sym[b, L_unp:]
    kidx[2, L_unp + 3] = (true_idx[2, L_unp + 3] + 1) % M
    if K > 1:
        ksym[3, L_unp + 1] = (true_sym[3, L_unp + 1] + 1) % K
    else:
        kidx[3, L_unp + 1] = (true_idx[3, L_unp + 1] + M // 2) % M
    for b in range(4, B):
        pick = rng.rand(L) < 0.25 + 0.5 * rng.rand()
        kidx[b, pick], ksym[b, pick] = true_idx[b, pick], true_sym[b, pick]
    return kidx, ksym
