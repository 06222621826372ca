"""The yardstick of the AMP decode with known sections (sg_amp_decode_partial*)
and of the three-stage concatenated decoder AMP -> BP -> AMP
(pipeline.DctConcat3Pipeline): NumPy restatements per codeword on
oracle.sparc_ref's DCT operators and estimators, and the geometry and
operating point the tests share.

amp_partial is oracle.sparc_ref.amp (sparc.py:883-999, W of ndim 0 or 1) with
two differences: the denoiser of a known section returns the one-hot of its
index, and the start is beta0 = the known one-hots, z0 = y - Ab(beta0), with
psi0_c the share of unknown sections of column block c in the place of 1
(gamma0 = W psi0, or dot(W, psi0) / Lc).  With no known section every
operation is sparc_ref.amp's, in its order.

known_sections restates sg_concat_known_sections_device; three_stage composes
dct_concat_ref's AMP -> LLR -> BP with both."""
import numpy as np

import dct_concat_ref as ref
from oracle import bp, sparc_ref

# ---- the geometry: 36 unprotected + 108 protected sections of M = 64; the protected ones hold one 802.11n r1/2
# z = 27 block (648 bits).  R_sparc = 1.0, P = 15; a quarter of the sections is left to the final pass.
GEOM = dict(L=144, M=64, n=864, P=15.0, L_unp=36, mults=1, ldpc=("802.11n", "1/2", 27))
# ---- the operating point of the value test (chosen on the CPU, tests/test_amp_partial_host.py): flat design of
# seed DESIGN_SEED, a batch of B_POINT codewords drawn as ConcatPipeline.make_batch draws them from
# default_rng(BATCH_SEED), noise variance VAR (known to the decoder), t_max = 25, 200 BP iterations
DESIGN_SEED, BATCH_SEED, B_POINT, VAR = 2, 11, 8, 4.0

_point = {}


def point():
    """The operating point's design and batch, made once: dict(W, o0, o1, Ab, Az,
    c, idx [B, L], info [B, K], beta0 [B, LM], Y [B, n])."""
    if not _point:
        from ldpc_sparc_amd.ldpc import code
        g = GEOM
        L, M, n = g["L"], g["M"], g["n"]
        c = code(*g["ldpc"])
        W, o0, o1 = ref.flat_design(L, M, n, g["P"], DESIGN_SEED)
        Ab, Az = sparc_ref.dct_operators(W, L, M, n, o0, o1)
        rng = np.random.default_rng(BATCH_SEED)
        idx, info = draw(c, L, M, g["L_unp"], g["mults"], B_POINT, rng)
        beta0 = np.zeros((B_POINT, L * M))
        beta0[np.arange(B_POINT)[:, None], np.arange(L) * M + idx] = 1
        Y = np.stack([Ab(b0) for b0 in beta0]) + np.sqrt(VAR) * rng.standard_normal((B_POINT, n))
        _point.update(W=W, o0=o0, o1=o1, Ab=Ab, Az=Az, c=c, idx=idx, info=info, beta0=beta0, Y=Y)
    return _point


def amp_partial(y, W, L, M, n, awgn_var, t_max, Ab, Az, beta0, known, rtol=1e-6, phi_method=1):
    """known [L]: index in [0, M) or -1.  Returns (map_idx [L], t_final, nmse,
    psi, beta_map [LM]) -- beta_map, t_final, nmse, psi as sparc_ref.amp."""
    W = np.asarray(W, dtype=float)
    assert W.ndim <= 1
    known = np.asarray(known)
    kn = np.flatnonzero((known >= 0) & (known < M))
    one_hot = np.zeros((L, M))
    one_hot[kn, known[kn]] = 1
    unknown = np.ones(L)
    unknown[kn] = 0
    beta = one_hot.ravel().copy()
    z = y - Ab(beta)
    atol = 2 * np.finfo(np.float64).resolution
    if W.ndim == 0:
        Lc = 1
        psi = unknown.sum() / L
        gamma = W * psi
        nmse = np.ones(t_max)
    else:
        Lc = W.shape[-1]
        Mc = L * M // Lc
        psi = unknown.reshape(Lc, -1).sum(axis=1) / (L / Lc)
        gamma = np.dot(W, psi) / Lc
        nmse = np.ones((t_max, Lc))
    phi = None
    for t in range(t_max - 1):
        if t > 0:
            psi_prev = np.copy(psi)
            phi_prev = np.copy(phi)
            gamma = W * psi if W.ndim == 0 else np.dot(W, psi) / Lc
            b = gamma / phi_prev
            z = y - Ab(beta) + b * z
        phi = awgn_var + gamma if phi_method == 1 else (np.abs(z) ** 2).mean()
        tau = (L * phi / n) / W
        tau_use = tau if W.ndim == 0 else tau.repeat(Mc)
        s = beta + tau_use * Az(z / phi)
        beta = sparc_ref.mmse_estimator(s, tau_use, M).reshape(L, M)
        beta[kn] = one_hot[kn]
        beta = beta.ravel()
        if W.ndim == 0:
            psi = 1 - (np.abs(beta) ** 2).sum() / L
            nmse[t + 1] = (np.abs(beta - beta0) ** 2).sum() / L
        else:
            psi = 1 - (np.abs(beta) ** 2).reshape(Lc, -1).sum(axis=1) / (L / Lc)
            nmse[t + 1] = (np.abs(beta - beta0) ** 2).reshape(Lc, -1).sum(axis=1) / (L / Lc)
        if t > 0 and np.allclose(psi, psi_prev, rtol, atol=atol):
            nmse[t:] = nmse[t]
            break
    bmap = sparc_ref.map_estimator(s, M).reshape(L, M)
    bmap[kn] = one_hot[kn]
    return np.argmax(bmap, 1).astype(np.int32), t + 1, nmse, psi, bmap.ravel()


def known_sections(app, it, max_it, B, mults, L, L_unp, logM):
    """app [B * mults, N] BP output, it [B * mults] -> known [B, L]: -1 for the
    unprotected sections and for a protected section any of whose bits lies in
    a block with it >= max_it, else the MSB-first index of its hard decisions."""
    app, it = np.asarray(app), np.asarray(it).reshape(B, mults)
    N = app.shape[1]
    bits = (app.reshape(B, mults * N) < 0).astype(np.int64)
    out = np.full((B, L), -1, dtype=np.int32)
    for b in range(B):
        for l in range(L_unp, L):
            q = (l - L_unp) * logM + np.arange(logM)
            if np.all(it[b, q // N] < max_it):
                out[b, l] = int(bits[b, q] @ (1 << np.arange(logM)[::-1]))
    return out


def two_stage(y, W, L, M, n, awgn_var, t_max, Ab, Az, beta0, L_unp, c, bp_its=200, rtol=1e-6, phi_method=1):
    """dct_concat_ref's composition for one codeword, keeping what the third
    stage needs: (map_idx [L] of the first AMP, app [mults, N], it [mults])."""
    beta, mp, _ = ref.amp_soft(y, W, L, M, n, awgn_var, t_max, Ab, Az, beta0, rtol, phi_method)
    llr = ref.llr_of_probs(ref.bit_probs(beta, L, M, L_unp)).reshape(-1, c.N)
    res = [bp.decode("sumprod2", blk, c.vdeg, c.cdeg, c.intrlv, bp_its) for blk in llr]
    return mp.astype(np.int32), np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32)


def three_stage(y, W, L, M, n, awgn_var, t_max, Ab, Az, beta0, L_unp, c, bp_its=200, final_t_max=None, rtol=1e-6,
                phi_method=1):
    """One codeword through AMP -> BP -> AMP with the converged blocks' sections
    known.  Returns dict(map2 [L] first-pass MAP, map3 [L] final-pass MAP, app,
    it, known [L])."""
    mp, app, it = two_stage(y, W, L, M, n, awgn_var, t_max, Ab, Az, beta0, L_unp, c, bp_its, rtol, phi_method)
    logM = int(np.log2(M))
    known = known_sections(app, it, bp_its, 1, app.shape[0], L, L_unp, logM)[0]
    m3 = amp_partial(y, W, L, M, n, awgn_var, t_max if final_t_max is None else final_t_max, Ab, Az, beta0, known,
                     rtol, phi_method)[0]
    return dict(map2=mp, map3=m3, app=app, it=it, known=known)


def counters(map_idx, true_idx, app, info, L_unp, logM, K):
    """The five counters of sg_concat_count_errors_device for one codeword."""
    unp = int(sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(map_idx[:L_unp], true_idx[:L_unp])))
    prot = int(np.sum((app[:, :K] < 0).astype(np.int64).reshape(-1) != np.asarray(info).reshape(-1)))
    return np.array([1, unp + prot, int(unp + prot > 0), unp, prot], dtype=np.int64)


def draw(c, L, M, L_unp, mults, B, rng):
    """ConcatPipeline.make_batch's draws of user bits: (idx [B, L], info [B * mults, K])."""
    logM = int(np.log2(M))
    unp = rng.integers(0, 2, (B, L_unp * logM))
    info = rng.integers(0, 2, (B * mults, c.K))
    cw = c.encode_batch(info).reshape(B, mults * c.N)
    bits = np.concatenate([unp, cw], axis=1).reshape(B, L, logM)
    idx = (bits.astype(np.int64) @ (1 << np.arange(logM)[::-1])).astype(np.int32)
    return idx, info


def mixed_known(true, L_unp, M, seed):
    """A known set per codeword of a batch true [B, L] (B >= 4): codeword 0 none
    known; 1 every protected section known; 2 the same with one wrong index; the
    others a random subset of all sections, another one per codeword."""
    rng = np.random.RandomState(seed)
    B, L = true.shape
    known = np.full((B, L), -1, dtype=np.int32)
    known[1, L_unp:] = true[1, L_unp:]
    known[2, L_unp:] = true[2, L_unp:]
    known[2, L_unp + 3] = (true[2, L_unp + 3] + 1) % M
    for b in range(3, B):
        pick = rng.rand(L) < 0.25 + 0.5 * rng.rand()
        known[b, pick] = true[b, pick]
    return known
