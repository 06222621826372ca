"""The yardstick of the DCT-design concatenated decoder, composed per codeword
from the CPU restatements under oracle/: sparc_ref.amp (its last iteration's
beta through `trace`, and its MAP output) -> sparc_ref.beta_to_bit_probs(beta,
L, M, 1.0) -> ldpc_bp's clip and log in NumPy -> oracle.bp.decode.  Shared by
tests/test_dct_concat_gpu.py and tests/test_dct_concat_host.py; also the small
geometries those tests use."""
import numpy as np

from oracle import bp, sparc_ref

EPS = 1e-15  # ldpc_bp's clip (sparc_new.py:1167)


def amp_soft(y, W, L, M, n, awgn_var, t_max, Ab, Az, beta0, rtol=1e-6, phi_method=1):
    """(beta of the last iteration, MAP section indices, t_final) of the CPU AMP."""
    last = {}

    def keep(t, st):
        last["beta"] = np.array(st["beta"], dtype=np.float64)

    bmap, tf, _, _ = sparc_ref.amp(y, W, L, M, n, awgn_var, t_max, Ab, Az, beta0, rtol, phi_method, trace=keep)
    return last["beta"], np.argmax(bmap.reshape(L, M), 1), int(tf)


def bit_probs(beta, L, M, l0=0, nl=None):
    """P(bit = 0), MSB first, of sections [l0, l0 + nl): [nl * log2 M]."""
    logM = int(np.log2(M))
    nl = L - l0 if nl is None else nl
    return sparc_ref.beta_to_bit_probs(beta, L, M, 1.0).reshape(L, logM)[l0:l0 + nl].reshape(-1)


def llr_of_probs(p):
    pc = np.clip(np.asarray(p, dtype=np.float64), EPS, 1 - EPS)
    return np.log(pc) - np.log(1 - pc)


def decode_user_bits(beta, map_idx, L, M, L_unp, c, bp_its=200):
    """User bits of one codeword: the MAP bits of the unprotected sections, then
    the systematic hard decisions of sumprod2 on every LDPC block of the
    protected sections (sparc_new.py:53-82 with the DCT-design AMP in front)."""
    logM = int(np.log2(M))
    unp = ((map_idx[:L_unp, None] >> np.arange(logM)[::-1]) & 1).reshape(-1)
    llr = llr_of_probs(bit_probs(beta, L, M, L_unp)).reshape(-1, c.N)
    out = [unp]
    for blk in llr:
        app, _ = bp.decode("sumprod2", blk, c.vdeg, c.cdeg, c.intrlv, bp_its)
        out.append((app[:c.K] < 0).astype(np.int64))
    return np.concatenate(out)


def user_bits_truth(idx_b, info_b, L_unp, logM):
    unp = ((idx_b[:L_unp, None] >> np.arange(logM)[::-1]) & 1).reshape(-1)
    return np.concatenate([unp, np.asarray(info_b).reshape(-1)])


# ---- the small concatenated geometry: 4 unprotected + 108 protected sections of M = 64 hold one 802.11n
# r1/2 z = 27 block (648 bits), R = 1.0, P = 15
SMALL = dict(L=112, M=64, n=672, P=15.0, L_unp=4, mults=1, ldpc=("802.11n", "1/2", 27))


def flat_design(L, M, n, P, seed):
    from ldpc_sparc_amd import sparc
    W = np.array(float(P))
    o0, o1 = sparc.generate_ordering(W, n, L * M, seed)
    return W, o0, o1


def pa_design(L, M, n, P, seed, awgn_var=1.0, B=4, R=1.0):
    """Power allocation over B column blocks (create_base_matrix, iterative allocation)."""
    from ldpc_sparc_amd import sparc
    W = sparc.create_base_matrix(P, power_allocated=True, awgn_var=awgn_var, B=B, R=R, R_PA_ratio=1.0)
    o0, o1 = sparc.generate_ordering(W, n, L * M // B, seed)
    return W, o0, o1


def batch(Ab, L, M, n, B, sigmas, seed):
    """B random codewords through the CPU design operator: (true indices [B, L],
    beta0 [B, LM], y [B, n]) with noise standard deviation sigmas[b]."""
    rng = np.random.RandomState(seed)
    true = rng.randint(0, M, (B, L))
    beta0 = np.zeros((B, L * M))
    beta0[np.arange(B)[:, None], np.arange(L) * M + true] = 1
    sig = np.broadcast_to(np.asarray(sigmas, dtype=np.float64), (B,))
    y = np.stack([Ab(beta0[b]) for b in range(B)]) + sig[:, None] * rng.randn(B, n)
    return true.astype(np.int32), beta0, y
