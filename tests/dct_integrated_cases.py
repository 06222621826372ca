"""Shared inputs of the integrated AMP <-> BP decoder tests on the sub-sampled
DCT design (test_dct_integrated_host.py, test_dct_integrated_gpu.py).

Every case is generated from seeds with numpy alone: the orders by
RandomState(design seed) shuffles of arange(1, w) (sub_dct, sparc.py:735-775),
the information bits and the noise of each codeword of the batch from its own
default_rng(seed), the codewords by code.encode_batch, the section index of a
codeword from its MSB-first bits.  P = 15, sigma^2 = 1, t_max = 6 throughout.
The seeds are chosen so that the operating points of DECODES hold in the oracle
(test_dct_integrated_host.py re-establishes them): the naive and the posterior
decoders diverge on a good share of the noise draws even where AMP alone
decodes, so a batch of three arbitrary draws seldom decodes in all four modes.

The flat DCT design written out as a matrix is
    A[i, j] = sqrt(2 / n) cos(pi (2 order1[j] + 1) order0[i] / (2 w)),
which is Ab(e_j) / sqrt(n P / L) of the operator: sqrt(w) dct(., norm='ortho')
has the entries sqrt(2) cos(...) away from row 0, and row 0 is never sampled.
oracle/integrated_ref.decode takes that matrix, so the oracle needs no change.
"""
import functools

import numpy as np

P, SIGMA2, T_MAX = 15.0, 1.0, 6
B = 3  # codewords per batch, independent noise
ORACLE_MODES = ("naive", "naivepost", "integ", "integpost")
API_MODES = {"naive": "naive", "naivepost": "naive_posteriors", "integ": "integrated",
             "integpost": "integrated_posteriors"}

# name -> (LDPC code, L, M, n, design seed, codeword seeds); the section-kernel path each one takes:
#   A  VMAX 1, two LDPC blocks per codeword      B  VMAX 8, two blocks
#   C  VMAX 32                                   D  M = 4: lanes >= M idle
#   E  rate too high to decode (tau^2 stays up)
CASES = {
    "A": (("802.16", "1/2", 3), 24, 64, 144, 1, (0, 1, 2)),
    "B": (("802.16", "1/2", 6), 32, 512, 360, 4, (4, 6, 21)),
    "C": (("802.16", "1/2", 11), 24, 2048, 330, 5, (5, 7, 16)),
    "D": (("802.16", "1/2", 3), 36, 4, 144, 6, (0, 1, 2)),
    "E": (("802.16", "1/2", 6), 16, 512, 120, 3, (0, 2, 3)),
}
# modes in which every codeword of the batch decodes to the transmitted bits (the oracle, double precision)
DECODES = {"A": ("naivepost", "integ"), "B": ORACLE_MODES, "C": ORACLE_MODES, "D": ORACLE_MODES, "E": ()}


def transform_size(n, LM):
    return 2 ** int(np.ceil(np.log2(max(n + 1, LM + 1))))


def orders(n, LM, seed):
    w = transform_size(n, LM)
    rows = np.arange(1, w, dtype=np.uint32)
    cols = np.arange(1, w, dtype=np.uint32)
    rs = np.random.RandomState(seed)
    rs.shuffle(rows)
    rs.shuffle(cols)
    return rows[:n].copy(), cols[:LM].copy()


def explicit_matrix(n, LM, order0, order1):
    w = transform_size(n, LM)
    # (2 order1 + 1) order0 reduced mod 4w in integers (the cosine's period), so that the argument is exact
    k = ((2 * order1.astype(np.int64)[None, :] + 1) * order0.astype(np.int64)[:, None]) % (4 * w)
    return np.sqrt(2.0 / n) * np.cos(np.pi * k / (2.0 * w))


class Case:
    pass


def codeword(c, seed):
    """One codeword of case c from default_rng(seed): (information bits [nblk, K], section indices [L], y [n])."""
    rng = np.random.default_rng(seed)
    info = rng.integers(0, 2, (c.nblk, c.K)).astype(np.uint8)
    cw = np.asarray(c.code.encode_batch(info)).reshape(c.L, c.logM)
    idx = (cw.astype(np.int64) @ (1 << np.arange(c.logM)[::-1])).astype(np.int32)
    x = c.snp * c.A[:, np.arange(c.L) * c.M + idx].sum(axis=1)
    return info, idx, x + np.sqrt(SIGMA2) * rng.standard_normal(c.n)


@functools.lru_cache(maxsize=None)
def build(name):
    """The case's design, codewords and received words (cached; treat as read-only)."""
    from ldpc_sparc_amd.ldpc import code
    ldpc, L, M, n, seed, cw_seeds = CASES[name]
    assert len(cw_seeds) == B
    c = Case()
    c.name, c.L, c.M, c.n, c.seed = name, L, M, n, seed
    c.code = code(*ldpc)
    c.N, c.K = c.code.N, c.code.K
    c.logM = int(np.log2(M))
    assert (L * c.logM) % c.N == 0
    c.nblk = L * c.logM // c.N
    c.graph = (c.code.vdeg, c.code.cdeg, c.code.intrlv)
    c.snp = float(np.sqrt(n * P / L))
    c.order0, c.order1 = orders(n, L * M, seed)
    c.A = explicit_matrix(n, L * M, c.order0, c.order1)
    words = [codeword(c, s) for s in cw_seeds]
    c.info = np.concatenate([w[0] for w in words])  # [B nblk, K]
    c.idx = np.stack([w[1] for w in words])
    c.Y = np.stack([w[2] for w in words])
    c.bits_in = c.info.reshape(B, c.nblk * c.K)
    for a in (c.A, c.Y, c.info, c.idx, c.bits_in, c.order0, c.order1):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def oracle(name, mode):
    """oracle/integrated_ref.decode of every codeword of the case: (bits [B, nblk K], tau^2 [B, T_MAX])."""
    from oracle import integrated_ref
    c = build(name)
    bits, taus = [], []
    for b in range(B):
        bo, to = integrated_ref.decode(mode, c.Y[b], c.A, P, c.L, c.M, c.graph, c.N, c.K, T_MAX)
        bits.append(np.asarray(bo, dtype=np.uint8))
        taus.append(np.asarray(to, dtype=np.float64))
    bits, taus = np.stack(bits), np.stack(taus)
    bits.setflags(write=False)
    taus.setflags(write=False)
    return bits, taus


def operator(c):
    """The case's design as a sparc.DesignOperator (flat, W = P)."""
    from ldpc_sparc_amd import sparc
    return sparc.DesignOperator(np.array(P), c.L, c.M, c.n, c.order0, c.order1)
