"""The section-size sweep's geometries, shared by tests/test_section_sizes_host.py
(the oracle alone: are the operating points what the GPU test needs?) and
tests/test_section_sizes_gpu.py (both DCT engines and both LLR kernels against
the oracle at every one of them).

Every case: P = 15, R = 1.0, n = round(L log2 M), awgn_var = 1, noise sigma = 1,
a batch of B = 3 codewords, design seed 3, batch seed 11; the oracle is
oracle.sparc_ref.amp at rtol 1e-6 (tests/dct_concat_ref.py composes its soft
output).  The section sizes reach every instantiation that dispatches on M:

    M       reg_llr_kernel VMAX   eta_kernel EPL   glue_llr_kernel trips
    2..64          1                   1                  1
    128            8 (V = 2)           2                  2
    256            8 (V = 4)           4                  4
    512            8 (V = 8)           8                  8
    1024          32 (V = 16)         16                 16
    2048          32 (V = 32)         32                 32
    4096       refused            refused at plan creation

The oracle's result per (case, t_max) is computed once per process and never
modified (arrays are returned read-only)."""
import numpy as np

import dct_concat_ref as ref
from oracle import sparc_ref

P, VAR, SIGMA, B = 15.0, 1.0, 1.0, 3
DESIGN_SEED, BATCH_SEED = 3, 11
T_SOFT, T_FULL = 3, 25

# name: (L, M, column blocks; 0 = flat design)
GEOMETRIES = {
    "m2": (64, 2, 0),
    "m4": (64, 4, 0),
    "m8": (32, 8, 0),
    "m32": (32, 32, 0),
    "m64": (32, 64, 0),
    "m128": (32, 128, 0),
    "m256": (16, 256, 0),
    "m512": (16, 512, 0),
    "m1024": (16, 1024, 0),
    "m2048": (8, 2048, 0),
    "m256pa": (16, 256, 4),  # power allocation over four column blocks of four sections, each with its own tau
}
UPPER = (8, 4096, 0)  # the upper bound's geometry: decoded by the regular engine only, no soft output
NAMES = list(GEOMETRIES)
# M = 2 and M = 4 stall (the oracle runs out of iterations at t_max = 25): the soft leg only
CONVERGING = [k for k in NAMES if GEOMETRIES[k][1] >= 8]


def n_of(L, M):
    return int(round(L * np.log2(M)))


class Case:
    """One geometry: design, CPU operators, the batch, the oracle per t_max."""

    def __init__(self, name, L, M, blocks):
        self.name, self.L, self.M, self.blocks = name, L, M, blocks
        self.n = n_of(L, M)
        self.logM = int(np.log2(M))
        if blocks:
            self.W, self.o0, self.o1 = ref.pa_design(L, M, self.n, P, DESIGN_SEED, awgn_var=VAR, B=blocks, R=1.0)
        else:
            self.W, self.o0, self.o1 = ref.flat_design(L, M, self.n, P, DESIGN_SEED)
        self.Ab, self.Az = sparc_ref.dct_operators(self.W, L, M, self.n, self.o0, self.o1)
        self.true, self.beta0, self.Y = ref.batch(self.Ab, L, M, self.n, B, SIGMA, BATCH_SEED)
        self._oracle = {}

    def oracle_of(self, Y, t_max):
        """The oracle on received words Y [b, n] (transmitted: the batch's first b
        codewords): dict of probs [b, L log2 M] = P(bit = 0) MSB first, map [b, L],
        t_final [b], nmse [b, t_max, Lc]."""
        probs, mp, tf, nm = [], [], [], []
        for b, y in enumerate(Y):
            last = {}

            def keep(t, st):
                last["beta"] = np.array(st["beta"], dtype=np.float64)

            bmap, t, nmse, _ = sparc_ref.amp(y, self.W, self.L, self.M, self.n, VAR, t_max, self.Ab, self.Az,
                                             self.beta0[b], 1e-6, 1, trace=keep)
            probs.append(ref.bit_probs(last["beta"], self.L, self.M))
            mp.append(np.argmax(bmap.reshape(self.L, self.M), 1))
            tf.append(int(t))
            nm.append(np.asarray(nmse, dtype=np.float64).reshape(t_max, -1))
        out = dict(probs=np.stack(probs), map=np.stack(mp).astype(np.int32), t_final=np.array(tf, dtype=np.int32),
                   nmse=np.stack(nm))
        for v in out.values():
            v.setflags(write=False)
        return out

    def oracle(self, t_max):
        if t_max not in self._oracle:
            self._oracle[t_max] = self.oracle_of(self.Y, t_max)
        return self._oracle[t_max]

    def soft_counts(self):
        """Bit probabilities inside (0.01, 0.99) at T_SOFT: (over the batch, of
        those in index bits >= 6 over the batch, the same of the last codeword)."""
        p = self.oracle(T_SOFT)["probs"].reshape(B, self.L, self.logM)
        soft = (p > 0.01) & (p < 0.99)
        hi = soft[:, :, :max(self.logM - 6, 0)]  # MSB first: positions 0 .. logM - 7 are bits logM - 1 .. 6
        return int(soft.sum()), int(hi.sum()), int(hi[-1].sum())


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name, *(UPPER if name == "m4096" else GEOMETRIES[name]))
    return _cases[name]
