"""Inputs of the layered-BP tests and their restatement outputs, computed once
per session (tests/bp_layered_ref.py) and shared, read-only, by the tests."""
import functools

import numpy as np

import bp_layered_ref as lr
from ldpc_sparc_amd.ldpc import code

B = 37        # not a multiple of anything the kernel groups by
MAX_ITS = (1, 5, 50)

# (standard, rate, z): Eb/N0 dB of the min-sum cases, of the sumprod2 cases.  Chosen on the CPU restatement so
# that at max_it = 50 most of the 37 codewords stop early and some reach max_it (float64 and float32 alike):
# codewords at max_it, min-sum / sumprod2, in the order below: 6 / 2, 3 / 2, 4 / 3, 5 / 1, 10 / 2 -- so the
# restatement stops at least 34 of 37 (91 %) of every sumprod2 batch.
CODES = {
    ("802.11n", "1/2", 27): (1.8, 1.8),    # less than one wave per layer
    ("802.11n", "5/6", 27): (3.6, 3.6),    # check degree above 8
    ("802.11n", "1/2", 81): (1.8, 1.07),   # a layer spanning two waves with a ragged tail
    ("802.16", "1/2", 24): (1.8, 1.8),
    ("802.16", "1/2", 96): (1.4, 1.4),     # the largest LDS image the flooding tests use
}
SPECS = list(CODES)


def awgn_llrs(c, n, ebn0, seed):
    """n random codewords over BPSK/AWGN at Eb/N0 dB: (bits, channel LLRs float64)."""
    rng = np.random.default_rng(seed)
    X = c.encode_batch(rng.integers(0, 2, (n, c.K)))
    s2 = 1 / (2 * (c.K / c.N) * 10 ** (ebn0 / 10))
    return X, 2 * ((1 - 2 * X) + np.sqrt(s2) * rng.standard_normal(X.shape)) / s2


@functools.lru_cache(maxsize=None)
def get_code(spec):
    return code(*spec)


@functools.lru_cache(maxsize=None)
def batch(spec, dectype):
    """(bits, channel LLRs) of a code's batch for a decoder type; read-only."""
    c = get_code(spec)
    X, ch = awgn_llrs(c, B, CODES[spec][dectype == "sumprod2"], 100 + SPECS.index(spec))
    assert X.any(axis=1).all()  # never the all-zero word
    ch.setflags(write=False)
    return X, ch


@functools.lru_cache(maxsize=None)
def reference(spec, dectype, dtype, max_it):
    """The restatement's (app, it) for batch(spec, dectype); read-only."""
    c = get_code(spec)
    app, it = lr.layered(c.vdeg, c.cdeg, c.intrlv, batch(spec, dectype)[1], c.z, max_it, dectype, 0.7,
                         {"f64": np.float64, "f32": np.float32}[dtype])
    app.setflags(write=False)
    it.setflags(write=False)
    return app, it
