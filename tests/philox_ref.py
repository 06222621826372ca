"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the device Monte-Carlo
generator: Philox4x32-10 (Salmon et al., SC'11; csrc/philox.hpp), its
Box-Muller normals, and the counter layouts of the kernels that draw from it
(csrc/channel.hip: rng_bits_kernel, awgn_kernel, bpsk_llr_kernel;
csrc/dense.hip: gen_A_kernel).  This module is the definition of the
throughput-mode stream: the kernels are pinned to it, not the other way round.

Every routine is vectorised over counters in uint64 arithmetic and evaluates
the floating-point part in float64.

Counter and key of one Philox call, as the kernels form them:

    bits   c = (j // 128, b, stream & 2^32-1, stream >> 32)   key = (seed_lo ^ 0xB175, seed_hi)
    noise  c = (i // 2,   b, stream & 2^32-1, stream >> 32)   key = (seed_lo ^ 0x0A1E, seed_hi)
    design c = (e // 4 & 2^32-1, e // 4 >> 32, 0x5eed5eed, 0) key = (seed_lo, seed_hi)

with b the row (codeword) of the call, j / i / e the bit / sample / matrix
element.  Bit j of a row is bit j % 32 of output word (j % 128) // 32; samples
2q and 2q + 1 of a row are the two normals of call q; elements 4q .. 4q + 3
of the row-major design are the two Box-Muller pairs of words (0, 1), (2, 3).

Normals (philox_normal2): k1 = c0 << 21 | c1 >> 11, k2 = c2 << 21 | c3 >> 11,

    u1 = (k1 + 1) 2^-53  in (0, 1],   u2 = k2 2^-53  in [0, 1),
    g0 = sqrt(-2 log u1) cos(2 pi u2),  g1 = sqrt(-2 log u1) sin(2 pi u2).

u1 does reach 1 (k1 = 2^53 - 1), where both normals are 0: the header's
literal 9007199254740993.0 is not a double and reads as 2^53.  cos and sin
are those of sincospi(2 u2): the argument is reduced in units of pi (a
quarter-turn index and a remainder in [-1/4, 1/4]) before the multiplication
by pi, so the quadrant points give exact 0 and +-1 and the relative error
stays a few ulps next to the zeros.
"""
import numpy as np

MASK32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
BITS_DOMAIN, NOISE_DOMAIN = 0xB175, 0x0A1E
DESIGN_TAG = 0x5EED5EED


def _u64(a):
    return np.asarray(a, dtype=np.uint64) & MASK32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 on the counters (c0, c1, c2, c3) with the key
    (k0, k1); the arguments broadcast.  Returns four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(a) for a in (c0, c1, c2, c3, k0, k1)])
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2  # 32 x 32 -> 64 bits, no overflow
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & MASK32, (p0 >> sh) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniforms53(c):
    """The two 53-bit integers (k1, k2) of one Philox output, as uint64."""
    c0, c1, c2, c3 = (_u64(w) for w in c)
    return (c0 << np.uint64(21)) ^ (c1 >> np.uint64(11)), (c2 << np.uint64(21)) ^ (c3 >> np.uint64(11))


def sincospi2(u2):
    """(sin, cos) of 2 pi u2 for float64 u2 in [0, 1), reduced in units of pi."""
    t = 2.0 * np.asarray(u2, dtype=np.float64)  # exact; the angle is pi t, t in [0, 2)
    q = np.rint(2.0 * t)                        # quarter turns, 0 .. 4
    rem = t - 0.5 * q                           # exact, in [-1/4, 1/4]
    s, c = np.sin(np.pi * rem), np.cos(np.pi * rem)
    q = q.astype(np.int64) & 3
    sn = np.choose(q, [s, c, -s, -c])
    cs = np.choose(q, [c, -s, -c, s])
    return sn, cs


def normal2(c):
    """The two standard normals (g0, g1) of one Philox output c = (c0..c3)."""
    k1, k2 = uniforms53(c)
    u1 = (k1.astype(np.float64) + 1.0) * 2.0 ** -53  # every step exact
    u2 = k2.astype(np.float64) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    sn, cs = sincospi2(u2)
    return r * cs, r * sn


def _split(v):
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError("seed and stream are unsigned 64-bit")
    return v & 0xFFFFFFFF, v >> 32


def _draw(seed, stream, B, ncalls, domain):
    (s_lo, s_hi), (t_lo, t_hi) = _split(seed), _split(stream)
    q = np.arange(ncalls, dtype=np.uint64)[None, :]
    b = np.arange(B, dtype=np.uint64)[:, None]
    return philox4x32_10(q, b, t_lo, t_hi, s_lo ^ domain, s_hi)


def rng_bits(seed, stream, B, nbits):
    """sg_rng_bits_device: uint8 [B, nbits] of 0 / 1."""
    nblk = (nbits + 127) // 128
    words = np.stack(_draw(seed, stream, B, nblk, BITS_DOMAIN), axis=-1)  # [B, nblk, 4]
    raw = np.ascontiguousarray(words.astype("<u4")).view(np.uint8).reshape(B, nblk * 16)
    return np.ascontiguousarray(np.unpackbits(raw, axis=1, bitorder="little")[:, :nbits])


def awgn_normals(seed, stream, B, n):
    """The float64 normals g [B, n] that awgn_kernel and bpsk_llr_kernel add."""
    nq = (n + 1) // 2
    g0, g1 = normal2(_draw(seed, stream, B, nq, NOISE_DOMAIN))
    return np.ascontiguousarray(np.stack([g0, g1], axis=-1).reshape(B, 2 * nq)[:, :n])


def awgn(x, sigma, seed, stream):
    """sg_awgn_device before the rounding to the output type: x + sigma g."""
    x = np.asarray(x)
    return x.astype(np.float64) + float(sigma) * awgn_normals(seed, stream, *x.shape)


def bpsk_llr(cw, sigma2, seed, stream):
    """sg_bpsk_awgn_llr_device before the rounding to the output type:
    (2 / sigma2) ((1 - 2 cw) + sqrt(sigma2) g) on the bytes of cw as they are."""
    cw = np.asarray(cw)
    g = awgn_normals(seed, stream, *cw.shape)
    return (2.0 / sigma2) * ((1.0 - 2.0 * cw.astype(np.float64)) + np.sqrt(sigma2) * g)


def gen_A_scale(n):
    """The scale of dense_launch_gen_A: entries are N(0, 1 / n)."""
    return 1.0 / np.sqrt(float(n))


def gen_A_float(seed, n, LM):
    """gen_A_kernel's float32 intermediate [n, LM]: unit normals from 32-bit
    uniforms, u1 = (c + 1) / (2^32 + 1), u2 = c / 2^32, cos / sin of the
    double product 2 pi u2, each normal rounded to float32."""
    total = n * LM
    s_lo, s_hi = _split(seed)
    q = np.arange((total + 3) // 4, dtype=np.uint64)
    c = philox4x32_10(q & MASK32, q >> np.uint64(32), DESIGN_TAG, 0, s_lo, s_hi)
    out = np.empty((len(q), 4), dtype=np.float32)
    for h in range(2):
        u1 = (c[2 * h].astype(np.float64) + 1.0) / (4294967296.0 + 1.0)
        u2 = c[2 * h + 1].astype(np.float64) / 4294967296.0
        r = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * h] = r * np.cos(2.0 * np.pi * u2)
        out[:, 2 * h + 1] = r * np.sin(2.0 * np.pi * u2)
    return out.reshape(-1)[:total].reshape(n, LM)


def gen_A(seed, n, LM):
    """The random design of sg_dense_plan_create_random as float64 [n, LM]:
    the float32 intermediate times the scale, the product in double (the f32
    plan rounds it to float32 once more)."""
    return gen_A_float(seed, n, LM).astype(np.float64) * gen_A_scale(n)
