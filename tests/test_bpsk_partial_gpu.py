"""GPU tests of the real K = 2 AMP decode with known section words
(sg_amp_decode_bpsk_partial*, amp_oploop.hip) and of the three-stage
concatenated K = 2 decoder built on it (pipeline.DctBpskConcat3Pipeline).

The yardstick is tests/bpsk_partial_ref.py: amp_bpsk_ref.amp_bpsk with known
words, per codeword, and its composition with bpsk_concat_ref's AMP -> LLR ->
BP.  tests/test_bpsk_partial_host.py holds it against amp_bpsk and asserts,
on the restatement alone, that the cases below are stable.

Bars (those of test_bpsk_gpu.py and test_amp_partial_gpu.py for this loop): in
double precision words and t_final equal and nmse / psi at atol 1e-9 on every
codeword whose restatement moves by less than 1e-10 when the received values
move by one ulp (at most one of eight per case, two of eight at the pipeline's
operating points); in single precision the words of the codewords the
restatement decodes without a section error outside its given words, and nmse
at 1e-3 at t_max = 4.  With nothing known the outputs are the plain K = 2
decode's, byte for byte.

Every output buffer handed to the device entry carries a guard tail."""
import numpy as np
import pytest

import bpsk_concat_ref as cr
import bpsk_partial_ref as ref
import section_size_cases as ssc
from ldpc_sparc_amd import _native, montecarlo, sparc
from ldpc_sparc_amd.pipeline import DctBpskConcat3Pipeline, DctBpskConcatPipeline

pytestmark = pytest.mark.gpu

F64, F32 = _native.SG_F64, _native.SG_F32
ATOL = {F64: 1e-9, F32: 1e-3}
TAIL = 64

_ops = {}


def op_of(c):
    if id(c) not in _ops:
        _ops[id(c)] = sparc.DesignOperator(c.W, c.L, c.M, c.n, c.o0, c.o1)
    return _ops[id(c)]


def _guarded(shape, dtype, fill):
    host = np.full(int(np.prod(shape)) + TAIL, fill, dtype)
    return _native.DeviceBuffer.from_array(host), host


def device_decode(c, prec, t_max, known, rows=slice(None), phi_method=1, with_truth=True):
    """sg_amp_decode_bpsk_partial_device on rows of the case: (map_word, t_final, nmse, psi), after checking that
    nothing was written past any output."""
    op = op_of(c)
    dt = np.float64 if prec == F64 else np.float32
    Y, kn, tw = c.Y[rows], np.ascontiguousarray(known[rows], np.int32), np.ascontiguousarray(c.true[rows], np.int32)
    nb, Lc = len(Y), op.Lc
    d_y = _native.DeviceBuffer.from_array(np.ascontiguousarray(Y, dt))
    d_k, d_t = _native.DeviceBuffer.from_array(kn), _native.DeviceBuffer.from_array(tw)
    shapes = [((nb, c.L), np.int32, -7), ((nb,), np.int32, -7), ((nb, t_max, Lc), np.float64, -7.0),
              ((nb, Lc), np.float64, -7.0)]
    bufs = [_guarded(*s) for s in shapes]
    _native.check(_native.lib().sg_amp_decode_bpsk_partial_device(
        op.plan(prec), d_y.ptr, nb, d_k.ptr, d_t.ptr if with_truth else None, c.var, t_max, 1e-6, phi_method,
        bufs[0][0].ptr, bufs[1][0].ptr, bufs[2][0].ptr, bufs[3][0].ptr, None))
    _native.synchronize()
    out = []
    for (buf, host), (shape, _, fill) in zip(bufs, shapes):
        got = buf.download(host)
        assert np.all(got[-TAIL:] == fill), "written past the output"
        out.append(got[:-TAIL].reshape(shape).copy())
    return tuple(out)


def host_decode(c, prec, t_max, known, rows=slice(None), phi_method=1):
    return sparc.amp_decode_bpsk_partial_batch(c.Y[rows], op_of(c), known[rows], c.var, t_max, 1e-6, phi_method,
                                               c.true[rows], prec)


# ---------------------------------------------------------------- against the restatement

@pytest.mark.parametrize("name,phi_method", ref.VS_NAMES)
def test_f64_vs_restatement(name, phi_method):
    c = ref.case(name)
    mp_r, tf_r, nm_r, ps_r = c.restatement(c.t_max, phi_method)
    stable = c.moves(c.t_max, phi_method) < 1e-10
    assert np.count_nonzero(~stable) <= 1, stable
    mp, tf, nm, ps = device_decode(c, F64, c.t_max, c.known, phi_method=phi_method)
    err = np.maximum(np.max(np.abs(nm - nm_r), axis=(1, 2)), np.max(np.abs(ps - ps_r), axis=1))
    print(f"{name} phi {phi_method}: t_final {tf.tolist()}, stable {stable.tolist()}, max |nmse, psi - ref| {err}")
    assert np.array_equal(tf[stable], tf_r[stable])
    assert np.array_equal(mp[stable], mp_r[stable])
    np.testing.assert_allclose(nm[stable], nm_r[stable], rtol=0, atol=ATOL[F64])
    np.testing.assert_allclose(ps[stable], ps_r[stable], rtol=0, atol=ATOL[F64])
    # the known words come back as given, the wrong ones included, on every codeword
    kn = c.known >= 0
    assert np.array_equal(mp[kn], c.known[kn])
    assert mp[2, c.L_unp + ref.WRONG_LOC] != c.true[2, c.L_unp + ref.WRONG_LOC]
    assert mp[3, c.L_unp + ref.WRONG_SIGN] == c.true[3, c.L_unp + ref.WRONG_SIGN] ^ 1
    # the host variant is the same decode
    for a, b in zip(host_decode(c, F64, c.t_max, c.known, phi_method=phi_method), (mp, tf, nm, ps)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name,phi_method", ref.VS_NAMES)
def test_f32_vs_restatement(name, phi_method):
    c = ref.case(name)
    mp_r, _, _, _ = c.restatement(c.t_max, phi_method)
    clean = np.all((mp_r == c.true) | (c.known >= 0), axis=1)  # no section error outside the given (wrong) words
    assert np.count_nonzero(clean) >= 5, clean
    mp, _, _, _ = device_decode(c, F32, c.t_max, c.known, phi_method=phi_method)
    assert np.array_equal(mp[clean], mp_r[clean])
    assert np.array_equal(mp[c.known >= 0], c.known[c.known >= 0])
    _, _, nm_r, _ = c.restatement(4, phi_method)
    _, _, nm, _ = device_decode(c, F32, 4, c.known, phi_method=phi_method)
    print(f"{name} phi {phi_method} f32 t_max=4: max |nmse - ref| = {np.max(np.abs(nm - nm_r)):.3e}")
    np.testing.assert_allclose(nm, nm_r, rtol=0, atol=ATOL[F32])


# ---------------------------------------------------------------- nothing known = the plain K = 2 decode

@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", ["flat", "pa", "bsc"])
def test_nothing_known_is_the_plain_decode(name, prec):
    """psi0 = 1.0 and z0 = y - Ab(0) = y exactly, so byte equality."""
    c = ref.case(name)
    plain = sparc.amp_decode_bpsk_batch(c.Y, op_of(c), c.var, c.t_max, 1e-6, 1, c.true, prec)
    assert len(set(plain[1].tolist())) >= 3
    for got in (device_decode(c, prec, c.t_max, c.none), host_decode(c, prec, c.t_max, c.none)):
        for a, b in zip(got, plain):
            assert a.tobytes() == b.tobytes()
    # the device variant takes anything outside [0, 2M) as unknown
    junk = c.none.copy()
    junk[0, :] = 2 * c.M
    junk[1, ::2] = -9
    junk[2, 1] = 2 * c.M + 77
    for a, b in zip(device_decode(c, prec, c.t_max, junk), plain):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- section sizes

@pytest.mark.parametrize("name", ref.SIZE_NAMES)
def test_section_sizes(name):
    """M = 2 (62 idle lanes, one entry per lane), M = 128 (8 per lane) and M = 2048 (32 per lane): half the
    sections known, one wrong sign and one wrong location among them, t_max 3."""
    c = ref.case(name)
    mp_r, tf_r, nm_r, ps_r = c.restatement(c.t_max)
    mp, tf, nm, ps = device_decode(c, F64, c.t_max, c.known)
    print(f"{name}: max |nmse - ref| {np.max(np.abs(nm - nm_r)):.3e}, max |psi - ref| {np.max(np.abs(ps - ps_r)):.3e}")
    assert np.array_equal(tf, tf_r) and np.array_equal(mp, mp_r)
    np.testing.assert_allclose(nm, nm_r, rtol=0, atol=ATOL[F64])
    np.testing.assert_allclose(ps, ps_r, rtol=0, atol=ATOL[F64])
    mp32, _, nm32, _ = device_decode(c, F32, c.t_max, c.known)
    assert np.array_equal(mp32[c.known >= 0], c.known[c.known >= 0])
    np.testing.assert_allclose(nm32, nm_r, rtol=0, atol=ATOL[F32])


# ---------------------------------------------------------------- batch independence

@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", ["flat", "pa", "bsc"])
def test_codeword_does_not_depend_on_its_batch(name, prec):
    c = ref.case(name)
    whole = host_decode(c, prec, c.t_max, c.known)
    assert len(set(whole[1].tolist())) >= 3
    for b in (0, 2, 4, 7):
        one = host_decode(c, prec, c.t_max, c.known, rows=slice(b, b + 1))
        for w, o in zip(whole, one):
            assert np.array_equal(w[b], o[0]), (name, prec, b)


# ---------------------------------------------------------------- refusals and the plan's state

def test_refusals_and_plan_state():
    c = ref.case("flat")
    op = op_of(c)
    lib, p = _native.lib(), _native.ptr
    B, L, per = c.nb, c.L, int(np.log2(c.M)) + 1
    BAD = _native.SG_ERR_BAD_ARG
    plan = op.plan(F64)
    kn = np.ascontiguousarray(c.known, np.int32)
    d_y, d_k = _native.DeviceBuffer.from_array(c.Y), _native.DeviceBuffer.from_array(kn)
    d_m, h_m = _guarded((B, L), np.int32, -7)
    # null buffers
    assert lib.sg_amp_decode_bpsk_partial_device(plan, None, B, d_k.ptr, None, 1.0, 25, 1e-6, 1, d_m.ptr, None, None,
                                                 None, None) == BAD
    assert lib.sg_amp_decode_bpsk_partial_device(plan, d_y.ptr, B, None, None, 1.0, 25, 1e-6, 1, d_m.ptr, None, None,
                                                 None, None) == BAD and b"d_known_word" in lib.sg_last_error()
    mp, tf, nm, ps = sparc._decode_outputs(B, op, 25)
    assert lib.sg_amp_decode_bpsk_partial(plan, p(c.Y), B, None, None, 1.0, 25, 1e-6, 1, p(mp), p(tf), p(nm),
                                          p(ps)) == BAD and b"null host buffer" in lib.sg_last_error()
    assert lib.sg_amp_decode_bpsk_partial(plan, p(c.Y), B, p(kn), None, 1.0, 25, 1e-6, 1, None, p(tf), p(nm),
                                          p(ps)) == BAD
    # bad scalars, as sg_amp_decode_bpsk
    for var, t_max, rtol, phi in ((1.0, 1, 1e-6, 1), (1.0, 25, 0.0, 1), (1.0, 25, 1e-6, 3), (-1.0, 25, 1e-6, 1)):
        assert lib.sg_amp_decode_bpsk_partial_device(plan, d_y.ptr, B, d_k.ptr, None, var, t_max, rtol, phi, d_m.ptr,
                                                     None, None, None, None) == BAD
    # a host word outside [-1, 2M) is refused, naming its index
    for bad in (-2, 2 * c.M):
        known = c.known.copy()
        known[3, 7] = bad
        with pytest.raises(_native.NativeError, match=rf"known_word\[{3 * L + 7}\]"):
            sparc.amp_decode_bpsk_partial_batch(c.Y, op, known, 1.0, 25)
    _native.synchronize()
    assert np.all(d_m.download(h_m) == -7)  # nothing was launched
    # B = 0 does nothing
    assert lib.sg_amp_decode_bpsk_partial(plan, p(np.zeros(0)), 0, None, None, 1.0, 25, 1e-6, 1, None, None, None,
                                          None) == _native.SG_OK
    # soft output: kept by a plain decode, not by a decode with known words, and kept again by the next plain one
    op.soft_output(True, F64)
    plain = sparc.amp_decode_bpsk_batch(c.Y, op, 1.0, 25, true_word=c.true)
    llr = sparc.amp_llr_bpsk(op, B, 0, L)
    host_decode(c, F64, 25, c.known)
    out = np.empty_like(llr)
    assert lib.sg_amp_bpsk_llr(plan, B, 0, L, 0, p(out)) == BAD and b"no K = 2 decode" in lib.sg_last_error()
    assert lib.sg_amp_llr(plan, B, 0, L, 0, p(np.empty((B, L * (per - 1))))) == BAD  # sg_amp_llr* keeps refusing
    device_decode(c, F64, 25, c.known)
    assert lib.sg_amp_bpsk_llr(plan, B, 0, L, 0, p(out)) == BAD
    again = sparc.amp_decode_bpsk_batch(c.Y, op, 1.0, 25, true_word=c.true)
    for a, b in zip(plain, again):
        assert np.array_equal(a, b)
    assert np.array_equal(sparc.amp_llr_bpsk(op, B, 0, L), llr)
    op.soft_output(False, F64)


def test_m4096_is_refused_before_any_launch():
    s = ssc.case("m4096")
    op = sparc.DesignOperator(s.W, s.L, s.M, s.n, s.o0, s.o1)
    lib, p = _native.lib(), _native.ptr
    known = np.full((ssc.B, s.L), -1, np.int32)
    mp, tf = np.full((ssc.B, s.L), -7, np.int32), np.full(ssc.B, -7, np.int32)
    nm, ps = np.full((ssc.B, 25, 1), -7.0), np.full((ssc.B, 1), -7.0)
    d_y, d_k = _native.DeviceBuffer.from_array(s.Y), _native.DeviceBuffer.from_array(known)
    d_m, h_m = _guarded((ssc.B, s.L), np.int32, -7)
    for prec in (F64, F32):
        rc = lib.sg_amp_decode_bpsk_partial(op.plan(prec), p(s.Y), ssc.B, p(known), None, 1.0, 25, 1e-6, 1, p(mp),
                                            p(tf), p(nm), p(ps))
        assert rc == _native.SG_ERR_UNSUPPORTED and b"2048" in lib.sg_last_error()
        rc = lib.sg_amp_decode_bpsk_partial_device(op.plan(prec), d_y.ptr, ssc.B, d_k.ptr, None, 1.0, 25, 1e-6, 1,
                                                   d_m.ptr, None, None, None, None)
        assert rc == _native.SG_ERR_UNSUPPORTED and b"2048" in lib.sg_last_error()
    _native.synchronize()
    assert np.all(mp == -7) and np.all(tf == -7) and np.all(nm == -7) and np.all(ps == -7)
    assert np.all(d_m.download(h_m) == -7)


def test_unmodulated_known_sections_on_an_sc_plan_stay_unsupported():
    c = ref.case("bsc")
    known = np.full((2, c.L), -1, np.int32)
    with pytest.raises(_native.NativeError, match="spatially coupled"):
        sparc.amp_decode_partial_batch(c.Y[:2], op_of(c), known, 1.0, 5)
    d_y, d_k = _native.DeviceBuffer.from_array(c.Y[:2]), _native.DeviceBuffer.from_array(known)
    assert _native.lib().sg_amp_decode_partial_device(op_of(c).plan(F64), d_y.ptr, 2, d_k.ptr, None, 1.0, 5, 1e-6, 1,
                                                      None, None, None, None, None) == _native.SG_ERR_UNSUPPORTED


# ---------------------------------------------------------------- pipeline

def _pipe(cls, name, precision, **kw):
    L, M, Lu, mults, n, var = cr.POINTS[name]
    return cls(L, M, n, cr.P, Lu, mults, ldpc=cr.LDPC, design_seed=0, precision=precision, **kw)


def _run(pipe, Y, words, info, var):
    pipe.d_y.upload(np.ascontiguousarray(Y, pipe.dt))
    pipe.d_true.upload(np.ascontiguousarray(words, np.int32))
    pipe.d_info.upload(np.ascontiguousarray(info, np.uint8))
    pipe.B, pipe.awgn_var = len(Y), float(var)
    pipe.reset_counts()
    pipe.decode()
    return pipe.counts()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_pipeline_at_the_operating_points(name, precision):
    """The operating points of tests/test_bpsk_partial_host.py with host-made batches: the five counters are the
    restatement's on the received words the pipeline holds, over the codewords the one-ulp rule keeps (at least 6 of
    8); at A the unprotected counter is below the two-stage pipeline's on the same batch."""
    L, M, Lu, mults, n, var = cr.POINTS[name]
    nb = cr.PIPE_B
    p = ref.point(name)
    pipe = _pipe(DctBpskConcat3Pipeline, name, precision)
    words, info = pipe.make_batch(nb, var, np.random.default_rng(1))
    info = info.reshape(nb, -1)
    assert np.array_equal(words, p["words"])  # the host test's batch
    Y = pipe.d_y.download(np.empty((nb, n), pipe.dt)).astype(np.float64)
    rs = ref.point_three_stage(name, Y)
    stable = ref.point_stable(name, Y, rs)
    assert np.count_nonzero(~stable) <= 2, stable
    keep = np.nonzero(stable)[0]
    want2 = sum(ref.counters(rs[b]["map2"], words[b], rs[b]["app"], info[b], Lu, pipe.c.K) for b in keep)
    want3 = sum(ref.counters(rs[b]["map3"], words[b], rs[b]["app"], info[b], Lu, pipe.c.K) for b in keep)
    three = _run(pipe, Y[keep], words[keep], info[keep], var)
    two_pipe = _pipe(DctBpskConcatPipeline, name, precision)
    two_pipe._ensure(nb)
    two = _run(two_pipe, Y[keep], words[keep], info[keep], var)
    print(f"point {name} {precision}: two-stage {two.tolist()}, three-stage {three.tolist()}; restatement "
          f"{want2.tolist()}, {want3.tolist()}; kept {len(keep)} of {nb}")
    assert three[0] == len(keep) and three[3] + three[4] == three[1]
    assert three[4] == two[4]  # the same BP output counts the protected bits
    assert np.array_equal(two, want2)
    assert np.array_equal(three, want3)
    if name == "A":
        assert three[3] < two[3]


def test_spatially_coupled_design_through_the_pipeline():
    """bsc's base matrix (omega = 2, Lambda = 4) at L = 128, M = 32: 108 protected sections of 6 bits."""
    L, M, Lu, n = 128, 32, 20, 700
    W = sparc.sc_basic(np.array(cr.P), 2, 4)
    Lr, Lc = W.shape
    o0, o1 = sparc.generate_ordering(W, n // Lr, L * M // Lc, 5)
    op = sparc.DesignOperator(W, L, M, n, o0, o1)
    pipe = DctBpskConcat3Pipeline(L, M, n, cr.P, Lu, 1, ldpc=cr.LDPC, precision="f64", op=op)
    pipe.make_batch(4, 1.0, np.random.default_rng(2))
    pipe.reset_counts()
    pipe.decode()
    cnt = pipe.counts()
    print("spatially coupled three-stage K = 2 pipeline: counters", cnt.tolist())
    assert cnt[0] == 4 and cnt[3] + cnt[4] == cnt[1]


def test_pipeline_device_batches_rank_invariant():
    """make_batch_device through ConcatTrial: the counters of four blocks are the same decoded by one rank and dealt
    to two (the Philox key of a block is (seed, point, block)), and final_t_max reaches the last pass."""
    var = cr.POINTS["A"][5]
    pipe = _pipe(DctBpskConcat3Pipeline, "A", "f32", final_t_max=12)
    assert pipe.final_t_max == 12 and _pipe(DctBpskConcat3Pipeline, "A", "f32").final_t_max == 25
    tr = montecarlo.ConcatTrial(pipe, [var], seed=4)
    one = tr(0, 0, 4, 8)
    shards = [montecarlo.shard_range(4, r, 2) for r in range(2)]
    split = sum(tr(0, lo, hi - lo, 8) for lo, hi in shards)
    assert int(one[0]) == 32 and np.array_equal(one, split)
    assert one[3] + one[4] == one[1]
