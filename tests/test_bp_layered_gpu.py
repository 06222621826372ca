"""GPU tests of the layered BP schedule (bp_layered.hip) against its NumPy
restatement (tests/bp_layered_ref.py): min-sum bit for bit in both
precisions, sumprod2 within the project's float64 bar and a measured float32
one, batch independence, the device entry point and its refusals, and the
campaign layer."""
import numpy as np
import pytest

import bp_layered_cases as cases
import bp_layered_ref as lr
from ldpc_sparc_amd import _native
from ldpc_sparc_amd import montecarlo as mc
from ldpc_sparc_amd.ldpc import code

pytestmark = pytest.mark.gpu

# float32 sumprod2 against the float64 restatement, over the codewords the restatement stops before max_it:
# largest |app - ref| / max(1, |ref|) observed on an MI355X over every case below.  The bar is 4 x that (the
# margin covers box-to-box last-ulp differences of exp / log).  Observed per code at max_it = 50, in the order
# of cases.SPECS: 1.1e-5, 6.0e-2, 2.7e-4, 6.5e-3, 8.7e-5 (at max_it = 5 at most 2.3e-6): the large ones are
# single codewords that stop late, whose float32 rounding the iterations have amplified.
F32_SUMPROD2_OBSERVED = 5.965e-2
F32_SUMPROD2_BAR = 4 * F32_SUMPROD2_OBSERVED


def decode(spec, dectype, precision, max_it, rows=slice(None)):
    c = cases.get_code(spec)
    ch = cases.batch(spec, dectype)[1][rows]
    return c.decode_batch(ch, max_it, dectype, 0.7, precision=precision, schedule="layered")


@pytest.mark.parametrize("max_it", cases.MAX_ITS)
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("spec", cases.SPECS)
def test_minsum_bit_identical_to_restatement(spec, precision, max_it):
    rapp, rit = cases.reference(spec, "minsum", precision, max_it)
    if max_it == 50:  # the inputs do what they were chosen for
        assert 0 < (rit == 50).sum() < cases.B / 2
    app, it = decode(spec, "minsum", precision, max_it)
    assert np.array_equal(it, rit)
    assert np.array_equal(app, rapp.astype(np.float64))  # (float32 -> float64 is exact)
    a1, i1 = decode(spec, "minsum", precision, max_it, slice(5, 6))  # B = 1
    assert i1[0] == rit[5] and np.array_equal(a1[0], rapp[5].astype(np.float64))


@pytest.mark.parametrize("max_it", cases.MAX_ITS)
@pytest.mark.parametrize("spec", cases.SPECS)
def test_sumprod2_f64_vs_restatement(spec, max_it):
    """The bar of test_bp_gpu.py test_high_degree_sumprod2_vs_oracle: 1e-9."""
    rapp, rit = cases.reference(spec, "sumprod2", "f64", max_it)
    if max_it == 50:
        assert 0 < (rit == 50).sum() <= cases.B // 10
    app, it = decode(spec, "sumprod2", "f64", max_it)
    print(f"{spec} max_it {max_it}: max |app - ref| / max(1, |ref|) = "
          f"{np.max(np.abs(app - rapp) / np.maximum(1, np.abs(rapp))):.3e}")
    assert np.array_equal(it, rit)
    np.testing.assert_allclose(app, rapp, rtol=1e-9, atol=1e-9)
    a1, i1 = decode(spec, "sumprod2", "f64", max_it, slice(5, 6))
    assert i1[0] == it[5] and np.array_equal(a1[0], app[5])


@pytest.mark.parametrize("max_it", cases.MAX_ITS)
@pytest.mark.parametrize("spec", cases.SPECS)
def test_sumprod2_f32_vs_f64_restatement(spec, max_it):
    """On every codeword the float64 restatement stops before max_it (at
    max_it = 50 at least 90 % of the batch): its hard decisions and iteration
    index, and app within the measured bar."""
    rapp, rit = cases.reference(spec, "sumprod2", "f64", max_it)
    stopped = rit < max_it
    if max_it == 50:
        assert stopped.mean() >= 0.9
    app, it = decode(spec, "sumprod2", "f32", max_it)
    dev = np.abs(app[stopped] - rapp[stopped]) / np.maximum(1, np.abs(rapp[stopped]))
    print(f"{spec} max_it {max_it}: {int(stopped.sum())} stopped, f32 deviation {dev.max() if dev.size else 0.0:.3e}")
    assert np.array_equal(it[stopped], rit[stopped])
    assert np.array_equal(app[stopped] < 0, rapp[stopped] < 0)
    if dev.size:
        assert dev.max() <= F32_SUMPROD2_BAR


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("dectype", ["minsum", "sumprod2"])
@pytest.mark.parametrize("spec", cases.SPECS)
def test_batch_independence(spec, dectype, precision):
    """Codeword b decoded alone equals codeword b within the batch of 37, bitwise."""
    app, it = decode(spec, dectype, precision, 50)
    for b in (0, 17, 36):
        a1, i1 = decode(spec, dectype, precision, 50, slice(b, b + 1))
        assert i1[0] == it[b] and np.array_equal(a1[0], app[b]), b


def _device_decode(c, dectype, prec, layer, ch, max_it, corr=0.7):
    dt = np.float64 if prec == _native.SG_F64 else np.float32
    n = ch.shape[0]
    d_ch = _native.DeviceBuffer.from_array(ch.astype(dt))
    d_app = _native.DeviceBuffer(max(ch.size, 1) * np.dtype(dt).itemsize)
    d_it = _native.DeviceBuffer(max(n, 1) * 4)
    rc = _native.lib().sg_ldpc_decode_layered_device(c._device_graph(), dectype, prec, int(layer), d_ch.ptr, n,
                                                     int(max_it), float(corr), d_app.ptr, d_it.ptr, None)
    if rc != _native.SG_OK:
        return rc, None, None
    _native.synchronize()
    return rc, d_app.download(np.zeros(ch.shape, dt)), d_it.download(np.zeros(n, np.int32))


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("dectype", ["minsum", "sumprod2"])
def test_device_entry_point_matches_host(dectype, precision):
    spec = ("802.11n", "1/2", 81)
    c = cases.get_code(spec)
    prec = {"f64": _native.SG_F64, "f32": _native.SG_F32}[precision]
    ch = cases.batch(spec, dectype)[1]
    if precision == "f32":
        ch = ch.astype(np.float32)
    rc, app, it = _device_decode(c, _native.DECTYPES[dectype], prec, c.z, np.asarray(ch), 50)
    assert rc == _native.SG_OK
    happ, hit = decode(spec, dectype, precision, 50)
    assert np.array_equal(it, hit) and np.array_equal(app.astype(np.float64), happ)


def test_device_entry_point_refusals():
    c = cases.get_code(("802.11n", "1/2", 27))
    L = _native.lib()
    ch = np.asarray(cases.batch(("802.11n", "1/2", 27), "minsum")[1][:2])
    rc, _, _ = _device_decode(c, _native.SG_SUMPROD, _native.SG_F64, c.z, ch, 10)
    assert rc == _native.SG_ERR_UNSUPPORTED and b"sumprod" in L.sg_last_error()
    rc, _, _ = _device_decode(c, _native.SG_MINSUM, _native.SG_F64, 2 * c.z, ch, 10)
    assert rc == _native.SG_ERR_INVALID and b"occurs twice in layer 0" in L.sg_last_error()
    rc, _, _ = _device_decode(c, _native.SG_MINSUM, _native.SG_F64, c.z + 1, ch, 10)
    assert rc == _native.SG_ERR_INVALID and b"does not divide" in L.sg_last_error()
    for max_it in (0, -1):
        rc, _, _ = _device_decode(c, _native.SG_MINSUM, _native.SG_F32, c.z, ch, max_it)
        assert rc == _native.SG_ERR_INVALID and b"max_it" in L.sg_last_error()
    with pytest.raises(_native.NativeError, match="max_it"):
        c.decode_batch(ch, 0, "minsum", schedule="layered")
    with pytest.raises(_native.NativeError, match="sumprod"):
        c.decode(ch[0], 10, "sumprod", schedule="layered")
    with pytest.raises(NameError, match="Schedule unknown"):
        c.decode_batch(ch, 10, "minsum", schedule="serial")
    # after the refusals the graph still decodes
    app, it = c.decode_batch(ch, 5, "minsum", schedule="layered")
    rapp, rit = cases.reference(("802.11n", "1/2", 27), "minsum", "f64", 5)
    assert np.array_equal(it, rit[:2]) and np.array_equal(app, rapp[:2])


def test_graph_too_large_for_lds_is_refused_before_launch():
    """Two copies of the 802.16 r1/2 protograph side by side at z = 96: app and
    R of one codeword are 154 KB in float64, the tables 29 KB more, above one
    workgroup's 160 KB; float32 (106 KB in all) decodes."""
    c = code("802.16", "1/2", 96)
    mp, np_ = c.proto.shape
    big = -np.ones((2 * mp, 2 * np_), dtype=c.proto.dtype)
    big[:mp, :np_] = c.proto
    big[mp:, np_:] = c.proto
    c2 = code("802.16", "1/2", 96)
    c2.proto = big
    c2.vdeg, c2.cdeg, c2.intrlv = c2.prepare_decoder()
    c2.Nv, c2.Nc, c2.Nmsg = len(c2.vdeg), len(c2.cdeg), len(c2.intrlv)
    c2.N, c2.K = c2.Nv, c2.Nv - c2.Nc
    X, ch = cases.batch(("802.16", "1/2", 96), "minsum")
    ch2 = np.concatenate([ch[:2], ch[2:4]], axis=1)  # two codewords of c side by side are one of c2
    with pytest.raises(_native.NativeError, match="LDS") as e:
        c2.decode_batch(ch2, 50, "minsum", schedule="layered")
    assert f"error {_native.SG_ERR_UNSUPPORTED}" in str(e.value)
    app, it = c2.decode_batch(ch2, 50, "minsum", precision="f32", schedule="layered")
    rapp, rit = lr.layered(c2.vdeg, c2.cdeg, c2.intrlv, ch2, c2.z, 50, "minsum", 0.7, np.float32)
    assert np.array_equal(it, rit) and np.array_equal(app, rapp.astype(np.float64))
    assert c2.decode_kernel("minsum", _native.SG_F32, schedule="layered") == "bp_layered_kernel<float, 2, 8, 128>"


def test_kernel_names():
    c = cases.get_code(("802.11n", "1/2", 27))
    assert c.decode_kernel("minsum", schedule="layered") == "bp_layered_kernel<float, 2, 8, 64>"
    assert c.decode_kernel("sumprod2", _native.SG_F64, schedule="layered") == "bp_layered_kernel<double, 1, 8, 64>"
    c = cases.get_code(("802.11n", "5/6", 27))
    assert c.decode_kernel("minsum", schedule="layered") == "bp_layered_kernel<float, 2, 0, 64>"
    c = cases.get_code(("802.11n", "1/2", 81))
    assert c.decode_kernel("minsum", schedule="layered") == "bp_layered_kernel<float, 2, 8, 128>"
    assert c.decode_kernel("minsum").startswith("bp_grouped")  # flooding's answer is unchanged


@pytest.mark.parametrize("rng", ["device", "host"])
def test_campaign_sharding_invariance_layered(rng):
    c = cases.get_code(("802.11n", "1/2", 27))
    trial = mc.LdpcTrial(c, [2.0], dectype="minsum", max_it=10, precision="f32", seed=3, rng=rng,
                         schedule="layered")
    whole = trial(0, 0, 4, 64)
    parts = sum(trial(0, a, b - a, 64) for a, b in (mc.shard_range(4, r, 2) for r in range(2)))
    assert whole.tolist() == parts.tolist()
    flood = mc.LdpcTrial(c, [2.0], dectype="minsum", max_it=10, precision="f32", seed=3, rng=rng)(0, 0, 4, 64)
    print(f"rng {rng}: frame errors of 256 at max_it = 10: layered {int(whole[2])}, flooding {int(flood[2])}")
    assert whole[0] == flood[0] == 256
    # (host streams: the float32 restatements give CAMPAIGN_FE on these very words, see below)
    if rng == "host":
        assert (int(whole[2]), int(flood[2])) == CAMPAIGN_FE
    assert whole[2] <= flood[2]


# frame errors (layered, flooding) of the 256 codewords of the host-stream campaign test above, from the float32
# restatements (bp_layered_ref.layered, oracle/bp.py minsum_numpy) on the CPU
CAMPAIGN_FE = (31, 119)
