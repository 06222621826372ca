"""CPU tests: LDPC host logic (protographs, Tanner graph, encoder) and the BP
oracle against the golden vectors generated from the reference
(tests/golden/make_golden.py), mirroring ldpc_jossy/py/test_ldpc.py."""
import os

import numpy as np
import pytest

from ldpc_sparc_amd.ldpc import code
from oracle import bp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALL_CODES = [("802.16", r, z, p) for z in (3, 27, 54, 81)
             for (r, p) in [("1/2", "A"), ("2/3", "A"), ("2/3", "B"), ("3/4", "A"), ("3/4", "B"),
                            ("5/6", "A")]] + \
            [("802.11n", r, z, "A") for z in (27, 54, 81) for r in ("1/2", "2/3", "3/4", "5/6")]


@pytest.mark.parametrize("standard,rate,z,ptype", ALL_CODES)
def test_code_structure_and_encoder(standard, rate, z, ptype):
    """test_ldpc.py:44-59: proto width, degree sums, syndrome of random codewords."""
    c = code(standard, rate, z, ptype)
    assert len(c.proto[0]) == 24
    H = c.pcmat()
    assert np.sum(c.vdeg) == np.sum(c.cdeg) == np.sum(H) == len(c.intrlv)
    assert sorted(c.intrlv.tolist()) == list(range(c.Nmsg))
    rng = np.random.default_rng(z)
    U = rng.integers(0, 2, (20, c.K))
    X = c.encode_batch(U)
    assert np.count_nonzero(np.mod(X @ H.T, 2)) == 0
    assert np.array_equal(X[:, :c.K], U)
    assert np.array_equal(c.encode(U[3]), X[3])


def test_errors_match_reference():
    with pytest.raises(NameError, match="802.11n invalid z"):
        code("802.11n", "1/2", 30)
    with pytest.raises(NameError, match="802.16 type must be either A or B"):
        code("802.16", "2/3", 27, "C")
    with pytest.raises(NameError, match="IEEE standard unknown"):
        code("802.3", "1/2", 27)
    with pytest.raises(NameError, match="invalid rate"):
        code("802.11n", "7/8", 27)
    c = code()
    with pytest.raises(NameError, match="information word length"):
        c.encode(np.zeros(c.K + 1, dtype=int))


def test_graph_matches_reference_c_header(ldpc_golden):
    """ldpc_jossy/src/ldpc802.16.81.h holds intrlv/vdeg/cdeg for 802.16 r1/2 z=81."""
    c = code("802.16", "1/2", 81)
    assert np.array_equal(c.intrlv, ldpc_golden["h16_81_intrlv"])
    assert np.array_equal(c.vdeg, ldpc_golden["h16_81_vdeg"])
    assert np.array_equal(c.cdeg, ldpc_golden["h16_81_cdeg"])


def _cases(g):
    out = []
    for ci in range(3):
        std, rate, z = [str(s) for s in g[f"c{ci}_meta"]]
        out.append((ci, std, rate, int(z)))
    return out


def test_graph_and_encoder_golden(ldpc_golden):
    for ci, std, rate, z in _cases(ldpc_golden):
        c = code(std, rate, z)
        assert np.array_equal(c.intrlv, ldpc_golden[f"c{ci}_intrlv"])
        X = c.encode_batch(ldpc_golden[f"c{ci}_enc_u"])
        assert np.array_equal(X, ldpc_golden[f"c{ci}_enc_x"])


@pytest.mark.parametrize("dectype", ["sumprod", "sumprod2", "minsum"])
def test_oracle_bitexact_vs_reference_vectors(ldpc_golden, oracle_built, dectype):
    """The CPU restatement reproduces the reference c_ldpc.c outputs bit for bit
    (minsum: the shipped defective indexing, reproduced by minsum_refbug)."""
    kind = "minsum_refbug" if dectype == "minsum" else dectype
    for ci, std, rate, z in _cases(ldpc_golden):
        c = code(std, rate, z)
        for ei in range(3):
            chs = ldpc_golden[f"c{ci}_e{ei}_ch"]
            for mi in (5, 50, 200):
                key = f"c{ci}_e{ei}_{dectype}_{mi}"
                for j, ch in enumerate(chs):
                    app, it = bp.decode(kind, ch, c.vdeg, c.cdeg, c.intrlv, mi, 0.7)
                    assert it == ldpc_golden[key + "_it"][j], key
                    if mi == 200:
                        assert np.array_equal((app < 0).astype(np.uint8), ldpc_golden[key + "_hard"][j])
                    else:
                        assert np.array_equal(app, ldpc_golden[key + "_app"][j], equal_nan=True), key


def _ref_pin():
    """Outputs of the reference's own C decoder core on the inputs drawn below."""
    return np.load(os.path.join(REPO, "tests", "golden", "ldpc_ref_pin.npz"))


def test_minsum_fixed_equals_reference_on_uniform_degree(oracle_built):
    """With uniform check degree the reference's offset defect is inert, so the
    corrected minsum must agree with the reference library bit for bit: with its
    recorded outputs (tests/golden/ldpc_ref_pin.npz, make_golden_ref_pin.py), and
    with the library itself where oracle/_ref is built."""
    pin = _ref_pin()
    c = code("802.16", "5/6", 27)          # cdeg == 20 everywhere
    assert len(set(c.cdeg.tolist())) == 1
    rng = np.random.default_rng(7)
    for j in range(6):
        x = c.encode(rng.integers(0, 2, c.K))
        llr = 2 * ((1 - 2 * x) + 0.6 * rng.standard_normal(c.N)) / 0.36
        a1, i1 = bp.decode("minsum", llr, c.vdeg, c.cdeg, c.intrlv, 50)
        assert i1 == pin["minsum_it"][j] and np.array_equal(a1, pin["minsum_app"][j])
        if bp.ref_available():
            a2, i2 = bp.decode("minsum_refbug", llr, c.vdeg, c.cdeg, c.intrlv, 50, use_ref=True)
            assert i1 == i2 and np.array_equal(a1, a2)


def test_minsum_fixed_decodes_nonuniform_code(oracle_built):
    """SURVEY finding 0.5: the shipped minsum fails on 802.11n r1/2 z=81 (cdeg 7/8)
    while the corrected indexing decodes at 2.5 dB."""
    c = code("802.11n", "1/2", 81)
    rng = np.random.default_rng(3)
    R = c.K / c.N
    s2 = 1 / (2 * R * 10 ** 0.25)
    fixed_err = ref_err = 0
    for _ in range(10):
        x = c.encode(rng.integers(0, 2, c.K))
        llr = 2 * ((1 - 2 * x) + np.sqrt(s2) * rng.standard_normal(c.N)) / s2
        a, _ = bp.decode("minsum", llr, c.vdeg, c.cdeg, c.intrlv, 50)
        fixed_err += int(np.any((a < 0) != x))
        a, _ = bp.decode("minsum_refbug", llr, c.vdeg, c.cdeg, c.intrlv, 50)
        ref_err += int(np.any((a < 0) != x))
    assert fixed_err <= 1 and ref_err >= 8


def test_lxor_lxfb_oracle(oracle_built):
    """Lxor / Lxfb of the restatement against the reference library's recorded
    outputs (tests/golden/ldpc_ref_pin.npz), and against the library itself where
    oracle/_ref is built."""
    pin = _ref_pin()
    live = bp.ref_available()
    rng = np.random.default_rng(0)
    for j in range(50):
        a, b = rng.standard_normal(2) * 5
        for corr in (0, 1):
            assert bp.lxor(a, b, corr) == pin["lxor"][j, corr]
            if live:
                assert bp.lxor(a, b, corr) == bp.lxor(a, b, corr, use_ref=True)
        L = rng.standard_normal(7) * 3
        assert bp.lxfb(L, 1)[0] == pin["lxfb_total"][j]
        assert np.array_equal(bp.lxfb(L, 1)[1], pin["lxfb_ext"][j])
        if live:
            assert bp.lxfb(L, 1)[0] == bp.lxfb(L, 1, use_ref=True)[0]
            assert np.array_equal(bp.lxfb(L, 1)[1], bp.lxfb(L, 1, use_ref=True)[1])


@pytest.mark.parametrize("std,rate,z", [("802.11n", "1/2", 27), ("802.11n", "5/6", 27), ("802.16", "2/3", 24)])
def test_oracle_under_sanitizers(tmp_path, std, rate, z):
    """the CPU restatement (oracle/bp_oracle.c) built with
    -fsanitize=address,undefined (make -C oracle san) decodes real graphs --
    every decoder, and Lxfb at the graph's check degree -- without a report,
    and gives the same results as the normal build."""
    import subprocess
    from oracle import bp
    r = subprocess.run(["make", "-s", "-C", os.path.join(REPO, "oracle"), "san"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer toolchain unavailable: " + r.stderr[-300:])
    c = code(std, rate, z)
    rng = np.random.default_rng(3)
    X = c.encode_batch(rng.integers(0, 2, (4, c.K)))
    ch = 2 * ((1 - 2 * X) + 0.7 * rng.standard_normal(X.shape)) / 0.49
    B, max_it, factor = len(ch), 20, 0.7
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([c.N, c.Nc, c.Nmsg, B, max_it], np.int32).tobytes())
        f.write(np.array([factor]).tobytes())
        for a in (c.vdeg, c.cdeg, c.intrlv):
            f.write(np.asarray(a, np.int64).tobytes())
        f.write(np.ascontiguousarray(ch, np.float64).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "bp_oracle_san"), str(inp), str(out)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(out, "rb").read()
    o = 0
    for kind in ("sumprod", "sumprod2", "minsum", "minsum_refbug"):
        app = np.frombuffer(raw, np.float64, B * c.N, o).reshape(B, c.N)
        o += 8 * B * c.N
        it = np.frombuffer(raw, np.int32, B, o)
        o += 4 * B
        if kind == "minsum_refbug":
            continue  # pinned to the reference library elsewhere (test_minsum_refbug_matches_reference)
        eapp, eit = bp.decode_batch(kind, ch, c.vdeg, c.cdeg, c.intrlv, max_it, factor)
        assert np.array_equal(it, eit), kind
        np.testing.assert_allclose(app, eapp, rtol=1e-12, atol=1e-12, err_msg=kind)


def test_numpy_minsum_restatement_pinned(oracle_built):
    """oracle/bp.py minsum_numpy (the float32 checker of the GPU's
    single-precision min-sum) run in float64 equals the C restatement bit for
    bit: on a QC code and on an irregular graph with degree-1 variables."""
    rng = np.random.default_rng(2)
    c = code("802.11n", "1/2", 27)
    X = c.encode_batch(rng.integers(0, 2, (12, c.K)))
    ch = 2 * ((1 - 2 * X) + 0.9 * rng.standard_normal(X.shape)) / 0.81
    graphs = [(c.vdeg, c.cdeg, c.intrlv, ch)]
    vdeg = np.array([(1, 2, 3, 5, 11, 2, 4)[v % 7] for v in range(210)], dtype=np.int64)
    E = int(vdeg.sum())
    cdeg = np.full(E // 6, 6, dtype=np.int64)
    cdeg[: E - cdeg.sum()] += 1
    graphs.append((vdeg, cdeg, rng.permutation(E).astype(np.int64), 1.0 + 2.0 * rng.standard_normal((12, 210))))
    for vd, cd, il, y in graphs:
        for mi in (1, 6, 40):
            app, it = bp.minsum_numpy(y, vd, cd, il, mi, 0.7, np.float64)
            oapp, oit = bp.decode_batch("minsum", y, vd, cd, il, mi, 0.7)
            assert np.array_equal(it, oit) and np.array_equal(app, oapp)
