"""A double-precision plan with fewer conjugate row pairs than the split
engine's 512 threads (n = 300: some threads own no output) keeps the f64
split engine (build_cw2 rejects such plans for f32 only, whose padding slots
need a last pair to write to), and the engine agrees with the staged one: the
bars of test_amp_cw2d_gpu.py::test_f64_split_engine_first_iterations."""
import numpy as np
import pytest

from ldpc_sparc_amd import _native, sparc

pytestmark = pytest.mark.gpu


def test_small_f64_plan_keeps_split_engine(monkeypatch):
    L, M, n, B = 1024, 512, 300, 4
    W = np.array(15.0)
    o0, o1 = sparc.generate_ordering(W, n, L * M, 7)
    op = sparc.DesignOperator(W, L, M, n, o0, o1)
    rng = np.random.default_rng(9)
    true = rng.integers(0, M, (B, L)).astype(np.int32)
    beta0 = np.zeros((B, L * M))
    beta0[np.arange(B)[:, None], np.arange(L) * M + true] = 1
    Y = op.apply(beta0, False) + rng.standard_normal((B, n))
    for tm in (2, 3, 4):
        out = {}
        for engine in ("cw", "staged"):
            monkeypatch.setenv("SG_AMP_ENGINE", engine)
            out[engine] = sparc.amp_decode_batch(Y, op, 1.0, tm, true_idx=true)
            info = _native.amp_last_decode(op.plan(_native.SG_F64))
            assert info["engine"] == (2 if engine == "cw" else 1)
        print(tm, np.abs(out["cw"][3] / out["staged"][3] - 1).max(), np.abs(out["cw"][2] - out["staged"][2]).max())
        np.testing.assert_allclose(out["cw"][3], out["staged"][3], rtol=1e-11)
        np.testing.assert_allclose(out["cw"][2], out["staged"][2], rtol=0, atol=1e-11)
