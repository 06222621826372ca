"""GPU state evolution for complex K-PSK SPARCs, K > 2 (se.hip,
ldpc_sparc_amd.sparc_se) against the reference's outputs
(tests/golden/se_psk_golden.npz, written by tests/golden/make_golden_se_psk.py:
the reference run with seeded numpy samples).  Bars as tests/test_se_gpu.py:
psi within rtol 1e-10 / atol 1e-14, tau within rtol 1e-10."""
import os
import sys

import numpy as np
import pytest

from ldpc_sparc_amd import sparc, sparc_se

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden_se_psk import CASES  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def se_psk_golden():
    with np.load(os.path.join(HERE, "golden", "se_psk_golden.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(CASES))
def test_state_evolution_matches_reference(se_psk_golden, name):
    cp, var, t_max, mc, seed = CASES[name]
    np.random.seed(seed)
    code_params = dict(cp)
    psi, tau = sparc_se.sparc_se(var, code_params, t_max, mc)
    ref_psi, ref_tau = se_psk_golden[name + "_psi"], se_psk_golden[name + "_tau"]
    assert np.all(np.isfinite(ref_psi)) and np.all(np.isfinite(ref_tau))
    print(name, "max |psi - ref|", np.max(np.abs(psi - ref_psi)), "max rel tau",
          np.max(np.abs(np.asarray(tau) - ref_tau) / np.abs(ref_tau)))
    np.testing.assert_allclose(psi, ref_psi, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(tau, ref_tau, rtol=1e-10)
    assert 'complex' in code_params and 'modulated' in code_params  # check_code_params rewrote it


def _se_E_host(tau, K, u):
    """sparc_se_E for K >= 8 restated in NumPy (sparc_se.py:99-115), exponents
    shifted by each sample's largest: the same quantity, never overflowing."""
    c = sparc.psk_constel(K)
    itau, rtau = 1 / tau, np.sqrt(1 / tau)
    g0 = np.real((itau + rtau * u[:, :1]) * c.conj()[None, :])            # [mc, K]
    gj = np.real((rtau * u[:, 1:, None]) * c.conj()[None, None, :])        # [mc, M-1, K]
    m = np.maximum(g0.max(axis=1), gj.max(axis=(1, 2)))
    e0, ej = np.exp(g0 - m[:, None]), np.exp(gj - m[:, None, None])
    return np.mean((e0 * c.real[None, :]).sum(axis=1) / (e0.sum(axis=1) + ej.sum(axis=(1, 2))))


def test_expectation_scalar_and_vector_k8():
    rng = np.random.default_rng(0)
    u = rng.standard_normal((300, 16)) + 1j * rng.standard_normal((300, 16))
    taus = np.array([0.004, 0.05, 0.3])  # 1 / 0.004 = 250: the shifted exponent stays finite where e^250 would still do
    E = sparc_se.sparc_se_E(taus, 8, u)
    assert E.shape == (3,)
    for t, e in zip(taus, E):
        one = sparc_se.sparc_se_E(float(t), 8, u)
        assert isinstance(one, float) and one == e  # the same kernel per tau, whatever the launch width
        assert abs(e - _se_E_host(t, 8, u)) <= 1e-12 * abs(e)
    assert 0 < E[2] < E[1] < E[0] <= 1


def test_k128_and_sample_kinds_raise():
    u = np.zeros((4, 8))
    with pytest.raises(NotImplementedError, match="K > 64"):
        sparc_se.sparc_se_E(0.1, 128, u + 0j)
    with pytest.raises(NotImplementedError, match="K > 64"):
        sparc_se.sparc_se(1.0, {'P': 15.0, 'R': 2.0, 'M': 16, 'complex': True, 'modulated': True, 'K': 128}, 5, 10)
    with pytest.raises(Exception, match="complex samples"):
        sparc_se.sparc_se_E(0.1, 4, u)        # K >= 4 needs complex samples
    with pytest.raises(Exception, match="complex samples"):
        sparc_se.sparc_se_E(0.1, 2, u + 0j)   # K <= 2 needs real samples
