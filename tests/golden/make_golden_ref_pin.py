"""Generate tests/golden/ldpc_ref_pin.npz: the outputs of the reference's own C
decoder core (oracle/_ref/libc_ldpc_ref.so, built by `make -C oracle` where the
reference sources are present) on the inputs that tests/test_ldpc_host.py draws,
so that those tests pin the CPU restatement to the reference on any checkout.

  python tests/golden/make_golden_ref_pin.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import bp  # noqa: E402
from ldpc_sparc_amd.ldpc import code  # noqa: E402


def main():
    if not bp.ref_available():
        raise SystemExit("oracle/_ref is not built: run `make -C oracle` with the reference sources present")
    # test_minsum_fixed_equals_reference_on_uniform_degree
    c = code("802.16", "5/6", 27)
    rng = np.random.default_rng(7)
    apps, its = [], []
    for _ in range(6):
        x = c.encode(rng.integers(0, 2, c.K))
        llr = 2 * ((1 - 2 * x) + 0.6 * rng.standard_normal(c.N)) / 0.36
        a, i = bp.decode("minsum_refbug", llr, c.vdeg, c.cdeg, c.intrlv, 50, use_ref=True)
        apps.append(np.array(a, np.float64))
        its.append(i)
    # test_lxor_lxfb_oracle
    rng = np.random.default_rng(0)
    lx, tot, ext = [], [], []
    for _ in range(50):
        a, b = rng.standard_normal(2) * 5
        lx.append([bp.lxor(a, b, corr, use_ref=True) for corr in (0, 1)])
        L = rng.standard_normal(7) * 3
        r = bp.lxfb(L, 1, use_ref=True)
        tot.append(r[0])
        ext.append(np.array(r[1], np.float64))
    np.savez_compressed(os.path.join(HERE, "ldpc_ref_pin.npz"), minsum_app=np.array(apps),
                        minsum_it=np.array(its, np.int64), lxor=np.array(lx, np.float64),
                        lxfb_total=np.array(tot, np.float64), lxfb_ext=np.array(ext))


if __name__ == "__main__":
    main()
