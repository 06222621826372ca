"""Outputs of the integrated AMP <-> BP decoders as the library computed them before the dense and the DCT host
loops became one (integ_loop.hpp), written to tests/golden/integ_same_bits.npz: the inputs and, per design x mode x
precision, the information bits, the tau^2 history and (DCT entry point) the final BP output
(tests/integ_same_bits_cases.py).  tests/test_integrated_same_bits_gpu.py holds the current library to them bit for
bit.

Run once by hand on a GPU, with the library of the commit to pin:

    tools/build_alt.sh <rev>
    LDPC_SPARC_AMD_LIB=ldpc_sparc_amd/_lib_alt/libldpc_sparc_amd.so python tests/golden/make_golden_integ_same_bits.py

Every case is decoded twice; a case whose second decode differs in any bit is reported and left out of the fixture
(name it in integ_same_bits_cases.LEFT_OUT, with the reason).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import integ_same_bits_cases as sb  # noqa: E402
from conftest import _golden_parts  # noqa: E402
from ldpc_sparc_amd import _native  # noqa: E402


def make():
    ds = sb.Designs(_golden_parts("integrated_golden"))
    out = dict(ds.inputs)
    print("library:", _native.LIB_PATH)
    unstable = []
    for design in sb.DESIGNS:
        for mode in sb.MODES:
            for prec in sb.PRECISIONS:
                first, second = ds.decode(design, mode, prec), ds.decode(design, mode, prec)
                bad = [k for k in first if not sb.same_bits(first[k], second[k])]
                finite = all(np.all(np.isfinite(v)) for v in first.values())
                print(design, mode, prec, "tau2[0]", first["tau2"][0], "bits set", int(first["bits"].sum()),
                      "finite" if finite else "NOT FINITE", "DIFFERS ON A SECOND RUN: %s" % bad if bad else "repeats")
                if bad:
                    unstable.append((design, mode, prec))
                    continue
                for k, v in first.items():
                    out[sb.key(design, mode, prec, k)] = v
    ds.release()
    path = os.path.join(HERE, sb.FIXTURE)
    np.savez_compressed(path, **out)
    print("wrote", sb.FIXTURE, os.path.getsize(path) / 1e3, "kB;", len(unstable), "cases left out:", unstable)


if __name__ == "__main__":
    make()
