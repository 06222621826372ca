"""SHA-256 digests of the raw soft-output buffers as the library computed them before the soft-output kernels were
rewritten on csrc/section_bits.hpp, written to tests/golden/soft_output_same_bits.npz: one digest per case and
output (tests/soft_output_same_bits_cases.py).  tests/test_soft_output_same_bits_gpu.py holds the current library
to them bit for bit.

Run once by hand on a GPU, with the library of the commit to pin:

    tools/build_alt.sh <rev>
    LDPC_SPARC_AMD_LIB=ldpc_sparc_amd/_lib_alt/libldpc_sparc_amd.so \\
        python tests/golden/make_golden_soft_output_same_bits.py

Every case is run twice; a case whose second run differs in any bit is reported and left out of the fixture (name it
in soft_output_same_bits_cases.LEFT_OUT, with the reason).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import soft_output_same_bits_cases as sb  # noqa: E402
from ldpc_sparc_amd import _native  # noqa: E402


def make():
    print("library:", _native.LIB_PATH)
    run = sb.Runner()
    out, unstable = {}, []
    for cid in sb.case_ids():
        first, second = run.run(cid), run.run(cid)
        bad = [k for k in first if sb.sha256(first[k]) != sb.sha256(second[k])]
        finite = all(np.all(np.isfinite(v)) for v in first.values())
        soft = sum(int(np.count_nonzero((v > 0.01) & (v < 0.99))) for k, v in first.items() if k == "p1")
        print(*cid, "soft probabilities", soft, "finite" if finite else "NOT FINITE",
              "DIFFERS ON A SECOND RUN: %s" % bad if bad else "repeats")
        if bad:
            unstable.append(cid)
            continue
        for k, v in first.items():
            out[sb.key(cid, k)] = np.array(sb.sha256(v))
    run.release()
    path = os.path.join(HERE, sb.FIXTURE)
    np.savez_compressed(path, **out)
    print("wrote", sb.FIXTURE, os.path.getsize(path) / 1e3, "kB;", len(unstable), "cases left out:", unstable)


if __name__ == "__main__":
    make()
