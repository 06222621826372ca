"""Fixtures too large for one committed file are stored as parts,
<name>_p0.npz, <name>_p1.npz, ..., each under the repository's 1 MiB limit for a
committed file; tests/conftest.py merges the parts of a fixture into one mapping."""
import glob
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PART_MAX_BYTES = 900 * 1024


def save_parts(name, arrays, n_parts=None):
    """Write `arrays` (name -> array, insertion order kept) as <name>_p<k>.npz,
    with as few parts as keep every file under PART_MAX_BYTES; returns the paths."""
    for old in glob.glob(os.path.join(HERE, name + "_p*.npz")):
        os.remove(old)
    keys = list(arrays)
    n = n_parts or 1
    while True:
        raw = sum(np.asarray(arrays[k]).nbytes for k in keys)
        paths, part, acc, k0 = [], {}, 0, 0
        for k in keys:
            part[k] = arrays[k]
            acc += np.asarray(arrays[k]).nbytes
            if acc >= raw / n and k0 < n - 1:
                paths.append(_write(name, k0, part))
                part, acc, k0 = {}, 0, k0 + 1
        if part:
            paths.append(_write(name, k0, part))
        if all(os.path.getsize(p) <= PART_MAX_BYTES for p in paths):
            return paths
        for p in paths:
            os.remove(p)
        n += 1


def _write(name, k, part):
    path = os.path.join(HERE, f"{name}_p{k}.npz")
    np.savez_compressed(path, **part)
    return path
