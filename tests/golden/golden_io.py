"""Golden fixtures larger than one committed file may be: tests/golden/<name>.partNN.npz.

A fixture set is one dict of arrays, stored as a few compressed .npz parts of under 1 MiB
each (every key in exactly one part); load_golden() puts them together again and
save_golden() (for the tests/golden/make_*.py generators) splits them."""
import glob
import os
import zlib

import numpy as np

GOLDEN = os.path.dirname(os.path.abspath(__file__))
PART_BYTES = 900_000        # target per part; a written part is checked against MAX_BYTES
MAX_BYTES = 1 << 20


def _parts(name):
    return sorted(glob.glob(os.path.join(GOLDEN, f"{name}.part[0-9][0-9].npz")))


def load_golden(name):
    """dict of every array of the fixture set `name`."""
    parts = _parts(name)
    if not parts:
        raise FileNotFoundError(f"no {name}.partNN.npz under {GOLDEN}")
    out = {}
    for p in parts:
        with np.load(p) as z:
            for k in z.files:
                assert k not in out, f"{k} in more than one part of {name}"
                out[k] = z[k]
    return out


def save_golden(name, arrays):
    """Write `arrays` as <name>.partNN.npz, keys in insertion order, replacing older parts."""
    for p in _parts(name):
        os.remove(p)
    groups, size = [{}], 0
    for k, v in arrays.items():
        v = np.asarray(v)
        n = len(zlib.compress(np.ascontiguousarray(v).tobytes(), 6)) + 256 + 2 * len(k)
        if groups[-1] and size + n > PART_BYTES:
            groups.append({})
            size = 0
        groups[-1][k] = v
        size += n
    paths = []
    for i, g in enumerate(groups):
        p = os.path.join(GOLDEN, f"{name}.part{i:02d}.npz")
        np.savez_compressed(p, **g)
        assert os.path.getsize(p) < MAX_BYTES, (p, os.path.getsize(p))
        paths.append(p)
    return paths
