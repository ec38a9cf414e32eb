"""TEST INFRASTRUCTURE: fixtures under tests/golden/ that are kept as several files, so that no committed file
exceeds 1 MiB.  tests/golden/make_golden.py writes them with `save_parts`; tests read them with `load_parts`."""
import glob
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_RAW_BYTES = 896 << 10   # arrays' bytes per part file before compression
CHUNK_RAW_BYTES = 256 << 10  # a larger array is stored as chunks `key@i` of its axis 1


def save_parts(stem, arrays):
    """Write `arrays` (name -> ndarray) as tests/golden/<stem>_NN.npz, in the order given."""
    items = []
    for k, a in arrays.items():
        n = -(-a.nbytes // CHUNK_RAW_BYTES)
        if n <= 1:
            items.append((k, a))
        else:
            items += [(f"{k}@{i}", c) for i, c in enumerate(np.array_split(a, n, axis=1))]
    parts, size = [{}], 0
    for k, a in items:
        if parts[-1] and size + a.nbytes > PART_RAW_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = a
        size += a.nbytes
    for old in glob.glob(os.path.join(G, f"{stem}_[0-9][0-9].npz")):
        os.remove(old)
    for i, p in enumerate(parts):
        np.savez_compressed(os.path.join(G, f"{stem}_{i:02d}.npz"), **p)


def load_parts(stem):
    """name -> ndarray of every array in tests/golden/<stem>_NN.npz, chunks joined again."""
    flat = {}
    for path in sorted(glob.glob(os.path.join(G, f"{stem}_[0-9][0-9].npz"))):
        with np.load(path) as f:
            flat.update({k: f[k] for k in f.files})
    if not flat:
        raise FileNotFoundError(f"no {stem}_NN.npz under {G}")
    out, chunks = {}, {}
    for k, a in flat.items():
        if "@" in k:
            name, i = k.split("@")
            chunks.setdefault(name, {})[int(i)] = a
        else:
            out[k] = a
    for name, c in chunks.items():
        out[name] = np.concatenate([c[i] for i in range(len(c))], axis=1)
    return out
