"""Storage of the .npz fixtures. A fixture is one archive `<name>.npz`, or, where that would pass
the repository's limit of 1 MiB per committed file, parts `<name>.partNN.npz`. In the parts an
array larger than CHUNK_BYTES is stored as flat chunks `<key>@<i>` with `<key>@shape` and
`<key>@n` beside them, and `@keys` (part 00) keeps the fixture's key order. load_golden() gives
back the same dict either way: same keys, order, dtypes, shapes and bits."""
import glob
import os
import zlib

import numpy as np

FILE_LIMIT = 2 ** 20        # bytes, per committed file
PART_BYTES = 900_000        # compressed payload one part is filled to
CHUNK_BYTES = 600_000       # raw bytes of one chunk (deflate never grows it past PART_BYTES)


def _files(root, name):
    single = os.path.join(root, name + ".npz")
    return [single] if os.path.exists(single) else sorted(
        glob.glob(os.path.join(root, name + ".part[0-9][0-9].npz")))


def load_golden(root, name):
    files = _files(root, name)
    if not files:
        raise FileNotFoundError(f"no fixture {name} under {root}")
    raw = {}
    for f in files:
        with np.load(f) as z:
            raw.update({k: z[k] for k in z.files})
    if "@keys" not in raw:
        return raw
    out = {}
    for k in raw["@keys"].tolist():
        if k in raw:
            out[k] = raw[k]
        else:
            flat = np.concatenate([raw[f"{k}@{i}"] for i in range(int(raw[f"{k}@n"]))])
            out[k] = flat.reshape(tuple(raw[f"{k}@shape"].tolist()))
    return out


def save_golden(root, name, arrays):
    """Write the fixture (replacing its earlier files) and return the paths written."""
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    assert not any("@" in k for k in arrays), "'@' is reserved in fixture keys"
    for f in _files(root, name):
        os.remove(f)
    single = os.path.join(root, name + ".npz")
    np.savez_compressed(single, **arrays)
    if os.path.getsize(single) <= PART_BYTES:
        return [single]
    os.remove(single)
    items = [("@keys", np.array(list(arrays)))]
    for k, a in arrays.items():
        if a.nbytes <= CHUNK_BYTES:
            items.append((k, a))
            continue
        per = max(1, CHUNK_BYTES // a.itemsize)
        flat = np.ascontiguousarray(a).reshape(-1)
        chunks = [flat[i:i + per] for i in range(0, flat.size, per)]
        items.append((f"{k}@shape", np.array(a.shape, np.int64)))
        items.append((f"{k}@n", np.array(len(chunks), np.int64)))
        items += [(f"{k}@{i}", c) for i, c in enumerate(chunks)]
    parts, cur, size = [], {}, 0
    for k, a in items:
        est = len(zlib.compress(np.ascontiguousarray(a).tobytes(), 6)) + 256 + 2 * len(k)
        if cur and size + est > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += est
    parts.append(cur)
    assert len(parts) < 100
    paths = []
    for i, part in enumerate(parts):
        p = os.path.join(root, f"{name}.part{i:02d}.npz")
        np.savez_compressed(p, **part)
        assert os.path.getsize(p) < FILE_LIMIT, (p, os.path.getsize(p))
        paths.append(p)
    return paths
