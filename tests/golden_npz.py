"""Golden fixtures stored in pieces: a fixture `<stem>.npz` larger than PIECE bytes is kept as `<stem>.1.npz`,
`<stem>.2.npz`, ... (every committed file stays below 1 MiB); an array too large for one piece is split by rows
into `<key>@0`, `<key>@1`, ... and joined again on loading.  load() returns {key: ndarray} either way."""
import glob
import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PIECE = 900 * 1024


def load(name):
    """The fixture tests/golden/<name> (one file, or its pieces) as {key: ndarray}."""
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    stem = path[:-len(".npz")]
    pieces = sorted(glob.glob(stem + ".[0-9]*.npz"), key=lambda p: int(p[len(stem) + 1:-len(".npz")]))
    if not pieces:
        raise FileNotFoundError(path)
    parts = {}
    for p in pieces:
        with np.load(p) as z:
            parts.update({k: z[k] for k in z.files})
    out = {k: v for k, v in parts.items() if "@" not in k}
    for k in sorted({k.split("@")[0] for k in parts if "@" in k}):
        n = sum(1 for j in parts if j.split("@")[0] == k and "@" in j)
        out[k] = np.concatenate([parts["%s@%d" % (k, i)] for i in range(n)], axis=0)
    return out


def _zsize(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def save(path, arrays):
    """Write `arrays` as the fixture `path` (np.savez_compressed), in pieces below PIECE bytes when it does not fit."""
    for old in glob.glob(path[:-len(".npz")] + ".[0-9]*.npz") + [path]:
        if os.path.exists(old):
            os.remove(old)
    if _zsize(arrays) <= PIECE:
        np.savez_compressed(path, **arrays)
        return [path]
    items = []
    for k, v in arrays.items():
        v = np.asarray(v)
        n = 1
        while v.ndim and v.shape[0] >= 2 * n and _zsize({k: v[:-(-v.shape[0] // n)]}) > PIECE * 0.9:
            n *= 2
        if n == 1:
            items.append((k, v))
        else:
            rows = -(-v.shape[0] // n)
            items += [("%s@%d" % (k, i), v[i * rows:(i + 1) * rows]) for i in range(-(-v.shape[0] // rows))]
    pieces, cur = [], {}
    for k, v in items:
        if cur and _zsize(dict(cur, **{k: v})) > PIECE:
            pieces.append(cur)
            cur = {}
        cur[k] = v
    pieces.append(cur)
    out = []
    for i, p in enumerate(pieces, 1):
        out.append(path[:-len(".npz")] + ".%d.npz" % i)
        np.savez_compressed(out[-1], **p)
    return out
