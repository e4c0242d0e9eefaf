"""Reading and writing the .npz fixtures of this directory.

Every committed file stays under 1 MiB, so a fixture that does not fit is stored in parts: `<name>.npz` holds its first
arrays and `<name>.part2.npz`, `<name>.part3.npz`, ... the rest, in the original order.  `load` joins them into one
mapping with the `files` list and `[key]` access of numpy's NpzFile; a fixture in one file is returned by np.load itself.
"""
import io
import os
import zipfile

import numpy as np

MAX_FILE_BYTES = 1 << 20


class Fixture(dict):
    """The arrays of a fixture stored in parts, in their original order."""

    @property
    def files(self):
        return list(self.keys())


def part_paths(path):
    stem = path[:-len(".npz")]
    paths, n = [path], 2
    while os.path.exists(f"{stem}.part{n}.npz"):
        paths.append(f"{stem}.part{n}.npz")
        n += 1
    return paths


def load(path):
    paths = part_paths(path)
    if len(paths) == 1:
        return np.load(path)
    out = Fixture()
    for p in paths:
        with np.load(p) as z:
            for k in z.files:
                assert k not in out, f"{k} is in more than one part of {path}"
                out[k] = z[k]
    return out


def _savez(path, arrays):
    """np.savez_compressed at the highest deflate level."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.save(buf, np.asanyarray(v), allow_pickle=False)
            z.writestr(k + ".npy", buf.getvalue())


def save(path, arrays):
    """Write `arrays` (an ordered mapping) as one .npz, or in as few parts of about equal raw size as keep every file
    under MAX_FILE_BYTES."""
    for p in part_paths(path)[1:]:
        os.remove(p)
    keys = list(arrays)
    total = sum(np.asanyarray(arrays[k]).nbytes for k in keys)
    for n in range(1, len(keys) + 1):
        parts, size = [[]], 0
        for k in keys:
            nb = np.asanyarray(arrays[k]).nbytes
            if parts[-1] and len(parts) < n and size + nb > total / n:
                parts.append([])
                size = 0
            parts[-1].append(k)
            size += nb
        paths = [path] + [f"{path[:-len('.npz')]}.part{i}.npz" for i in range(2, len(parts) + 1)]
        for p, ks in zip(paths, parts):
            _savez(p, {k: arrays[k] for k in ks})
        if all(os.path.getsize(p) < MAX_FILE_BYTES for p in paths):
            return paths
        for p in paths[1:]:
            os.remove(p)
    raise ValueError(f"{path}: one array alone is larger than {MAX_FILE_BYTES} bytes compressed")
