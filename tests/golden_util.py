"""Helpers shared by the golden-vector tests."""
import glob
import hashlib
import io
import os
import re

import numpy as np
import scipy.sparse as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 900 * 1024      # a fixture larger than this is stored as <name>.part<k>.npz files (committed files stay < 1 MiB)


class NpzParts(object):
    """The members of <name>.part0.npz, <name>.part1.npz, ... read as ONE ``np.load`` result (``files``, ``[key]``)."""

    def __init__(self, paths):
        self._parts = [np.load(p) for p in paths]
        self._where = {}
        for z in self._parts:
            for k in z.files:
                assert k not in self._where, k
                self._where[k] = z
        self.files = list(self._where)

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where

    def __iter__(self):
        return iter(self.files)

    def __len__(self):
        return len(self.files)

    def keys(self):
        return list(self.files)

    def close(self):
        for z in self._parts:
            z.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def part_paths(path):
    """<stem>.part<k>.npz beside ``path`` (= <stem>.npz), in k order."""
    stem = path[:-len(".npz")]
    got = glob.glob(glob.escape(stem) + ".part*.npz")
    got = [p for p in got if re.fullmatch(r"\.part\d+\.npz", p[len(stem):])]
    return sorted(got, key=lambda p: int(p[len(stem) + 5:-4]))


def load_npz(path):
    """``np.load(path)``, or the union of its parts when the fixture is stored split (see ``save_npz``)."""
    if os.path.exists(path):
        return np.load(path)
    parts = part_paths(path)
    if not parts:
        raise FileNotFoundError(path)
    return NpzParts(parts)


def load(name):
    return load_npz(os.path.join(GOLDEN, name))


def save_npz(path, arrays, limit=PART_BYTES):
    """``np.savez_compressed(path, **arrays)``; when that file would exceed ``limit`` bytes, the arrays (in order) go to
    <stem>.part0.npz, .part1.npz, ... instead, each at most ``limit`` bytes.  Stale copies of either form are removed.
    Returns the paths written."""
    def packed(d):
        buf = io.BytesIO()
        np.savez_compressed(buf, **d)
        return buf.getvalue()
    for p in part_paths(path) + ([path] if os.path.exists(path) else []):
        os.remove(p)
    whole = packed(arrays)
    if len(whole) <= limit:
        chunks = [(path, whole)]
    else:
        # a zip archive is its members plus one 22-byte end record: members are costed one by one
        empty = len(packed({}))
        chunks, cur, size = [], {}, empty
        for k, v in arrays.items():
            cost = len(packed({k: v})) - empty
            if cur and size + cost > limit:
                chunks.append(packed(cur))
                cur, size = {}, empty
            cur[k] = v
            size += cost
        chunks.append(packed(cur))
        stem = path[:-len(".npz")]
        chunks = [("%s.part%d.npz" % (stem, i), b) for i, b in enumerate(chunks)]
    for p, b in chunks:
        assert len(b) <= limit, (p, len(b))
        with open(p, "wb") as f:
            f.write(b)
    return [p for p, _ in chunks]


def placeholders(L):
    return {'adj': ['adj_%d' % i for i in range(L)], 'madj': ['madj_%d' % i for i in range(L)],
            'fadj': ['fadj_%d' % i for i in range(L)],
            'fields': ['fields_%d' % i for i in range(L + 1)],
            'ffields': ['ffields_%d' % i for i in range(L + 1)],
            'scales': ['scales_%d' % i for i in range(L)], 'labels': 'labels'}


def graph(z, gname):
    ip, ix, d = z[gname + "/indptr"], z[gname + "/indices"], z[gname + "/data"]
    n = ip.shape[0] - 1
    return sp.csr_matrix((d, ix, ip), shape=(n, n))


def cases(z, gname):
    """{case: [it0, it1, it2]} -> sorted list of (case, n_iters)."""
    out = {}
    pre = gname + "/"
    for k in z.files:
        if not k.startswith(pre) or "/it" not in k:
            continue
        case = k[len(pre):].split("/")[0]
        it = int(k[len(pre):].split("/")[1][2:])
        out[case] = max(out.get(case, 0), it + 1)
    return sorted(out.items())


def parse_case(case):
    parts = case.split("_")
    return dict(seed=int(parts[0][1:]), cv=bool(int(parts[1][2:])), imp=bool(int(parts[2][2:])),
                L=int(parts[3][1:]), deg=int(parts[4][1:]))


def flatten_feed(fd):
    flat = {}
    for k, v in fd.items():
        if isinstance(k, tuple):       # ('csr', placeholder): product-only extra
            continue
        if isinstance(v, tuple):
            flat["%s/idx" % k] = np.asarray(v[0], dtype=np.int32).reshape(-1, 2)
            flat["%s/w" % k] = np.asarray(v[1], dtype=np.float32)
            flat["%s/shape" % k] = np.asarray(v[2], dtype=np.int64)
        else:
            flat[str(k)] = np.asarray(v)
    return flat


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_feed_against_golden(z, prefix, fd, big):
    """Bit-exact comparison of a feed-dict with the stored reference output."""
    flat = flatten_feed(fd)
    stored = [k for k in z.files if k.startswith(prefix + "/") and not k.endswith("/ids")]
    names = set()
    for k in stored:
        names.add(k[len(prefix) + 1:].split("#")[0])
    assert names == set(flat.keys()), (prefix, sorted(names ^ set(flat.keys())))
    for name, arr in flat.items():
        if big:
            assert tuple(z["%s/%s#shape" % (prefix, name)]) == arr.shape, (prefix, name)
            assert np.array_equal(z["%s/%s#sha" % (prefix, name)], digest(_canon(arr, name))), (prefix, name)
        else:
            ref = z["%s/%s" % (prefix, name)]
            assert bits_equal(_canon(arr, name), ref), (prefix, name, arr, ref)


def _canon(arr, name):
    if name.endswith("/idx"):
        return np.ascontiguousarray(arr, dtype=np.int32).reshape(-1, 2)
    if name.endswith("/w"):
        return np.ascontiguousarray(arr, dtype=np.float32)
    if name.endswith("/shape"):
        return np.ascontiguousarray(arr, dtype=np.int64)
    return np.ascontiguousarray(arr)
