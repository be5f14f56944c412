"""Plain-loop restatement of gingr_mesh_decimate (include/gingr_hip.h) in the order its kernels work, and the inputs the two test
modules share.  No tests in here: test_mesh_decimate_host.py checks it against gingr_amd.simple.cluster_decimate (the definition),
test_gpu_mesh_decimate.py checks the device against that definition on the same inputs.

On purpose none of numpy's set machinery: a dict for the cells (the device's hash table), per-cluster sums added in ascending vertex
number (the device's sorted runs), the two-pass integer argmin, flag / running count / scatter, and the first triangle of every corner
set found through a dict keyed by the sorted triple.  Every float operation is a Python float operation, i.e. one IEEE double
operation, in the order gingr_amd/csrc/decimate_bisect.h and mesh_decimate.hip spell out."""
from __future__ import annotations

import math
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_STEPS = 60


# ------------------------------------------------------------------------------------------------------------------ the recurrence
def bisect(extent: float, counts, n_target: int):
    """decimate_bisect_init / decimate_bisect_step fed with `counts(mid) -> distinct cells` (a callable, or a sequence consumed one per
    step): returns (h, steps, accepted, mids)."""
    nxt = counts if callable(counts) else (lambda mid, it=iter(counts): next(it))
    lo, hi = extent * 1e-6, extent * 2.0
    h, steps, accepted, mids = lo, 0, False, []
    while True:
        mid = math.sqrt(lo * hi)
        mids.append(mid)
        if nxt(mid) >= n_target:
            accepted, h, lo = True, mid, mid
        else:
            hi = mid
        steps += 1
        if hi / lo < 1.0005 or steps >= MAX_STEPS:
            break
    return (h if accepted else lo), steps, accepted, mids


def cell_key(p, lo_corner, h: float) -> int:
    """decimate_cell_key: 21 bits per axis."""
    k = 0
    for d in range(3):
        k |= (int(math.floor((p[d] - lo_corner[d]) / h)) & ((1 << 21) - 1)) << (21 * d)
    return k


def _bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ------------------------------------------------------------------------------------------------------------------ the algorithm
def decimate(vertices, cells, n_target: int):
    """(kept ids ascending int32, cells int32 or None, cube size) -- what Context.mesh_decimate returns."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    c = None if cells is None else np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    n = v.shape[0]
    if n_target >= n:
        return np.arange(n, dtype=np.int32), None if c is None else c.astype(np.int32), 0.0
    P = [tuple(float(x) for x in row) for row in v]
    lo_corner = [min(p[d] for p in P) for d in range(3)]
    hi_corner = [max(p[d] for p in P) for d in range(3)]
    extent = max(hi_corner[d] - lo_corner[d] for d in range(3))
    if extent == 0.0:
        extent = 1.0

    def slots(h):
        table, slot = {}, [0] * n
        for i, p in enumerate(P):
            slot[i] = table.setdefault(cell_key(p, lo_corner, h), len(table))
        return slot, len(table)

    h, _, _, _ = bisect(extent, lambda mid: slots(mid)[1], n_target)
    slot, k = slots(h)
    # sums in ascending vertex number, then the mean
    s = [[0.0, 0.0, 0.0] for _ in range(k)]
    cnt = [0] * k
    for i, p in enumerate(P):
        a = s[slot[i]]
        a[0] += p[0]
        a[1] += p[1]
        a[2] += p[2]
        cnt[slot[i]] += 1
    mean = [(s[q][0] / float(cnt[q]), s[q][1] / float(cnt[q]), s[q][2] / float(cnt[q])) for q in range(k)]
    # two integer passes: the smallest bit pattern of d2, then the smallest number among those that have it
    d2bits = [0] * n
    min_bits = [(1 << 64) - 1] * k
    for i, p in enumerate(P):
        m = mean[slot[i]]
        dx, dy, dz = p[0] - m[0], p[1] - m[1], p[2] - m[2]
        d2bits[i] = _bits((dx * dx + dy * dy) + dz * dz)
        min_bits[slot[i]] = min(min_bits[slot[i]], d2bits[i])
    min_number = [n] * k
    for i in range(n):
        if d2bits[i] == min_bits[slot[i]]:
            min_number[slot[i]] = min(min_number[slot[i]], i)
    # flag, running count, scatter
    kept, new_id, run = [], [0] * k, 0
    for i in range(n):
        if min_number[slot[i]] == i:
            kept.append(i)
            new_id[slot[i]] = run
            run += 1
    kept = np.array(kept, dtype=np.int32)
    if c is None:
        return kept, None, h
    rtri = [tuple(new_id[slot[int(a)]] for a in t) for t in c]
    first = {}
    for t, (a, b, d) in enumerate(rtri):
        if a == b or b == d or a == d:
            continue
        key = tuple(sorted((a, b, d)))
        first[key] = min(first.get(key, t), t)
    out = [tr for t, tr in enumerate(rtri)
           if not (tr[0] == tr[1] or tr[1] == tr[2] or tr[0] == tr[2]) and first[tuple(sorted(tr))] == t]
    return kept, np.array(out, dtype=np.int32).reshape(-1, 3), h


def cluster_decimate(vertices, cells, n_target: int):
    """The restatement with gingr_amd.simple.cluster_decimate's return value."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    kept, c, _ = decimate(v, cells, n_target)
    return v[kept].copy(), c


# ------------------------------------------------------------------------------------------------------------------ the inputs
def femur():
    d = np.load(os.path.join(HERE, "golden", "inputs.npz"))
    m = np.load(os.path.join(HERE, "golden", "femur_mesh.npz"))
    return d["femur"].astype(np.float64), np.asarray(m["femur_cells"])


FEMUR_TARGETS = (1, 2, 100, 400, 1000, 1621, 1622, 10 ** 6)
CLOUD_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
LATTICE_TARGETS = (8, 27, 100)


def cloud(n: int) -> np.ndarray:
    return np.random.default_rng(1000 + n).normal(0.0, 25.0, (n, 3))


def cloud_targets(n: int):
    return sorted({t for t in (1, 2, (n + 1) // 2, n - 1) if t >= 1})


def lattice(shifted: bool) -> np.ndarray:
    g = np.arange(12, dtype=np.float64)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return p + np.array([1e6, -1e6, 0.5]) if shifted else p


def repeated_positions() -> np.ndarray:
    """300 points, 40 distinct positions: no cube size ever reaches 100 cells."""
    rng = np.random.default_rng(5)
    return rng.normal(0.0, 10.0, (40, 3))[rng.integers(0, 40, 300)]


def degenerate(kind: str) -> np.ndarray:
    rng = np.random.default_rng(6)
    if kind == "identical":
        return np.tile(np.array([[3.25, -1.5, 7.0]]), (50, 1))
    if kind == "line":
        return np.outer(rng.uniform(-40.0, 40.0, 200), np.array([1.0, 0.0, 0.0])) + np.array([2.0, 5.0, -3.0])
    if kind == "plane":
        p = rng.uniform(-30.0, 30.0, (300, 3))
        p[:, 2] = 4.0
        return p
    raise ValueError(kind)


DEGENERATE = (("identical", 5), ("line", 20), ("plane", 40))


def grid_surface(m: int):
    """An m x m height field over a square (m * m vertices, 2 (m - 1)^2 triangles); m = 224: 50 176 / 99 458."""
    u = np.linspace(0.0, 1.0, m)
    U, V = np.meshgrid(u, u, indexing="ij")
    rng = np.random.default_rng(m)
    x = 200.0 * U + rng.normal(0.0, 0.05, U.shape)
    y = 200.0 * V + rng.normal(0.0, 0.05, U.shape)
    z = 30.0 * np.sin(5.0 * U) * np.cos(4.0 * V) + 10.0 * U * V
    v = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    i = np.arange(m * m).reshape(m, m)
    a, b, c, d = i[:-1, :-1].ravel(), i[1:, :-1].ravel(), i[:-1, 1:].ravel(), i[1:, 1:].ravel()
    tri = np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)], axis=0)
    return v, tri.astype(np.int32)


def repeated_triangles():
    """Six well separated groups of four close vertices each (at n_target = 6 every group is one cluster; the tests assert that) under
    a small fan of triangles: the list holds the same triangle twice more -- rotated, and with reversed winding --, two that collapse,
    and two that only repeat an earlier one after the clustering."""
    rng = np.random.default_rng(8)
    centres = np.array([[1.0, 1, 1], [11, 1, 1], [1, 11, 1], [11, 11, 1], [6, 6, 9], [6, 1, 14]])
    v = np.concatenate([c + rng.normal(0.0, 0.05, (4, 3)) for c in centres], axis=0)     # vertex 4 g + j: group g
    q = lambda g, j=0: 4 * g + j
    tri = np.array([[q(0), q(1), q(4)], [q(1), q(4), q(0)],                  # the same triangle, rotated
                    [q(4), q(1), q(0)],                                       # and with reversed winding
                    [q(1), q(3), q(4)], [q(3, 1), q(2), q(4, 2)], [q(2), q(0, 3), q(4)],
                    [q(0), q(0, 1), q(1)],                                    # collapses: two corners in one group
                    [q(2, 1), q(2, 2), q(2, 3)],                              # collapses to a point
                    [q(1, 2), q(3, 3), q(4, 1)],                              # equals triangle 3 after the clustering
                    [q(0), q(5), q(1)], [q(1, 1), q(0, 2), q(5, 3)]],         # the second equals the first with reversed winding
                   dtype=np.int32)
    return v, tri
