"""The context wrapper: `Context` (gingr_ctx: one device, one stream, the stateless all-pairs and mesh operators) and `_check`, which
turns a native error code into a GingrNativeError.  Everything else in the package is built on these two."""
from __future__ import annotations

import ctypes
import dataclasses
from ctypes import c_int64, c_void_p
from typing import Optional, Tuple

import numpy as np

from . import _native as nat
from ._native import GingrNativeError, f64, dptr, iptr


def _check(ctx_handle, code: int, where: str):
    if code != nat.GINGR_OK:
        text = ""
        if ctx_handle:
            text = (nat.load().gingr_last_error(ctx_handle) or b"").decode("utf-8", "replace")
        raise GingrNativeError(code, where, text)


@dataclasses.dataclass
class RigidSearchResult:
    """What Context.rigid_search returns: the winner (best, R, t, score) and every pose's end state -- rotations (S, 3, 3), translations
    (S, 3), scores (S,), kept (S,) pairs of the scoring pass, failed (S,) -- so that the runner-up basins of a near-symmetric shape can
    be inspected."""
    best: int
    R: np.ndarray
    t: np.ndarray
    score: float
    rotations: np.ndarray
    translations: np.ndarray
    scores: np.ndarray
    kept: np.ndarray
    failed: np.ndarray


@dataclasses.dataclass
class RigidSearchPosesResult(RigidSearchResult):
    """What Context.rigid_search_poses returns: a RigidSearchResult with inliers (S,), the moving points of every pose within the
    inlier distance of the target in the scoring pass.  The field is defaulted, so a record built without it is the plain one."""
    inliers: Optional[np.ndarray] = None


# ----------------------------------------------------------------------------- context + operators
class Context:
    """One device + one stream (gingr_ctx).  Not thread-safe; one per chain / per GPU."""

    def __init__(self, device: int = 0):
        self._lib = nat.load()
        h = c_void_p()
        code = self._lib.gingr_ctx_create(int(device), ctypes.byref(h))
        if code != nat.GINGR_OK:
            raise GingrNativeError(code, "gingr_ctx_create", "(no usable GPU: this package has no CPU path)")
        self.handle = h
        self.device = device

    def close(self):
        if getattr(self, "handle", None):
            self._lib.gingr_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(self.handle, self._lib.gingr_ctx_synchronize(self.handle), "gingr_ctx_synchronize")

    def set_stream(self, hip_stream: Optional[int]):
        _check(self.handle, self._lib.gingr_ctx_set_stream(self.handle, c_void_p(hip_stream or 0)), "gingr_ctx_set_stream")

    # timing hooks (bench.py roofline)
    def get_stream(self) -> int:
        """The hipStream_t (as an integer) the context's kernels are enqueued on."""
        return int(self._lib.gingr_ctx_get_stream(self.handle) or 0)

    def timing_enable(self, on: bool = True):
        _check(self.handle, self._lib.gingr_ctx_timing_enable(self.handle, 1 if on else 0), "timing_enable")

    def timing_reset(self):
        _check(self.handle, self._lib.gingr_ctx_timing_reset(self.handle), "timing_reset")

    def timing_read(self, which: int) -> Tuple[float, int]:
        ms = ctypes.c_double()
        n = c_int64()
        _check(self.handle, self._lib.gingr_ctx_timing_read(self.handle, which, ctypes.byref(ms), ctypes.byref(n)), "timing_read")
        return ms.value, n.value

    def set_option(self, option: int, value: int):
        """gingr_ctx_set_option: nat.OPT_CULL / OPT_FINE_CULL / OPT_NN_GRID -- code paths with identical results (tests, A/B timing)."""
        _check(self.handle, self._lib.gingr_ctx_set_option(self.handle, int(option), int(value)), "gingr_ctx_set_option")

    def get_option(self, option: int) -> int:
        v = ctypes.c_int32()
        _check(self.handle, self._lib.gingr_ctx_get_option(self.handle, int(option), ctypes.byref(v)), "gingr_ctx_get_option")
        return int(v.value)

    # ---- native RCCL exchange (one process per GPU; the library enqueues ncclAllReduce on this context's stream)
    def rccl_load(self, path: Optional[str] = None):
        """Bind a specific librccl (default: the copy already loaded in the process, e.g. torch's, else the loader's search path)."""
        _check(self.handle, self._lib.gingr_rccl_load(self.handle, path.encode() if path else None), "gingr_rccl_load")

    def rccl_unique_id(self) -> bytes:
        """ncclGetUniqueId: rank 0 creates it, the host distributes the 128 bytes to every rank."""
        buf = ctypes.create_string_buffer(nat.RCCL_UNIQUE_ID_BYTES)
        _check(self.handle, self._lib.gingr_rccl_unique_id(self.handle, buf), "gingr_rccl_unique_id")
        return bytes(buf.raw)

    def rccl_init(self, unique_id: bytes, world: int, rank: int):
        """ncclCommInitRank on this context's device (collective over the `world` ranks); the communicator dies with the context."""
        assert len(unique_id) == nat.RCCL_UNIQUE_ID_BYTES
        buf = ctypes.create_string_buffer(unique_id, nat.RCCL_UNIQUE_ID_BYTES)
        _check(self.handle, self._lib.gingr_ctx_rccl_init(self.handle, buf, int(world), int(rank)), "gingr_ctx_rccl_init")

    def rccl_info(self) -> dict:
        w, r, v = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        path = ctypes.create_string_buffer(512)
        _check(self.handle, self._lib.gingr_ctx_rccl_info(self.handle, ctypes.byref(w), ctypes.byref(r), ctypes.byref(v), path, 512),
               "gingr_ctx_rccl_info")
        return {"world": int(w.value), "rank": int(r.value), "version": int(v.value), "library": path.value.decode()}

    def rccl_allreduce(self, device_ptr: int, count: int):
        """In-place float64 sum all-reduce of `count` elements at `device_ptr`, enqueued on this context's stream."""
        _check(self.handle, self._lib.gingr_ctx_rccl_allreduce_async(self.handle, c_void_p(int(device_ptr)), int(count)),
               "gingr_ctx_rccl_allreduce_async")

    def nn_counting(self, on: bool = True):
        """Diagnostics: count the distance tests the nearest-neighbour launches of this context really execute (clears the counter)."""
        _check(self.handle, self._lib.gingr_ctx_nn_counting(self.handle, 1 if on else 0), "nn_counting")

    def nn_tests(self) -> int:
        n = c_int64()
        _check(self.handle, self._lib.gingr_ctx_nn_tests(self.handle, ctypes.byref(n)), "nn_tests")
        return int(n.value)

    # ---- stateless all-pairs operators -------------------------------------------------
    def cpd_stats(self, fit, target, sigma2: float, w: float = 0.0) -> dict:
        """CPD statistics of one affinity evaluation (CPD.scala:54-75,36,133-147), P never materialised."""
        y, x = f64(fit), f64(target)
        M, N = y.shape[0], x.shape[0]
        den, Pt1 = np.empty(N), np.empty(N)
        P1, PX, sc = np.empty(M), np.empty((M, 3)), np.empty(6)
        _check(self.handle, self._lib.gingr_cpd_stats(self.handle, M, dptr(y), N, dptr(x), float(sigma2), float(w),
                                                      dptr(den), dptr(P1), dptr(PX), dptr(Pt1), dptr(sc)), "gingr_cpd_stats")
        return dict(den=den, P1=P1, PX=PX, Pt1=Pt1, Np=float(sc[0]), xPx=float(sc[1]), trPXY=float(sc[2]),
                    yPy=float(sc[3]), sigma2_next=float(sc[4]), c=float(sc[5]))

    def cpd_initial_sigma2(self, reference, target) -> float:
        y, x = f64(reference), f64(target)
        out = ctypes.c_double()
        _check(self.handle, self._lib.gingr_cpd_initial_sigma2(self.handle, y.shape[0], dptr(y), x.shape[0], dptr(x),
                                                               ctypes.byref(out)), "gingr_cpd_initial_sigma2")
        return out.value

    def nn(self, query, target) -> Tuple[np.ndarray, np.ndarray, float]:
        """Exact nearest neighbour, lowest index on ties (ClosestPointRegistrator.scala:133-148)."""
        y, x = f64(query), f64(target)
        idx = np.empty(y.shape[0], dtype=np.int32)
        d2 = np.empty(y.shape[0])
        md = ctypes.c_double()
        _check(self.handle, self._lib.gingr_nn(self.handle, y.shape[0], dptr(y), x.shape[0], dptr(x), iptr(idx), dptr(d2),
                                               ctypes.byref(md)), "gingr_nn")
        return idx, d2, md.value

    def cloud_knn(self, points, k: int, info: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The k nearest neighbours of every point of a cloud within the cloud itself -- gingr_cloud_knn: (idx (N, k) int32, d2 (N, k)),
        each row sorted ascending by (d2, index), the point itself (or a lower-indexed duplicate) first; ties go to the lowest index and
        d2 has the bits of dx*dx + dy*dy + dz*dz in float64.  3 <= k <= 64, k <= N.  info: a dict that receives the grid's cell_size,
        its dimensions and the number of queries the grid could not certify (answered by a scan of the whole cloud)."""
        x = f64(points).reshape(-1, 3)
        n = x.shape[0]
        idx, d2 = np.empty((n, max(int(k), 0)), dtype=np.int32), np.empty((n, max(int(k), 0)))
        ki = nat.CloudKnnInfo()
        _check(self.handle, self._lib.gingr_cloud_knn(self.handle, n, dptr(x), int(k), iptr(idx), dptr(d2), ctypes.byref(ki)), "gingr_cloud_knn")
        if info is not None:
            info.update(cell_size=float(ki.cell_size), grid=tuple(int(g) for g in ki.grid), flagged=int(ki.flagged))
        return idx, d2

    def cloud_normals(self, points, k: int = 16, viewpoint=None, info: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
        """A normal per point of an unorganised cloud from the PCA of its k nearest neighbours (Hoppe et al.) -- gingr_cloud_normals:
        (normals (N, 3), variation (N,)).  The normal is the unit eigenvector of the smallest eigenvalue of the neighbourhood's
        covariance, the zero vector where that direction is not defined (coincident points, a line, an isotropic blob); its largest
        component is positive, or with a viewpoint (3,) it points towards the viewpoint.  variation = lam0 / trace, 0 on a plane."""
        x = f64(points).reshape(-1, 3)
        n = x.shape[0]
        v = None if viewpoint is None else f64(viewpoint).reshape(3)
        normals, var = np.empty((n, 3)), np.empty(n)
        ki = nat.CloudKnnInfo()
        _check(self.handle, self._lib.gingr_cloud_normals(self.handle, n, dptr(x), int(k), dptr(v), dptr(normals), dptr(var), ctypes.byref(ki)),
               "gingr_cloud_normals")
        if info is not None:
            info.update(cell_size=float(ki.cell_size), grid=tuple(int(g) for g in ki.grid), flagged=int(ki.flagged))
        return normals, var

    def order_statistic(self, values, k: int) -> float:
        """The k-th smallest (0-based) of non-negative values, the element itself bit for bit -- gingr_order_statistic: the exact radix
        selection behind the robust scale of point-to-plane ICP, as an operator.  +inf is a value; a negative or NaN value raises."""
        v = f64(values).reshape(-1)
        out = ctypes.c_double()
        _check(self.handle, self._lib.gingr_order_statistic(self.handle, v.shape[0], dptr(v), int(k), ctypes.byref(out)), "gingr_order_statistic")
        return float(out.value)

    def rotation_samples(self, n: int) -> np.ndarray:
        """The n rotations (n, 3, 3) of the super-Fibonacci spiral over SO(3) (Alexa 2022) -- gingr_rotation_samples: the default start
        rotations of rigid_search.  Computed on the host."""
        if int(n) < 1:
            raise ValueError("n >= 1 required")
        out = np.empty((int(n), 3, 3))
        _check(self.handle, self._lib.gingr_rotation_samples(int(n), dptr(out)), "gingr_rotation_samples")
        return out

    def rigid_search(self, moving, target, rotations=64, iterations: int = 10, overlap: float = 1.0) -> "RigidSearchResult":
        """Global rigid pre-alignment -- gingr_rigid_search: every start rotation (a count of spiral samples, or an (S, 3, 3) array) gives
        the start pose R0 (x - mean moving) + mean target; all poses run `iterations` iterations of trimmed ICP (the `overlap` fraction
        of closest pairs is kept, ties included) together on the device, and the pose of the smallest score sqrt(mean kept d2) wins,
        the lowest index on ties.  p -> R p + t maps `moving` onto `target`."""
        x, y = f64(moving).reshape(-1, 3), f64(target).reshape(-1, 3)
        r0 = self.rotation_samples(rotations) if np.ndim(rotations) == 0 else f64(rotations).reshape(-1, 3, 3)
        S = r0.shape[0]
        best = c_int64(-1)
        poses, scores = np.empty((S, 12)), np.empty(S)
        kept, failed = np.empty(S, dtype=np.int64), np.empty(S, dtype=np.int32)
        _check(self.handle, self._lib.gingr_rigid_search(self.handle, x.shape[0], dptr(x), y.shape[0], dptr(y), S, dptr(r0), int(iterations),
                                                         float(overlap), ctypes.byref(best), dptr(poses), dptr(scores),
                                                         kept.ctypes.data_as(ctypes.POINTER(c_int64)), iptr(failed)), "gingr_rigid_search")
        b = int(best.value)
        rot, tr = poses[:, :9].reshape(S, 3, 3).copy(), poses[:, 9:].copy()
        return RigidSearchResult(best=b, R=rot[b].copy(), t=tr[b].copy(), score=float(scores[b]), rotations=rot, translations=tr,
                                 scores=scores, kept=kept, failed=failed.astype(bool))

    def rigid_search_poses(self, moving, target, poses, iterations: int = 10, overlap: float = 1.0, inlierDistance: float = 0.0,
                           select: int = 0) -> "RigidSearchPosesResult":
        """rigid_search from given start poses -- gingr_rigid_search_poses: poses (S, 12), R row-major then t (or a pair (R (S, 3, 3),
        t (S, 3))).  A pose with a non-finite word is failed from the start and takes no part.  inliers = the moving points with
        d2 <= inlierDistance^2 in the scoring pass; select 0 picks the smallest score, 1 the most inliers, then the smaller score, then
        the lowest index.  Given (R0, mean target - R0 mean moving) the outputs are rigid_search's, bit for bit."""
        x, y = f64(moving).reshape(-1, 3), f64(target).reshape(-1, 3)
        if isinstance(poses, tuple):
            poses = np.concatenate([f64(poses[0]).reshape(-1, 9), f64(poses[1]).reshape(-1, 3)], axis=1)
        p = f64(poses).reshape(-1, 12)
        S = p.shape[0]
        best = c_int64(-1)
        out, scores = np.empty((S, 12)), np.empty(S)
        kept, failed, inliers = np.empty(S, dtype=np.int64), np.empty(S, dtype=np.int32), np.empty(S, dtype=np.int64)
        i64 = ctypes.POINTER(c_int64)
        _check(self.handle, self._lib.gingr_rigid_search_poses(self.handle, x.shape[0], dptr(x), y.shape[0], dptr(y), S, dptr(p), int(iterations),
                                                               float(overlap), float(inlierDistance), int(select), ctypes.byref(best),
                                                               dptr(out), dptr(scores), kept.ctypes.data_as(i64), iptr(failed),
                                                               inliers.ctypes.data_as(i64)), "gingr_rigid_search_poses")
        b = int(best.value)
        rot, tr = out[:, :9].reshape(S, 3, 3).copy(), out[:, 9:].copy()
        return RigidSearchPosesResult(best=b, R=rot[b].copy(), t=tr[b].copy(), score=float(scores[b]), rotations=rot, translations=tr,
                                      scores=scores, kept=kept, failed=failed.astype(bool), inliers=inliers)

    def cloud_fpfh(self, points, normals, k: int = 64, radius: float = 0.0, info: Optional[dict] = None
                   ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Fast Point Feature Histograms of a cloud with normals -- gingr_cloud_fpfh, this package's definition (include/gingr_hip.h):
        (fpfh (N, 33), counts (N, 33) int32, valid (N,) int32).  The neighbours of a point are the entries of its k-nearest list within
        `radius` (required, > 0); a zero normal means "none" and its pairs are skipped.  3 <= k <= 64, k <= N."""
        x, n = f64(points).reshape(-1, 3), f64(normals).reshape(-1, 3)
        if n.shape[0] != x.shape[0]:
            raise ValueError("one normal per point required")
        N = x.shape[0]
        fpfh, counts, valid = np.empty((N, 33)), np.empty((N, 33), dtype=np.int32), np.empty(N, dtype=np.int32)
        ki = nat.CloudKnnInfo()
        _check(self.handle, self._lib.gingr_cloud_fpfh(self.handle, N, dptr(x), dptr(n), int(k), float(radius), iptr(counts), iptr(valid),
                                                       dptr(fpfh), ctypes.byref(ki)), "gingr_cloud_fpfh")
        if info is not None:
            info.update(cell_size=float(ki.cell_size), grid=tuple(int(g) for g in ki.grid), flagged=int(ki.flagged))
        return fpfh, counts, valid

    def feature_match(self, a, b) -> Tuple[np.ndarray, np.ndarray]:
        """For every row of a (M, D) the closest row of b (N, D) in feature space -- gingr_feature_match: (idx (M,) int32, d2 (M,)),
        d2 = sum_c (a_c - b_c)^2 added in ascending c with the bits of that expression in float64, the lowest index on ties.  D <= 64."""
        a, b = f64(a), f64(b)
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
            raise ValueError("two matrices with the same number of columns required")
        idx, d2 = np.empty(a.shape[0], dtype=np.int32), np.empty(a.shape[0])
        _check(self.handle, self._lib.gingr_feature_match(self.handle, a.shape[0], dptr(a), b.shape[0], dptr(b), a.shape[1], iptr(idx), dptr(d2)),
               "gingr_feature_match")
        return idx, d2

    def rigid_poses_from_triples(self, moving, target, triMoving, triTarget) -> Tuple[np.ndarray, np.ndarray]:
        """The rigid pose of every triple of pairs (moving[triMoving[h]], target[triTarget[h]]) -- gingr_rigid_poses_from_triples:
        (poses (H, 12): R row-major then t, degenerate (H,) bool).  A degenerate triple (a repeated index, a triangle without area in
        either cloud) gives a NaN pose, which rigid_search_poses passes over."""
        x, y = f64(moving).reshape(-1, 3), f64(target).reshape(-1, 3)
        tm = np.ascontiguousarray(triMoving, dtype=np.int32).reshape(-1, 3)
        tt = np.ascontiguousarray(triTarget, dtype=np.int32).reshape(-1, 3)
        if tm.shape != tt.shape:
            raise ValueError("as many target triples as moving triples required")
        H = tm.shape[0]
        poses, deg = np.empty((H, 12)), np.empty(H, dtype=np.int32)
        _check(self.handle, self._lib.gingr_rigid_poses_from_triples(self.handle, x.shape[0], dptr(x), y.shape[0], dptr(y), H, iptr(tm), iptr(tt),
                                                                     dptr(poses), iptr(deg)), "gingr_rigid_poses_from_triples")
        return poses, deg.astype(bool)

    def gauss_block(self, A, B, sigma: float, scaling: float) -> np.ndarray:
        """scaling * exp(-|a-b|^2 / sigma^2)  (GPMMHelper.scala:99-102)."""
        A, B = f64(A), f64(B)
        out = np.empty((A.shape[0], B.shape[0]))
        _check(self.handle, self._lib.gingr_gauss_block(self.handle, A.shape[0], dptr(A), B.shape[0], dptr(B), float(sigma),
                                                        float(scaling), dptr(out)), "gingr_gauss_block")
        return out

    def mesh_distance_stats(self, points, vertices, cells, boundary_aware: bool = False, sdev: float = 0.0
                            ) -> Tuple[float, float, int, float]:
        """(sum, max, count, sum of log N(d; 0, sdev)) of d = |p - closestPointOnSurface(p)| for the rows of `points` against
        the triangle mesh (vertices, cells); boundary_aware as RegistrationComparison.avgDistanceBoundaryAware (:63-73)."""
        p, v = f64(points), f64(vertices)
        c = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
        out = np.zeros(4)
        _check(self.handle, self._lib.gingr_mesh_distance_stats(self.handle, p.shape[0], dptr(p), v.shape[0], dptr(v), c.shape[0],
                                                                iptr(c), int(bool(boundary_aware)), float(sdev), dptr(out)),
               "gingr_mesh_distance_stats")
        return float(out[0]), float(out[1]), int(out[2]), float(out[3])

    def mesh_set_distances(self, sets, meshes, cells, pairing: str = "all", corresponding: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """(avg, max) of d = |p - closestPointOnSurface(p)| over the points of every query set (n_sets x n_points x 3) against the meshes
        (n_meshes x n_vertices x 3) that share the triangles `cells` -- gingr_mesh_set_distances, one batched pass.  pairing "all":
        every set against every mesh, (n_sets, n_meshes) each; "cyclic": set c against mesh c % n_meshes, (n_sets,) each.  The direction
        is set -> mesh surface: per pair what mesh_distance_stats(set, mesh, cells) gives as sum / count and max (max bit for bit, avg to
        the order of the sum).  corresponding=True (n_points == n_vertices) declares that point k of a set lies near vertex k of the
        mesh: a hint that seeds the search and never changes a bit."""
        S, V = f64(sets), f64(meshes)
        S, V = (S[None] if S.ndim == 2 else S), (V[None] if V.ndim == 2 else V)
        if S.ndim != 3 or S.shape[2] != 3 or V.ndim != 3 or V.shape[2] != 3:
            raise ValueError(f"sets / meshes: expected (n, points, 3), got {S.shape} and {V.shape}")
        if pairing not in ("all", "cyclic"):
            raise ValueError(f"pairing: 'all' or 'cyclic', got {pairing!r}")
        c = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
        shape = (S.shape[0], V.shape[0]) if pairing == "all" else (S.shape[0],)
        avg, mx = np.empty(shape), np.empty(shape)
        _check(self.handle, self._lib.gingr_mesh_set_distances(self.handle, S.shape[1], S.shape[0], dptr(S), V.shape[1], V.shape[0], dptr(V),
                                                               c.shape[0], iptr(c), 0 if pairing == "all" else 1, int(bool(corresponding)),
                                                               dptr(avg), dptr(mx)), "gingr_mesh_set_distances")
        return avg, mx

    def mesh_closest_points(self, points, vertices, cells) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """mesh.operations.closestPointOnSurface for every row of `points`: (closest points (n,3), squared distances (n,), triangle
        ids (n,), barycentric weights of that triangle's corners (n,3)) -- gingr_mesh_closest_points."""
        p, v = f64(points).reshape(-1, 3), f64(vertices).reshape(-1, 3)
        c = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
        n = p.shape[0]
        cp, d2, tid, bary = np.empty((n, 3)), np.empty(n), np.empty(n, dtype=np.int32), np.empty((n, 3))
        _check(self.handle, self._lib.gingr_mesh_closest_points(self.handle, n, dptr(p), v.shape[0], dptr(v), c.shape[0], iptr(c),
                                                                dptr(cp), dptr(d2), iptr(tid), dptr(bary)),
               "gingr_mesh_closest_points")
        return cp, d2, tid, bary

    def mesh_decimate(self, vertices, cells, n_target: int) -> Tuple[np.ndarray, Optional[np.ndarray], float]:
        """Vertex clustering to about `n_target` vertices on the device -- gingr_mesh_decimate, the result of
        `gingr_amd.simple.cluster_decimate` bit for bit: (kept vertex ids, ascending (k,) int32; the re-indexed triangles (t,3) int32,
        or None for a point cloud (cells=None); the chosen cube size, 0.0 when nothing was decimated)."""
        v = f64(vertices).reshape(-1, 3)
        c = None if cells is None else np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
        n, t = v.shape[0], 0 if c is None else c.shape[0]
        kept = np.empty(max(n, 1), dtype=np.int32)
        out = None if c is None else np.empty((max(t, 1), 3), dtype=np.int32)
        nk, nt, h = c_int64(), c_int64(), ctypes.c_double()
        _check(self.handle, self._lib.gingr_mesh_decimate(self.handle, n, dptr(v), t, iptr(c), int(n_target), ctypes.byref(nk), iptr(kept),
                                                          ctypes.byref(nt), iptr(out), ctypes.byref(h)), "gingr_mesh_decimate")
        return kept[:nk.value].copy(), None if c is None else out[:nt.value].copy(), h.value

