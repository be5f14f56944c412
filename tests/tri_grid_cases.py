"""The small sheet the triangle-grid tests share (tests/test_tri_grid_host.py, tests/test_gpu_surface_icp.py): 13 x 13 vertices over the
unit square, 288 triangles -- one full 256-triangle tile plus 32, so the last tile and its last quarter are partial."""
import numpy as np


def sheet(bumpy=True, n=13):
    xs = np.linspace(0.0, 1.0, n)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    Z = 0.08 * np.sin(5.0 * X) * np.cos(4.0 * Y) + np.random.default_rng(3).normal(0.0, 0.004, X.shape) if bumpy else np.zeros_like(X)
    v = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)
    return v, tris
