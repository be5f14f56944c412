"""Device memory comes back: create / estimate / run / destroy cycles of a fitter on the point-cloud route, repeated normal estimates
on one fitter, re-targets, and the stateless gingr_cloud_knn / gingr_cloud_normals leave the free device memory where it was (the
pattern of tests/test_gpu_no_leaks.py)."""
import gc

import numpy as np
import pytest

from tests.test_gpu_plane_cloud import Cloud, case
from tests.test_gpu_plane_pairs import pose_state

pytestmark = pytest.mark.gpu


def _free_bytes():
    import torch
    torch.cuda.synchronize(0)
    return torch.cuda.mem_get_info(0)[0]


def test_cloud_route_releases_its_device_memory(ctx):
    from gingr_amd._native import dptr
    mo, tv = case("grid30")
    st = pose_state(mo, "identity")
    other = np.ascontiguousarray(tv[::-1] * 1.01)

    def cycle():
        f = Cloud(ctx, mo, tv)
        try:
            f.set_state(st)
            for k in (12, 16, 33):                                     # repeated estimates: every group width
                f.estimate(k=k)
            _, sc, _ = f.update_plane(100.0, n=3)
            assert sc.status == 0
            f.ok(f.lib.gingr_fitter_set_target(f.h, other.shape[0], dptr(other)), "set_target")   # a re-target drops the normals
            f.set_normals(f_normals)
            f.plane(100.0)
            f.precisions()
        finally:
            f.close()
        ctx.cloud_knn(tv, 8)
        ctx.cloud_normals(tv, 12)

    f_normals, _ = ctx.cloud_normals(other, 12)
    cycle()                                                            # warm-up: code objects, allocator pools
    gc.collect()
    before = _free_bytes()
    for _ in range(15):
        cycle()
    gc.collect()
    after = _free_bytes()
    assert before - after < 16 << 20, f"{(before - after) / 2**20:.1f} MiB of device memory did not come back"
