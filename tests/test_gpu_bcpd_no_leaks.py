"""Device memory comes back: repeated create / iterate / destroy cycles of the Bayesian CPD handle (gingr_bcpd_*) leave the free
device memory where it was -- the pattern of test_gpu_no_leaks.py."""
import gc

import numpy as np
import pytest

from tests import bcpd_restatement as br

pytestmark = pytest.mark.gpu


def _free_bytes():
    import torch
    torch.cuda.synchronize(0)
    return torch.cuda.mem_get_info(0)[0]


def test_bcpd_handles_release_their_device_memory(ctx):
    from gingr_amd import classic as cl
    y, x = br.grid_case(9)                    # M = 729: 12 panels, 2 x 768 x 768 doubles of system and as much again of G and vectors

    def cycle():
        reg = cl.BCPD(ctx, y, x, w=0.1, lambda_=10.0, gamma=0.3, k=1.0, beta=1.5)
        reg.Iteration()
        assert np.isfinite(reg.sigma2())
        reg.close()
        assert cl.BCPDRegistration(ctx, y, w=0.1, lambda_=10.0, gamma=0.3, beta=1.5, max_iterations=2).register(x).shape == (729, 3)

    cycle()                                   # warm-up: code objects, allocator pools
    gc.collect()
    before = _free_bytes()
    for _ in range(15):
        cycle()
    gc.collect()
    after = _free_bytes()
    assert before - after < 64 << 20, f"{(before - after) / 2**20:.1f} MiB of device memory did not come back"
