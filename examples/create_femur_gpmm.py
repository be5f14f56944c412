#!/usr/bin/env python3
"""The reference's CreateArmadilloGPMM demo (examples/CreateArmadilloGPMM.scala) on the femur reference (needs an MI355X):

    PYTHONPATH=. python examples/create_femur_gpmm.py

A template model built to the relative tolerance 0.01 -- the pivoted Cholesky runs until the tolerance is met (1 358 factor
columns here, far past the 512 a model holds) -- and truncated to its 100 leading basis functions, `model.truncate(100)`.
The truncation is folded into the build: only the kept columns of the basis are ever formed.
"""
import os
import time

import numpy as np
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
import torch  # noqa: F401  (first: one HIP runtime per process)

import gingr_amd as ga

HERE = os.path.dirname(os.path.abspath(__file__))
ref = np.load(os.path.join(HERE, "..", "tests", "golden", "inputs.npz"))["femur"].astype(np.float64)

ctx = ga.Context(0)
t0 = time.perf_counter()
model = ga.automaticGPMMfromTemplate(ctx, ref, 0.01, toTolerance=True).truncate(100)
info = model.buildInfo
print(f"GPMM: {info.columns} factor columns (tolerance reached: {info.tolerance_reached}, residual {info.residual_fraction:.4f}), "
      f"truncated to rank {model.rank} = {100 * info.kept_variance_fraction:.1f} % of the variance, built in {time.perf_counter() - t0:.3f} s")
print(info)

# without truncate() the model would have 1 358 basis functions: an error that says so, never a shorter model
try:
    ga.automaticGPMMfromTemplate(ctx, ref, 0.01, toTolerance=True).device()
except ga.GingrNativeError as e:
    print("untruncated:", e)

# a resident model is truncated in HBM
smaller = model.truncate(40)
print(f"truncate(40) of the resident model: rank {smaller.rank}, leading variance {smaller.variance[0]:.3f} == {model.variance[0]:.3f}")
