"""ctypes binding of libgingr_hip.so (the C ABI declared in include/gingr_hip.h).

There is NO CPU fallback: if the shared library is missing or a call fails, an exception is raised.
The library is built in-tree by ``__graft_entry__.build()`` (``make -C gingr_amd/csrc``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GINGR_HIP_LIB: A/B timing of two builds on one box (development aid); default = the in-tree library
LIB_PATH = os.environ.get("GINGR_HIP_LIB") or os.path.join(_HERE, "libgingr_hip.so")

GINGR_OK = 0
ERR_BAD_ARGUMENT, ERR_HIP, ERR_NONFINITE, ERR_NOT_SPD, ERR_NO_DEVICE, ERR_STATE, ERR_NOT_CONVERGED = 1, 2, 3, 4, 5, 6, 7
NUM_PHASES = 3
NUM_SEGMENTS = 2
SEGMENT_FULLFIT = 2   # the gather of a sharded surface update (gingr_hip.h)
SEGMENT_REVSUM = 3    # per-template-vertex sums of the sharded reversed correspondence direction
FLAVOUR_CPD, FLAVOUR_ICP, FLAVOUR_ICP_SURFACE, FLAVOUR_PAIRS = 0, 1, 2, 3   # enum Flavour of gingr_amd/csrc/correspondence.h
# flavour -> the entry points named after it, indexed by OP_*; each takes (fitter, [the flavour's parameter struct,] the operation's own)
OP_UPDATE, OP_UPDATE_SAMPLE, OP_LOGPDF, OP_POSTERIOR_COVARIANCE, OP_POSTERIOR_MODEL = range(5)
FITTER_OPS = {
    flavour: tuple("gingr_fitter_" + op.format(name) for op in
                   ("update_{}_async", "update_{}_sample_async", "posterior_logpdf_{}", "posterior_covariance_{}", "posterior_model_{}"))
    for flavour, name in ((FLAVOUR_CPD, "cpd"), (FLAVOUR_ICP, "icp"), (FLAVOUR_ICP_SURFACE, "icp_surface"), (FLAVOUR_PAIRS, "pairs"))
}
RCCL_UNIQUE_ID_BYTES = 128

_STATUS_NAMES = {
    1: "GINGR_ERR_BAD_ARGUMENT", 2: "GINGR_ERR_HIP", 3: "GINGR_ERR_NONFINITE", 4: "GINGR_ERR_NOT_SPD",
    5: "GINGR_ERR_NO_DEVICE", 6: "GINGR_ERR_STATE", 7: "GINGR_ERR_NOT_CONVERGED",
}


class GingrNativeError(RuntimeError):
    def __init__(self, code: int, where: str, text: str = ""):
        self.code = code
        super().__init__(f"{where}: {_STATUS_NAMES.get(code, code)} {text}".strip())


class StateScalars(ctypes.Structure):
    """gingr_state_scalars"""
    _fields_ = [
        ("euler", c_double * 3), ("center", c_double * 3), ("translation", c_double * 3),
        ("scale", c_double), ("sigma2", c_double), ("iteration", c_int32), ("status", c_int32),
    ]


class CpdParams(ctypes.Structure):
    _fields_ = [("w", c_double), ("lambda_", c_double)]


class IcpParams(ctypes.Structure):
    _fields_ = [("initial_sigma", c_double), ("end_sigma", c_double), ("max_iterations", c_int32)]


class PlaneParams(ctypes.Structure):
    """gingr_plane_params"""
    _fields_ = [("tangent_over_normal", c_double), ("reject", c_int32)]


class PlaneCloudParams(ctypes.Structure):
    """gingr_plane_cloud_params"""
    _fields_ = [("tangent_over_normal", c_double), ("max_distance", c_double)]


class RobustParams(ctypes.Structure):
    """gingr_robust_params"""
    _fields_ = [("loss", c_int32), ("scale_mode", c_int32), ("scale", c_double), ("min_scale", c_double)]


class CloudKnnInfo(ctypes.Structure):
    """gingr_cloud_knn_info"""
    _fields_ = [("cell_size", c_double), ("grid", c_int32 * 3), ("flagged", c_int32)]


class MhRequest(ctypes.Structure):
    """gingr_mh_request"""
    _fields_ = [
        ("flavour", c_int32), ("kind", c_int32), ("cpd", POINTER(CpdParams)), ("icp", POINTER(IcpParams)),
        ("z", POINTER(c_double)), ("alpha", POINTER(c_double)), ("scalars", POINTER(StateScalars)),
        ("eval_sdev", c_double), ("eval_points", c_int64), ("need_forward", c_int32),
    ]


class MhResult(ctypes.Structure):
    """gingr_mh_result"""
    _fields_ = [
        ("scalars", StateScalars), ("log_value", c_double), ("dist_sum", c_double), ("dist_max", c_double), ("count", c_int64),
        ("log_q_forward", c_double), ("log_q_backward", c_double), ("forward_status", c_int32), ("backward_status", c_int32),
    ]


# int (*gingr_allreduce_fn)(void *user, int32_t segment, void *device_ptr, int64_t count)
ALLREDUCE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_int32, c_void_p, c_int64)
_dp = POINTER(c_double)
_ip = POINTER(c_int32)

KERNEL_GAUSSIAN_MIXTURE, KERNEL_DOT, KERNEL_LOOKUP = 0, 1, 2
OPT_CULL, OPT_FINE_CULL, OPT_NN_GRID, OPT_TRI_GRID, OPT_SPLIT_EXCHANGE, OPT_GRAM_DOWNDATE, OPT_DECIMATE_BATCH = 0, 1, 2, 3, 4, 5, 6  # gingr_ctx_option
OPT_SEPARABLE = 7


class ScalarKernel(ctypes.Structure):
    """gingr_scalar_kernel"""
    _fields_ = [("kind", c_int32), ("n_kernels", c_int32), ("sigmas", _dp), ("scalings", _dp), ("mirror", c_double),
                ("scaling", c_double), ("lookup", _dp)]


GPMM_MAX_COLUMNS = 1536
RADIAL_GAUSSIAN, RADIAL_RATIONAL_QUADRATIC, RADIAL_INVERSE_MULTIQUADRIC = 0, 1, 2


class RadialTerm(ctypes.Structure):
    """gingr_radial_term"""
    _fields_ = [("family", c_int32), ("parameter", c_double), ("scaling", c_double), ("weight", _dp)]


class RadialKernel(ctypes.Structure):
    """gingr_radial_kernel"""
    _fields_ = [("n_terms", c_int32), ("terms", POINTER(RadialTerm))]


class GpmmInfo(ctypes.Structure):
    """gingr_gpmm_info"""
    _fields_ = [("columns", c_int32), ("rank", c_int32), ("tolerance_reached", c_int32), ("residual_fraction", c_double),
                ("kept_variance_fraction", c_double)]


CLASSIC_CPD_MAX_COLUMNS = 512


class ClassicCpdLowRankInfo(ctypes.Structure):
    """gingr_classic_cpd_lowrank_info"""
    _fields_ = [("columns", c_int32), ("tolerance_reached", c_int32), ("residual_fraction", c_double), ("factor_bytes", c_int64)]


class PcaInfo(ctypes.Structure):
    """gingr_pca_info"""
    _fields_ = [("rank", c_int32), ("gpa_sweeps", c_int32), ("gpa_last_change", c_double), ("total_variance", c_double),
                ("kept_variance", c_double)]


class AugmentInfo(ctypes.Structure):
    """gingr_augment_info"""
    _fields_ = [("columns", c_int32), ("rank", c_int32), ("total_variance", c_double), ("kept_variance", c_double)]


class LocalizeInfo(ctypes.Structure):
    """gingr_localize_info"""
    _fields_ = [("columns", c_int32), ("rank", c_int32), ("tolerance_reached", c_int32), ("residual_fraction", c_double),
                ("total_variance", c_double), ("kept_variance", c_double)]


class LaplacianInfo(ctypes.Structure):
    """gingr_laplacian_info"""
    _fields_ = [("n_components", c_int32), ("n_dropped", c_int32), ("block_columns", c_int32), ("outer_iterations", c_int32),
                ("total_degree", c_int32), ("converged", c_int32), ("max_residual", c_double), ("cut_gap", c_double)]


class NicpInfo(ctypes.Structure):
    """gingr_nicp_info"""
    _fields_ = [("iterations", c_int32), ("converged", c_int32), ("residual", c_double * 3), ("rhs_norm", c_double * 3)]


# name -> (restype, argtypes); every symbol include/gingr_hip.h declares
SIGNATURES = {
    "gingr_device_count": (c_int, []),
    "gingr_ctx_create": (c_int, [c_int, POINTER(c_void_p)]),
    "gingr_ctx_destroy": (None, [c_void_p]),
    "gingr_last_error": (c_char_p, [c_void_p]),
    "gingr_ctx_set_stream": (c_int, [c_void_p, c_void_p]),
    "gingr_ctx_get_stream": (c_void_p, [c_void_p]),
    "gingr_ctx_synchronize": (c_int, [c_void_p]),
    "gingr_build_info": (c_char_p, []),
    "gingr_ctx_set_option": (c_int, [c_void_p, c_int32, c_int32]),
    "gingr_ctx_get_option": (c_int, [c_void_p, c_int32, POINTER(c_int32)]),
    "gingr_cpd_stats": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_double, c_double, _dp, _dp, _dp, _dp, _dp]),
    "gingr_cpd_initial_sigma2": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, _dp]),
    "gingr_nn": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, _ip, _dp, _dp]),
    "gingr_gauss_block": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_double, c_double, _dp]),
    "gingr_model_upload": (c_int, [c_void_p, c_int64, c_int32, _dp, _dp, _dp, _dp, c_int64, c_int64, POINTER(c_void_p)]),
    "gingr_model_destroy": (None, [c_void_p]),
    "gingr_model_gram_exchange": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64)]),
    "gingr_model_finalize": (c_int, [c_void_p, c_void_p]),
    "gingr_fitter_set_meshes": (c_int, [c_void_p, c_int64, POINTER(c_int32), c_int64, POINTER(c_int32)]),
    "gingr_fitter_set_surface_method": (c_int, [c_void_p, c_int32]),
    "gingr_fitter_set_correspondence_direction": (c_int, [c_void_p, c_int32]),
    "gingr_fitter_get_reversed_correspondence": (c_int, [c_void_p, POINTER(c_int32), _dp]),
    "gingr_fitter_update_icp_surface_async": (c_int, [c_void_p, POINTER(IcpParams), c_int32]),
    "gingr_fitter_set_stop_threshold": (c_int, [c_void_p, c_double]),
    "gingr_fitter_stop_rule_hit": (c_int, [c_void_p, POINTER(c_int32)]),
    "gingr_fitter_icp_surface_phase_async": (c_int, [c_void_p, POINTER(IcpParams), c_int32]),
    "gingr_fitter_get_surface_correspondence": (c_int, [c_void_p, _dp, _dp]),
    "gingr_fitter_surface_distance_stats": (c_int, [c_void_p, c_int32, c_int64, _dp, c_int32, c_double, _dp]),
    "gingr_fitter_mh_step": (c_int, [c_void_p, POINTER(MhRequest), _dp, _dp, POINTER(MhResult)]),
    "gingr_fitter_mh_restore": (c_int, [c_void_p]),
    "gingr_classic_cpd_create": (c_int, [c_void_p, c_int32, c_int64, _dp, c_int64, _dp, c_double, c_double, c_double, POINTER(c_void_p)]),
    "gingr_classic_cpd_destroy": (None, [c_void_p]),
    "gingr_classic_cpd_iterate": (c_int, [c_void_p, c_int32]),
    "gingr_classic_cpd_get": (c_int, [c_void_p, _dp, POINTER(c_double), _dp, _dp]),
    "gingr_classic_cpd_set": (c_int, [c_void_p, _dp, c_double]),
    "gingr_classic_cpd_create_lowrank": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_double, c_double, c_double, c_double, c_int32,
                                                 POINTER(ClassicCpdLowRankInfo), POINTER(c_void_p)]),
    "gingr_classic_cpd_get_factor": (c_int, [c_void_p, _ip, _dp]),
    "gingr_bcpd_create": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_double, c_double, c_double, c_double, c_double, POINTER(c_void_p)]),
    "gingr_bcpd_destroy": (None, [c_void_p]),
    "gingr_bcpd_iterate": (c_int, [c_void_p, c_int32]),
    "gingr_bcpd_get": (c_int, [c_void_p, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gingr_bcpd_set": (c_int, [c_void_p, _dp, _dp, _dp, _dp, c_double]),
    "gingr_bcpd_create_lowrank": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_double, c_double, c_double, c_double, c_double, c_double,
                                          c_int32, POINTER(ClassicCpdLowRankInfo), POINTER(c_void_p)]),
    "gingr_bcpd_get_factor": (c_int, [c_void_p, _ip, _dp]),
    "gingr_classic_cpd_transform_points": (c_int, [c_void_p, c_int64, _dp, _dp]),
    "gingr_bcpd_transform_points": (c_int, [c_void_p, c_int64, _dp, _dp]),
    "gingr_bcpd_get_coefficients": (c_int, [c_void_p, _dp]),
    "gingr_mesh_distance_stats": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_int64, POINTER(c_int32), c_int32, c_double, _dp]),
    "gingr_fitter_update_icp_surface_sample_async": (c_int, [c_void_p, POINTER(IcpParams), _dp]),
    "gingr_fitter_posterior_logpdf_icp_surface": (c_int, [c_void_p, POINTER(IcpParams), _dp, POINTER(c_double)]),
    "gingr_rigid_icp_create": (c_int, [c_void_p, c_int32, c_int64, _dp, c_int64, _dp, POINTER(c_void_p)]),
    "gingr_rigid_icp_destroy": (None, [c_void_p]),
    "gingr_rigid_icp_iterate": (c_int, [c_void_p, c_int32, _dp]),
    "gingr_rigid_icp_get": (c_int, [c_void_p, _dp, _dp]),
    "gingr_rigid_icp_set": (c_int, [c_void_p, _dp]),
    "gingr_fitter_set_fit_points": (c_int, [c_void_p, _dp]),
    "gingr_nicp_solve": (c_int, [c_void_p, c_int32, c_int64, _dp, c_int64, _ip, _dp, _dp, c_int32, _ip, _dp, c_double, c_double, c_double,
                                 _dp, _dp]),
    "gingr_nicp_create": (c_int, [c_void_p, c_int32, c_int64, c_int64, _ip, c_int32, _ip, POINTER(c_void_p)]),
    "gingr_nicp_destroy": (None, [c_void_p]),
    "gingr_nicp_step": (c_int, [c_void_p, _dp, _dp, _dp, _dp, c_double, c_double, c_double, c_double, c_int32, _dp, _dp, POINTER(NicpInfo)]),
    "gingr_nicp_get_solution": (c_int, [c_void_p, _dp]),
    "gingr_mesh_closest_points": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_int64, _ip, _dp, _dp, _ip, _dp]),
    "gingr_mesh_decimate": (c_int, [c_void_p, c_int64, _dp, c_int64, _ip, c_int64, POINTER(c_int64), _ip, POINTER(c_int64), _ip, _dp]),
    "gingr_model_new_reference": (c_int, [c_void_p, c_void_p, c_int64, _dp, _ip, _dp, c_int64, c_int64, POINTER(c_void_p)]),
    "gingr_gpmm_build_diagonal": (c_int, [c_void_p, c_int64, _dp, POINTER(ScalarKernel), POINTER(ScalarKernel), POINTER(ScalarKernel),
                                          c_double, c_int32, c_int64, c_int64, POINTER(c_void_p)]),
    "gingr_gpmm_build_diagonal_ex": (c_int, [c_void_p, c_int64, _dp, POINTER(ScalarKernel), POINTER(ScalarKernel), POINTER(ScalarKernel),
                                             c_double, c_int32, c_int32, c_int64, c_int64, POINTER(GpmmInfo), POINTER(c_void_p)]),
    "gingr_model_truncate": (c_int, [c_void_p, c_void_p, c_int32, POINTER(c_void_p)]),
    "gingr_model_kernel_extension": (c_int, [c_void_p, _ip, _ip, _ip]),
    "gingr_model_get_kernel_extension": (c_int, [c_void_p, c_void_p, c_int32, _ip, _dp]),
    "gingr_model_extend": (c_int, [c_void_p, c_void_p, c_int64, _dp, POINTER(c_void_p)]),
    "gingr_model_warp_points": (c_int, [c_void_p, c_void_p, _dp, _dp, _dp, _dp, c_double, c_int64, _dp, _dp]),
    "gingr_gpmm_build_radial": (c_int, [c_void_p, c_int64, _dp, POINTER(RadialKernel), POINTER(RadialKernel), POINTER(RadialKernel),
                                        c_double, c_int32, c_int32, c_int64, c_int64, POINTER(GpmmInfo), POINTER(c_void_p)]),
    "gingr_gpmm_build_gaussian": (c_int, [c_void_p, c_int64, _dp, c_int32, _dp, _dp, c_double, c_int32, c_int64, c_int64,
                                          POINTER(c_void_p)]),
    "gingr_pointset_distance_extrema": (c_int, [c_void_p, _dp, c_int64, _dp, _dp]),
    "gingr_model_download": (c_int, [c_void_p, c_void_p, _dp, _dp, _dp, _dp]),
    "gingr_model_num_points": (c_int64, [c_void_p]),
    "gingr_model_rank": (c_int32, [c_void_p]),
    "gingr_model_separable": (c_int, [c_void_p, _ip, _ip, _ip]),
    "gingr_model_instance": (c_int, [c_void_p, c_void_p, _dp, _dp, _dp, _dp, c_double, _dp]),
    "gingr_model_coefficients": (c_int, [c_void_p, c_void_p, _dp, _dp, _dp, _dp, _dp]),
    "gingr_model_posterior_mean": (c_int, [c_void_p, c_void_p, _dp, _dp, _dp, _dp, _dp, c_int32, _ip, _dp, _dp, _dp, _dp]),
    "gingr_fitter_create": (c_int, [c_void_p, c_void_p, POINTER(c_void_p)]),
    "gingr_fitter_destroy": (None, [c_void_p]),
    "gingr_fitter_set_target": (c_int, [c_void_p, c_int64, _dp]),
    "gingr_fitter_set_landmarks": (c_int, [c_void_p, c_int32, _ip, _dp, _dp]),
    "gingr_fitter_set_options": (c_int, [c_void_p, c_int32, c_double]),
    "gingr_fitter_set_state": (c_int, [c_void_p, _dp, POINTER(StateScalars)]),
    "gingr_fitter_get_state": (c_int, [c_void_p, _dp, POINTER(StateScalars), _dp]),
    "gingr_fitter_get_cpd_stats": (c_int, [c_void_p, _dp, _dp, _dp, _dp]),
    "gingr_fitter_get_icp_idx": (c_int, [c_void_p, _ip, _dp]),
    "gingr_fitter_update_cpd_async": (c_int, [c_void_p, POINTER(CpdParams), c_int32]),
    "gingr_fitter_update_icp_async": (c_int, [c_void_p, POINTER(IcpParams), c_int32]),
    "gingr_fitter_update_cpd_sample_async": (c_int, [c_void_p, POINTER(CpdParams), _dp]),
    "gingr_fitter_update_icp_sample_async": (c_int, [c_void_p, POINTER(IcpParams), _dp]),
    "gingr_fitter_posterior_logpdf_cpd": (c_int, [c_void_p, POINTER(CpdParams), _dp, _dp]),
    "gingr_fitter_posterior_logpdf_icp": (c_int, [c_void_p, POINTER(IcpParams), _dp, _dp]),
    "gingr_model_marginal_covariance": (c_int, [c_void_p, c_void_p, _dp, _dp, _dp]),
    "gingr_model_cross_covariance": (c_int, [c_void_p, c_void_p, _dp, _dp, c_int64, _dp]),
    "gingr_fitter_posterior_covariance_cpd": (c_int, [c_void_p, POINTER(CpdParams), _dp]),
    "gingr_fitter_posterior_covariance_icp": (c_int, [c_void_p, POINTER(IcpParams), _dp]),
    "gingr_fitter_posterior_covariance_icp_surface": (c_int, [c_void_p, POINTER(IcpParams), _dp]),
    "gingr_model_posterior": (c_int, [c_void_p, c_void_p, _dp, _dp, _dp, _dp, _dp, c_int32, _ip, _dp, _dp, POINTER(c_void_p)]),
    "gingr_fitter_posterior_model_cpd": (c_int, [c_void_p, POINTER(CpdParams), POINTER(c_void_p)]),
    "gingr_fitter_posterior_model_icp": (c_int, [c_void_p, POINTER(IcpParams), POINTER(c_void_p)]),
    "gingr_fitter_posterior_model_icp_surface": (c_int, [c_void_p, POINTER(IcpParams), POINTER(c_void_p)]),
    # correspondences given by the caller (flavour 3, fitter_pairs.hip)
    "gingr_fitter_set_pairs": (c_int, [c_void_p, c_int64, _ip, _dp, _dp]),
    "gingr_fitter_set_pairs_cov": (c_int, [c_void_p, c_int64, _ip, _dp, _dp]),
    "gingr_fitter_set_pairs_cov_dense": (c_int, [c_void_p, c_int64, _ip, _dp, _dp]),
    "gingr_fitter_get_pair_observations": (c_int, [c_void_p, _dp, _dp]),
    "gingr_fitter_get_pair_precisions": (c_int, [c_void_p, _dp, _dp]),
    "gingr_fitter_set_sigma2": (c_int, [c_void_p, c_double]),
    "gingr_fitter_last_update_error": (c_int, [c_void_p, POINTER(c_int32)]),
    "gingr_fitter_update_pairs_async": (c_int, [c_void_p, c_int32]),
    "gingr_fitter_pairs_phase_async": (c_int, [c_void_p, c_int32]),
    "gingr_fitter_update_pairs_sample_async": (c_int, [c_void_p, _dp]),
    "gingr_fitter_posterior_logpdf_pairs": (c_int, [c_void_p, _dp, _dp]),
    "gingr_fitter_posterior_covariance_pairs": (c_int, [c_void_p, _dp]),
    "gingr_fitter_posterior_model_pairs": (c_int, [c_void_p, POINTER(c_void_p)]),
    # point-to-plane ICP: the dense list made on the device from the surface scan
    "gingr_fitter_set_pairs_plane_async": (c_int, [c_void_p, POINTER(PlaneParams)]),
    "gingr_fitter_update_plane_async": (c_int, [c_void_p, POINTER(PlaneParams), POINTER(IcpParams), c_int32]),
    # k nearest neighbours of a cloud within itself, normals from them; point-to-plane ICP against a point cloud
    "gingr_cloud_knn": (c_int, [c_void_p, c_int64, _dp, c_int32, _ip, _dp, POINTER(CloudKnnInfo)]),
    "gingr_cloud_normals": (c_int, [c_void_p, c_int64, _dp, c_int32, _dp, _dp, _dp, POINTER(CloudKnnInfo)]),
    "gingr_fitter_set_target_normals": (c_int, [c_void_p, _dp]),
    "gingr_fitter_estimate_target_normals": (c_int, [c_void_p, c_int32, _dp, POINTER(CloudKnnInfo)]),
    "gingr_fitter_get_target_normals": (c_int, [c_void_p, _dp]),
    "gingr_fitter_set_pairs_plane_cloud_async": (c_int, [c_void_p, POINTER(PlaneCloudParams)]),
    "gingr_fitter_update_plane_cloud_async": (c_int, [c_void_p, POINTER(PlaneCloudParams), POINTER(IcpParams), c_int32]),
    # robust point-to-plane ICP: M-estimator weights with the median scale on the device; the selection as an operator
    "gingr_fitter_set_plane_robust": (c_int, [c_void_p, POINTER(RobustParams)]),
    "gingr_fitter_get_plane_robust": (c_int, [c_void_p, _dp, _dp, _dp, _dp, POINTER(c_int64)]),
    "gingr_order_statistic": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp]),
    "gingr_rotation_samples": (c_int, [c_int64, _dp]),
    "gingr_rigid_search": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_int64, _dp, c_int32, c_double, POINTER(c_int64), _dp, _dp,
                                   POINTER(c_int64), _ip]),
    "gingr_rigid_search_poses": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_int64, _dp, c_int32, c_double, c_double, c_int32,
                                         POINTER(c_int64), _dp, _dp, POINTER(c_int64), _ip, POINTER(c_int64)]),
    # feature-based global alignment: descriptors, their match, poses from triples of matches
    "gingr_cloud_fpfh": (c_int, [c_void_p, c_int64, _dp, _dp, c_int32, c_double, _ip, _ip, _dp, POINTER(CloudKnnInfo)]),
    "gingr_feature_match": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_int32, _ip, _dp]),
    "gingr_rigid_poses_from_triples": (c_int, [c_void_p, c_int64, _dp, c_int64, _dp, c_int64, _ip, _ip, _dp, _ip]),
    "gingr_model_from_shapes": (c_int, [c_void_p, c_int64, c_int32, _dp, _dp, c_int32, c_int32, c_double, c_double, c_int32,
                                        POINTER(c_void_p), POINTER(PcaInfo)]),
    "gingr_model_augment": (c_int, [c_void_p, c_void_p, c_void_p, c_double, c_int32, POINTER(c_void_p), POINTER(AugmentInfo)]),
    "gingr_model_localize": (c_int, [c_void_p, c_void_p, c_double, c_double, c_int32, POINTER(c_void_p), POINTER(LocalizeInfo)]),
    "gingr_model_instances": (c_int, [c_void_p, c_void_p, c_int64, _dp, _dp]),
    "gingr_model_generalization": (c_int, [c_void_p, c_void_p, c_int32, _dp, c_int32, _ip, _dp, _dp, _dp]),
    "gingr_model_specificity": (c_int, [c_void_p, c_void_p, c_int32, _dp, c_int64, _dp, c_int32, _ip, _dp, _ip]),
    "gingr_mesh_set_distances": (c_int, [c_void_p, c_int64, c_int64, _dp, c_int64, c_int64, _dp, c_int64, _ip, c_int32, c_int32, _dp, _dp]),
    "gingr_model_generalization_surface": (c_int, [c_void_p, c_void_p, c_int32, _dp, c_int64, _ip, c_int32, _ip, _dp, _dp, _dp]),
    "gingr_model_specificity_surface": (c_int, [c_void_p, c_void_p, c_int32, _dp, c_int64, _ip, c_int64, _dp, c_int32, _ip, _dp, _ip]),
    "gingr_pca_leave_one_out": (c_int, [c_void_p, c_int64, c_int32, _dp, c_double, c_int32, _ip, _dp, _dp, _ip]),
    "gingr_model_from_laplacian": (c_int, [c_void_p, c_int64, _dp, c_int64, _ip, c_double, c_int32, c_double, c_int32,
                                           POINTER(LaplacianInfo), POINTER(c_void_p)]),
    "gingr_fitter_retry_counter": (c_int, [c_void_p, c_int32, POINTER(c_int32)]),
    "gingr_fitter_exchange": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64), POINTER(c_int64)]),
    "gingr_fitter_cpd_phase_async": (c_int, [c_void_p, POINTER(CpdParams), c_int32]),
    "gingr_fitter_update_cpd_sharded_async": (c_int, [c_void_p, POINTER(CpdParams), c_int32, ALLREDUCE_FN, c_void_p]),
    "gingr_fitter_update_icp_sharded_async": (c_int, [c_void_p, POINTER(IcpParams), c_int32, ALLREDUCE_FN, c_void_p]),
    "gingr_fitter_icp_phase_async": (c_int, [c_void_p, POINTER(IcpParams), c_int32]),
    "gingr_fitter_update_sharded_async": (c_int, [c_void_p, c_int32, POINTER(CpdParams), POINTER(IcpParams), c_int32, _dp, ALLREDUCE_FN, c_void_p]),
    "gingr_fitter_posterior_logpdf_sharded": (c_int, [c_void_p, c_int32, POINTER(CpdParams), POINTER(IcpParams), _dp, ALLREDUCE_FN, c_void_p, _dp]),
    "gingr_fitter_fullfit_exchange": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64)]),
    "gingr_fitter_reversal_exchange": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int64)]),
    "gingr_fitter_gather_stage": (c_int, [c_void_p, c_int32, c_int32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int64)]),
    "gingr_fitter_gather_finish": (c_int, [c_void_p, c_int32]),
    "gingr_fitter_update_rccl_async": (c_int, [c_void_p, c_int32, POINTER(CpdParams), POINTER(IcpParams), c_int32, _dp]),
    "gingr_fitter_posterior_logpdf_rccl": (c_int, [c_void_p, c_int32, POINTER(CpdParams), POINTER(IcpParams), _dp, _dp]),
    "gingr_group_set_meshes": (c_int, [c_void_p, c_int64, _ip, c_int64, _ip]),
    "gingr_group_set_surface_method": (c_int, [c_void_p, c_int32]),
    "gingr_group_set_correspondence_direction": (c_int, [c_void_p, c_int32]),
    "gingr_group_update_async": (c_int, [c_void_p, c_int32, POINTER(CpdParams), POINTER(IcpParams), c_int32, _dp]),
    "gingr_group_posterior_logpdf": (c_int, [c_void_p, c_int32, POINTER(CpdParams), POINTER(IcpParams), _dp, _dp]),
    "gingr_rccl_load": (c_int, [c_void_p, c_char_p]),
    "gingr_rccl_unique_id": (c_int, [c_void_p, c_void_p]),
    "gingr_ctx_rccl_init": (c_int, [c_void_p, c_void_p, c_int32, c_int32]),
    "gingr_ctx_rccl_info": (c_int, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), c_char_p, c_int32]),
    "gingr_ctx_rccl_allreduce_async": (c_int, [c_void_p, c_void_p, c_int64]),
    "gingr_fitter_update_cpd_rccl_async": (c_int, [c_void_p, POINTER(CpdParams), c_int32]),
    "gingr_fitter_update_icp_rccl_async": (c_int, [c_void_p, POINTER(IcpParams), c_int32]),
    "gingr_group_create": (c_int, [c_int32, _ip, POINTER(c_void_p)]),
    "gingr_group_destroy": (None, [c_void_p]),
    "gingr_group_size": (c_int32, [c_void_p]),
    "gingr_group_last_error": (c_char_p, [c_void_p]),
    "gingr_group_ctx": (c_void_p, [c_void_p, c_int32]),
    "gingr_group_shard_rows": (c_int, [c_void_p, c_int32, POINTER(c_int64), POINTER(c_int64)]),
    "gingr_group_model_upload": (c_int, [c_void_p, c_int64, c_int32, _dp, _dp, _dp, _dp]),
    "gingr_group_gpmm_build_gaussian": (c_int, [c_void_p, c_int64, _dp, c_int32, _dp, _dp, c_double, c_int32]),
    "gingr_group_model_rank": (c_int32, [c_void_p]),
    "gingr_group_set_target": (c_int, [c_void_p, c_int64, _dp]),
    "gingr_group_set_landmarks": (c_int, [c_void_p, c_int32, _ip, _dp, _dp]),
    "gingr_group_set_options": (c_int, [c_void_p, c_int32, c_double]),
    "gingr_group_set_state": (c_int, [c_void_p, _dp, POINTER(StateScalars)]),
    "gingr_group_get_state": (c_int, [c_void_p, _dp, POINTER(StateScalars), _dp]),
    "gingr_group_update_cpd_async": (c_int, [c_void_p, POINTER(CpdParams), c_int32]),
    "gingr_group_update_icp_async": (c_int, [c_void_p, POINTER(IcpParams), c_int32]),
    "gingr_group_synchronize": (c_int, [c_void_p]),
    "gingr_group_exchange_info": (c_int, [c_void_p, POINTER(c_int32), POINTER(c_int32)]),
    "gingr_ctx_nn_counting": (c_int, [c_void_p, c_int32]),
    "gingr_ctx_nn_tests": (c_int, [c_void_p, POINTER(c_int64)]),
    "gingr_ctx_timing_enable": (c_int, [c_void_p, c_int32]),
    "gingr_ctx_timing_read": (c_int, [c_void_p, c_int32, _dp, POINTER(c_int64)]),
    "gingr_ctx_timing_reset": (c_int, [c_void_p]),
}

_LIB = None


def load():
    """Load libgingr_hip.so and set the prototypes.  Raises if the library has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GingrNativeError(
                ERR_STATE, "load",
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        lib = ctypes.CDLL(LIB_PATH)
        # GINGR_HIP_LIB_ALLOW_OLDER=1 (set by tools/abn.sh only: same-box A/B timing against an OLDER build of the library)
        # tolerates symbols that build does not have yet and says which; any other library -- the in-tree one, or a user's
        # GINGR_HIP_LIB override -- must export every declared symbol
        older_build = os.environ.get("GINGR_HIP_LIB_ALLOW_OLDER") == "1"
        skipped = []
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
            except AttributeError:
                if older_build:
                    skipped.append(name)
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        if skipped:
            import sys
            print(f"gingr_amd: {LIB_PATH} lacks {len(skipped)} declared symbols (older build): {', '.join(skipped)}", file=sys.stderr)
        _LIB = lib
    return _LIB


def f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def dptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def iptr(a):
    return None if a is None else a.ctypes.data_as(_ip)
