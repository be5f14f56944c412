"""Host-side mirror of GiNGR's plugin surface for the MI355X update path: every name of it, importable from one place.

The reference's host language is Scala (no JVM exists in this image, see INTEGRATION.md for the Scala/JNI binding);
these modules are the Python host layer over the same C ABI.  They keep the reference's names, argument meaning and
error behaviour so that tests read like uses of the reference API:

  context        Context (gingr_ctx) and _check
  models         PointDistributionModel, the models built or adopted in HBM, DeviceModel, the GPMM helpers
  states         enums, fitting parameters, correspondence lists, the configuration / state records
  registration   GingrAlgorithm, CpdRegistration, IcpRegistration, TemplateRegistration, PointToPlaneIcpRegistration,
                 normalTangentCovariances

Dependencies run one way, context <- models <- registration; states needs none of them.  In their comments G/ stands for
src/main/scala/gingr/ of unibas-gravis/GiNGR.  All arithmetic runs in libgingr_hip.so on the GPU; nothing here computes on
the CPU and there is no fallback.
"""
from __future__ import annotations  # noqa: F401

import ctypes  # noqa: F401
import dataclasses  # noqa: F401
from ctypes import c_int64, c_void_p  # noqa: F401
from typing import Callable, List, Optional, Sequence, Tuple  # noqa: F401

import numpy as np  # noqa: F401

from . import _native as nat  # noqa: F401
from ._native import GingrNativeError, f64, dptr, iptr  # noqa: F401
from .context import Context, RigidSearchResult, RigidSearchPosesResult, _check  # noqa: F401
from .models import (  # noqa: F401
    AugmentInfo, AugmentedDevicePointDistributionModel, DeviceModel, DevicePointDistributionModel, ExtendedDevicePointDistributionModel,
    GPMMTriangleMesh3D, KernelExtensionInfo,
    GaussianKernelParameters, GpmmBuildInfo, InterpolatedDevicePointDistributionModel, LaplacianDevicePointDistributionModel,
    LaplacianHelper, LaplacianInfo, LocalizeInfo, LocalizedDevicePointDistributionModel, PcaDevicePointDistributionModel, PcaInfo, PointDistributionModel, PointSetHelper,
    PosteriorDevicePointDistributionModel, RadialKernelTerm, ScalarKernelSpec, TruncatedDevicePointDistributionModel, _cells_of, _resident,
    automaticGPMMfromTemplate, sigmoidField,
)
from .states import (  # noqa: F401
    CorrespondencePairs, CpdConfiguration, CpdRegistrationState, EulerAngles, FittingStatuses, GeneralRegistrationState,
    GlobalTranformationType, IcpConfiguration, IcpRegistrationState, LandmarkCorrespondences, ModelFittingParameters,
    PointToPlaneConfiguration, PointToPlaneRegistrationState, RobustLoss,
    TemplateConfiguration, TemplateRegistrationState, _cpd_converged, _empty_pairs, _never_converged, _with_fields,
)
from .registration import (  # noqa: F401
    CpdRegistration, GingrAlgorithm, IcpRegistration, PointToPlaneIcpRegistration, TemplateRegistration, _initial_general,
    normalTangentCovariances,
)
from .metrics import GeneralizationResult, LeaveOneOutResult, ModelMetrics, SpecificityResult  # noqa: F401
