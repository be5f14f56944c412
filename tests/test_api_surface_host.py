"""CPU test of the package's import surface: gingr_amd.api is a façade over context / models / states / registration, and every
name that could be imported from it (and from gingr_amd) before the split still can be.  The lists were recorded from
vars(gingr_amd.api) and vars(gingr_amd) of the commit before the split (names not starting with "__"); the one name left out is
_run_resident_impl, the module-level function that used to be attached to GingrAlgorithm and is now a method in its class body."""
import dataclasses
import importlib

import pytest

API = ['AugmentInfo', 'AugmentedDevicePointDistributionModel', 'Callable', 'Context', 'CorrespondencePairs', 'CpdConfiguration',
       'CpdRegistration', 'CpdRegistrationState', 'DeviceModel', 'DevicePointDistributionModel', 'EulerAngles', 'FittingStatuses',
       'GPMMTriangleMesh3D', 'GaussianKernelParameters', 'GeneralRegistrationState', 'GingrAlgorithm', 'GingrNativeError',
       'GlobalTranformationType', 'GpmmBuildInfo', 'IcpConfiguration', 'IcpRegistration', 'IcpRegistrationState',
       'InterpolatedDevicePointDistributionModel', 'LandmarkCorrespondences', 'LaplacianDevicePointDistributionModel', 'LaplacianHelper',
       'LaplacianInfo', 'List', 'ModelFittingParameters', 'Optional', 'PcaDevicePointDistributionModel', 'PcaInfo',
       'PointDistributionModel', 'PointSetHelper', 'PosteriorDevicePointDistributionModel', 'ScalarKernelSpec', 'Sequence',
       'TemplateConfiguration', 'TemplateRegistration', 'TemplateRegistrationState', 'TruncatedDevicePointDistributionModel', 'Tuple',
       '_cells_of', '_check', '_cpd_converged', '_empty_pairs', '_initial_general', '_never_converged', '_resident', '_with_fields',
       'annotations', 'automaticGPMMfromTemplate', 'c_int64', 'c_void_p', 'ctypes', 'dataclasses', 'dptr', 'f64', 'iptr', 'nat', 'np']

PACKAGE = ['AugmentInfo', 'AugmentedDevicePointDistributionModel', 'Context', 'CorrespondencePairs', 'CpdConfiguration',
           'CpdRegistration', 'CpdRegistrationState', 'DeviceGroup', 'DeviceModel', 'DevicePointDistributionModel', 'EulerAngles',
           'FittingStatuses', 'GPMMTriangleMesh3D', 'GaussianKernelParameters', 'GeneralRegistrationState', 'GingrAlgorithm',
           'GingrInterface', 'GingrNativeError', 'GlobalTranformationType', 'GpmmBuildInfo', 'IcpConfiguration', 'IcpRegistration',
           'IcpRegistrationState', 'IndependentPointDistanceEvaluator', 'IndependentPoints', 'LandmarkCorrespondences',
           'LaplacianDevicePointDistributionModel', 'LaplacianInfo', 'ModelEvaluator', 'ModelFittingParameters',
           'PcaDevicePointDistributionModel', 'PcaInfo', 'PointDistributionModel', 'PointSetHelper',
           'PosteriorDevicePointDistributionModel', 'ProbabilisticSettings', 'RegistrationComparison', 'SimpleRegistrator',
           'TemplateConfiguration', 'TemplateRegistration', 'TemplateRegistrationState', 'TranslationAfterRotation', 'TriangleMesh3D',
           'TruncatedDevicePointDistributionModel', '_native', 'api', 'automaticGPMMfromTemplate', 'classic', 'group', 'helper', 'io',
           'sampling', 'simple']

MODEL_KINDS = ['InterpolatedDevicePointDistributionModel', 'TruncatedDevicePointDistributionModel',
               'PosteriorDevicePointDistributionModel', 'PcaDevicePointDistributionModel', 'LaplacianDevicePointDistributionModel',
               'AugmentedDevicePointDistributionModel']

FIELDS = {
    'AugmentInfo': ['columns', 'rank', 'total_variance', 'kept_variance'],
    'CorrespondencePairs': ['pids', 'points'],
    'CpdConfiguration': ['maxIterations', 'threshold', 'converged', 'useLandmarkCorrespondence', 'initialSigma', 'w', 'lambda_'],
    'CpdRegistrationState': ['general', 'config'],
    'EulerAngles': ['phi', 'theta', 'psi'],
    'GaussianKernelParameters': ['sigma', 'scaling'],
    'GeneralRegistrationState': ['model', 'modelParameters', 'target', 'fit', 'sigma2', 'globalTransformation', 'stepLength',
                                 'generatedBy', 'iteration', 'status', 'landmarkCorrespondences', 'targetCells'],
    'GpmmBuildInfo': ['columns', 'rank', 'tolerance_reached', 'residual_fraction', 'kept_variance_fraction'],
    'IcpConfiguration': ['maxIterations', 'threshold', 'converged', 'useLandmarkCorrespondence', 'initialSigma', 'endSigma',
                         'reverseCorrespondenceDirection', 'correspondenceMethod'],
    'IcpRegistrationState': ['general', 'config'],
    'LandmarkCorrespondences': ['pids', 'points', 'covs'],
    'LaplacianInfo': ['n_components', 'n_dropped', 'block_columns', 'outer_iterations', 'total_degree', 'converged', 'max_residual',
                      'cut_gap'],
    'ModelFittingParameters': ['scale', 'translation', 'rotation', 'center', 'shape'],
    'PcaInfo': ['rank', 'gpa_sweeps', 'gpa_last_change', 'total_variance', 'kept_variance'],
    'PointDistributionModel': ['reference', 'mean', 'basis', 'variance', 'cells'],
    'ScalarKernelSpec': ['kind', 'sigmas', 'scalings', 'mirror', 'scaling', 'lookup'],
    'TemplateConfiguration': ['maxIterations', 'threshold', 'converged', 'useLandmarkCorrespondence'],
    'TemplateRegistrationState': ['general', 'config'],
}


@pytest.mark.parametrize("module, names", [("gingr_amd.api", API), ("gingr_amd", PACKAGE)])
def test_every_recorded_name_is_still_importable_from_the_same_place(module, names):
    mod = importlib.import_module(module)
    missing = [n for n in names if not hasattr(mod, n)]
    assert not missing, f"{module} lost {missing}"
    scope = {}
    exec(f"from {module} import " + ", ".join(names), scope)       # the import statement itself, as the callers write it
    assert all(scope[n] is getattr(mod, n) for n in names)


def test_the_package_and_the_facade_hand_out_the_same_objects():
    import gingr_amd
    import gingr_amd.api as api
    shared = [n for n in PACKAGE if n in API]
    assert len(shared) > 30 and all(getattr(gingr_amd, n) is getattr(api, n) for n in shared)


def test_the_seven_model_classes_are_device_point_distribution_models():
    import gingr_amd.api as api
    base = api.DevicePointDistributionModel
    kinds = [getattr(api, name) for name in MODEL_KINDS]
    assert len(set(kinds + [base])) == 7
    for cls in kinds:
        assert issubclass(cls, base), cls.__name__
    # the host dataclass and the handle wrapper are no such models, as before
    assert not issubclass(api.PointDistributionModel, base) and not issubclass(api.DeviceModel, base)


def test_run_resident_is_defined_in_the_class_body():
    import gingr_amd.api as api
    import gingr_amd.registration as registration
    assert '_run_resident' in api.GingrAlgorithm.__dict__
    assert api.GingrAlgorithm.__dict__['_run_resident'].__qualname__ == 'GingrAlgorithm._run_resident'
    assert not hasattr(api, '_run_resident_impl') and not hasattr(registration, '_run_resident_impl')
    assert '_run_resident' in api.TemplateRegistration.__dict__          # Template keeps its own
    for cls in (api.CpdRegistration, api.IcpRegistration):
        assert '_run_resident' not in cls.__dict__ and cls._run_resident is api.GingrAlgorithm._run_resident


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_records_keep_their_fields_in_order(name):
    import gingr_amd.api as api
    assert [f.name for f in dataclasses.fields(getattr(api, name))] == FIELDS[name]


def test_the_modules_depend_on_each_other_one_way():
    """context <- models <- registration; states imports none of them at run time"""
    import gingr_amd.context as context
    import gingr_amd.models as models
    import gingr_amd.states as states
    for mod, forbidden in ((context, ("models", "states", "registration")), (models, ("states", "registration")),
                           (states, ("context", "models", "registration"))):
        src = open(mod.__file__).read().replace("if TYPE_CHECKING:\n    from .models import PointDistributionModel\n", "")
        for other in forbidden:
            assert f"from .{other} import" not in src and f"from . import {other}" not in src, (mod.__name__, other)
