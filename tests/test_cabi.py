"""CPU tests of the drop-in boundary: the C-ABI library loads and exports exactly what include/gingr_hip.h declares,
the ctypes prototypes cover every symbol, and the Python host layer fails loudly without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gingr_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gingr_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_expected_surface():
    names = declared_functions()
    for must in ("gingr_ctx_create", "gingr_cpd_stats", "gingr_nn", "gingr_gauss_block", "gingr_model_upload",
                 "gingr_model_posterior_mean", "gingr_fitter_update_cpd_async", "gingr_fitter_update_icp_async",
                 "gingr_fitter_cpd_phase_async", "gingr_fitter_exchange", "gingr_last_error"):
        assert must in names
    assert len(names) >= 35


def test_library_exports_every_declared_symbol():
    from gingr_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, f"declared in gingr_hip.h but not exported: {missing}"


def test_ctypes_prototypes_cover_the_header():
    from gingr_amd import _native
    assert sorted(_native.SIGNATURES) == declared_functions()
    _native.load()


def test_no_torch_or_cxx_types_in_the_boundary():
    raw = open(HEADER).read()
    assert 'extern "C"' in raw
    code = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)     # declarations only, comments stripped
    for forbidden in ("torch", "std::", "hipStream_t", "at::", "jobject", "JNIEnv", "template", "class "):
        assert forbidden not in code, forbidden


def test_fails_loudly_without_a_gpu():
    import gingr_amd as ga
    from gingr_amd import _native
    lib = _native.load()
    if lib.gingr_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(ga.GingrNativeError) as e:
        ga.Context(0)
    assert e.value.code == _native.ERR_NO_DEVICE
    h = ctypes.c_void_p()
    assert lib.gingr_ctx_create(0, ctypes.byref(h)) == _native.ERR_NO_DEVICE and not h.value


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "gingr_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="replace").read()
                assert not re.search(r"^\s*(from|import)\s+oracle|#include.*oracle|cpd_oracle|libcpd_oracle", src, flags=re.M), f


def test_header_is_self_contained_c():
    """The boundary header must compile on its own as plain C (what a cgo / JNI / FFI binding generator feeds on): catches
    C++-isms and declarations that use a type before its definition."""
    import shutil
    import subprocess
    import tempfile
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    hdr = os.path.join(ROOT, "include", "gingr_hip.h")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as f:
            f.write('#include "gingr_hip.h"\nint main(void) { return (int)sizeof(gingr_state_scalars) == 0; }\n')
        subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.dirname(hdr), src])


# ------------------------------------------------------------------------------------------------ errors of the flavours (GPU)
# One call per correspondence flavour and operation that violates exactly one precondition: the code and the message text an ABI
# client sees.  The operations: update, sampled update, transition density, posterior covariance, posterior model, and the flavour's
# phase entry point; then the entry points that take the flavour as an integer.  The pairs flavour has no parameters to get wrong.
FLAVOUR_NAMES = {0: "cpd", 1: "icp", 2: "icp_surface", 3: "pairs"}
BAD_PARAMS = {"cpd-w-1": (0, (1.0, 1.0)), "cpd-w-negative": (0, (-0.5, 1.0)), "cpd-lambda-0": (0, (0.1, 0.0)), "cpd-null": (0, None),
              "icp-0-iterations": (1, (4.0, 1.0, 0)), "icp-null": (1, None),
              "surface-0-iterations": (2, (4.0, 1.0, 0)), "surface-null": (2, None)}
PARAM_MESSAGE = {0: "cpd params: need 0 <= w < 1 and lambda > 0", 1: "icp params: max_iterations < 1", 2: "icp params: max_iterations < 1"}
NO_MESH_MESSAGE = "icp surface: no meshes set (gingr_fitter_set_meshes)"


class FlavourCalls:
    """a 64-vertex fitter with a state and no meshes, and every call that takes a flavour"""

    def __init__(self, ctx):
        import numpy as np
        from gingr_amd.sharded import ShardedFitter
        from tests.test_gpu_posterior_covariance import ga_model, model_of
        self.np, self.ctx, self.lib = np, ctx, ctx._lib
        self.mo = model_of(64, 5)
        self.sf = ShardedFitter(ctx, ga_model(self.mo), self.mo.ref + 1.0)
        self.h = self.sf.handle
        self.sf.set_state(np.zeros(self.mo.rank), 4.0)
        self.mesh = np.ascontiguousarray(self.mo.ref + 0.5)
        self.z = np.ascontiguousarray(np.linspace(-1.0, 1.0, self.mo.rank))

    def params(self, flavour, values):
        """(struct or None kept alive, [the parameter argument of the named entry points])"""
        from gingr_amd import _native as nat
        if flavour == 3:
            return None, []
        if values is None:
            return None, [None]
        p = nat.CpdParams(*values) if flavour == 0 else nat.IcpParams(*values)
        return p, [ctypes.byref(p)]

    def named(self, flavour, values):
        """name -> call of the six entry points named after the flavour"""
        from gingr_amd._native import dptr
        np, lib, h, s = self.np, self.lib, self.h, FLAVOUR_NAMES[flavour]
        keep, p = self.params(flavour, values)
        lp, pm, cov = ctypes.c_double(), ctypes.c_void_p(), np.empty((self.mo.M, 6))

        def model():
            rc = getattr(lib, f"gingr_fitter_posterior_model_{s}")(h, *p, ctypes.byref(pm))
            if rc == 0:
                lib.gingr_model_destroy(pm)
            else:
                assert not pm.value
            return rc
        return {
            "update": lambda: getattr(lib, f"gingr_fitter_update_{s}_async")(h, *p, 1),
            "update_sample": lambda: getattr(lib, f"gingr_fitter_update_{s}_sample_async")(h, *p, dptr(self.z)),
            "posterior_logpdf": lambda: getattr(lib, f"gingr_fitter_posterior_logpdf_{s}")(h, *p, dptr(self.mesh), ctypes.byref(lp)),
            "posterior_covariance": lambda: getattr(lib, f"gingr_fitter_posterior_covariance_{s}")(h, *p, dptr(cov)),
            "posterior_model": model,
            "phase": lambda: getattr(lib, f"gingr_fitter_{s}_phase_async")(h, *p, 0),
            "_keep": keep,
        }

    def by_integer(self, flavour, values):
        """name -> call of the entry points that take the flavour as an integer"""
        from gingr_amd import _native as nat
        from gingr_amd._native import dptr
        lib, h = self.lib, self.h
        cp = nat.CpdParams(*values) if flavour == 0 and values is not None else None
        ip = nat.IcpParams(*values) if flavour in (1, 2) and values is not None else None
        cpp, ipp = (ctypes.byref(cp) if cp else None), (ctypes.byref(ip) if ip else None)
        cb = nat.ALLREDUCE_FN(lambda user, seg, ptr, count: 0)
        lp = ctypes.c_double()
        req, res = nat.MhRequest(), nat.MhResult()
        req.flavour, req.kind, req.z = flavour, 0, dptr(self.z)
        req.cpd, req.icp = (ctypes.pointer(cp) if cp else None), (ctypes.pointer(ip) if ip else None)
        req.eval_sdev, req.eval_points, req.need_forward = 1.0, 0, 1
        alpha = self.np.empty(self.mo.rank)
        return {
            "update_sharded": lambda: lib.gingr_fitter_update_sharded_async(h, flavour, cpp, ipp, 1, None, cb, None),
            "posterior_logpdf_sharded": lambda: lib.gingr_fitter_posterior_logpdf_sharded(h, flavour, cpp, ipp, dptr(self.mesh), cb, None,
                                                                                          ctypes.byref(lp)),
            "mh_step": lambda: lib.gingr_fitter_mh_step(h, ctypes.byref(req), dptr(alpha), None, ctypes.byref(res)),
            "_keep": (cp, ip, cb, req, res),
        }

    def message(self):
        return (self.lib.gingr_last_error(self.ctx.handle) or b"").decode()

    def close(self):
        self.sf.close()


@pytest.fixture()
def flavour_calls(ctx):
    c = FlavourCalls(ctx)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(BAD_PARAMS))
def test_bad_parameters_are_refused_by_every_operation_of_the_flavour(flavour_calls, case):
    from gingr_amd import _native as nat
    flavour, values = BAD_PARAMS[case]
    calls = {**flavour_calls.named(flavour, values), **flavour_calls.by_integer(flavour, values)}
    for name, call in calls.items():
        if name == "_keep":
            continue
        rc = call()
        want = "mh_step: bad request" if name == "mh_step" and values is None else PARAM_MESSAGE[flavour]
        assert rc == nat.ERR_BAD_ARGUMENT and want in flavour_calls.message(), (name, rc, flavour_calls.message())


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", [0, 1, 2, 3])
def test_only_the_surface_flavour_asks_for_meshes(flavour_calls, flavour):
    from gingr_amd import _native as nat
    values = {0: (0.1, 1.0), 1: (4.0, 1.0, 10), 2: (4.0, 1.0, 10), 3: None}[flavour]
    calls = {**flavour_calls.named(flavour, values), **flavour_calls.by_integer(flavour, values)}
    for name, call in calls.items():
        if name == "_keep":
            continue
        flavour_calls.sf.set_state(flavour_calls.np.zeros(flavour_calls.mo.rank), 4.0)
        rc = call()
        if name == "mh_step":      # the likelihood of a step is measured on the surfaces, whatever the flavour; no step for pairs
            want = "mh_step: bad request" if flavour == 3 else "mh_step: no meshes set (gingr_fitter_set_meshes)"
            assert rc == (nat.ERR_BAD_ARGUMENT if flavour == 3 else nat.ERR_STATE) and want in flavour_calls.message(), (name, rc)
        elif flavour == 2:
            assert rc == nat.ERR_STATE and NO_MESH_MESSAGE in flavour_calls.message(), (name, rc, flavour_calls.message())
        else:
            assert rc == nat.GINGR_OK, (name, rc, flavour_calls.message())


@pytest.mark.gpu
def test_flavours_outside_an_entry_points_range_are_refused(flavour_calls):
    from gingr_amd import _native as nat
    from gingr_amd.group import DeviceGroup
    c = flavour_calls
    for flavour in (-1, 4):
        calls = c.by_integer(flavour, None)
        assert calls["update_sharded"]() == nat.ERR_BAD_ARGUMENT and "sharded update: bad arguments" in c.message()
        assert calls["posterior_logpdf_sharded"]() == nat.ERR_BAD_ARGUMENT and "sharded posterior_logpdf: bad arguments" in c.message()
        assert calls["mh_step"]() == nat.ERR_BAD_ARGUMENT and "mh_step: bad request" in c.message()
    g = DeviceGroup([0])
    try:
        g.upload_model(c.mo.ref, c.mo.mean, c.mo.U, c.mo.lam)
        g.set_target(c.mo.ref + 1.0)
        g.set_state(c.np.zeros(c.mo.rank), 4.0)
        lp = ctypes.c_double()
        from gingr_amd._native import dptr
        for flavour in (-1, 3):
            assert c.lib.gingr_group_update_async(g.handle, flavour, None, None, 1, None) == nat.ERR_BAD_ARGUMENT
            assert c.lib.gingr_group_posterior_logpdf(g.handle, flavour, None, None, dptr(c.mesh), ctypes.byref(lp)) == nat.ERR_BAD_ARGUMENT
        ip = nat.IcpParams(4.0, 1.0, 10)
        assert c.lib.gingr_group_update_async(g.handle, 2, None, ctypes.byref(ip), 1, None) == nat.ERR_STATE
        assert "group update: no meshes set (gingr_group_set_meshes)" in (c.lib.gingr_group_last_error(g.handle) or b"").decode()
        bad = nat.IcpParams(4.0, 1.0, 0)      # the one-device group hands the call to its fitter
        assert c.lib.gingr_group_update_async(g.handle, 1, None, ctypes.byref(bad), 1, None) == nat.ERR_BAD_ARGUMENT
        assert "icp params: max_iterations < 1" in (c.lib.gingr_group_last_error(g.handle) or b"").decode()
    finally:
        g.close()
