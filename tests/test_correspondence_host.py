"""CPU pin of gingr_amd/csrc/correspondence.h, the one definition of the fitter's correspondence flavour: the header compiled for the
host with the address and undefined-behaviour sanitizers into a stand-alone driver (tests/c/correspondence_driver.cpp).

Validation: every refusal rule on its own, at its edges, and a wrong or null pointer for each kind.

Derived facts: tabulated over kind x reversed x surface method x landmarks (0 / 1) and compared with the conditions the fitter spelled
out before the header existed, restated below (icp = the flavour is not CPD, pairs / surface = the two sticky flags the phase entry
points used to set; file:line on the commit before the header):
  uniform weights        icp && !f->pairs && !f->icp_surface && !f->reversed && f->n_lm == 0            fitter_phases.hip:454, :496, :596
  gated Gram downdate    icp && !f->pairs && f->icp_surface && !f->reversed                             fitter_phases.hip:460
  post-solve sigma2      a.is_icp = !icp ? 0 : f->pairs ? 2 : 1                                         fitter_phases.hip:513
  ICP's schedule         if (icp && !f->pairs) a.icp_step = ...                                         fitter_phases.hip:514
  reversed phase 0       (not pairs) icp && f->reversed                                                 fitter_phases.hip:566-568
  needs meshes           the check of gingr_fitter_icp_surface_phase_async only                         fitter_phases.hip:693
  gathered fit           flavour == 2 || (flavour == 1 && f->reversed)                                  fitter_phases.hip:753, fitter_mh.hip:215,
                                                                                                        group.hip:389, :443
  segment 0 exchanged    !(flavour != 0 && ph == 0) / flavour == 0                                      fitter_phases.hip:787, fitter_mh.hip:217,
                                                                                                        group.hip:421, :467
  reversal sums          (flavour == 1 || flavour == 2) && f->reversed                                  fitter_phases.hip:792, fitter_mh.hip:219
                         flavour != 0 && g->reversed (the group takes flavours 0..2)                    group.hip:417, :426, :465, :470
  memo key               !icp ? 0 : f->pairs ? 3 : ((f->icp_surface ? 2 : 1) + 4 * f->surface_method + 16 * (f->reversed ? 1 : 0))
                                                                                                        fitter_phases.hip:135"""
import itertools
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
NONE, BAD_FLAVOUR, CPD_PARAMS, ICP_PARAMS = 0, 1, 2, 3
CPD, CLOUD, SURFACE, PAIRS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("correspondence") / "correspondence_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "correspondence_driver.cpp"), "-o", str(exe)])
    return str(exe)


def text(x):
    return "nan" if math.isnan(x) else float(x).hex()


def validate(driver, flavour, cp=(0.1, 2.0), ip=10):
    """cp: (w, lambda) or None for a null pointer; ip: max_iterations or None -> (error, kind, w, lambda, max_iterations)"""
    w, lam = cp if cp is not None else (0.5, 1.0)
    line = f"{flavour} {int(cp is not None)} {text(w)} {text(lam)} {int(ip is not None)} {ip if ip is not None else 5}\n"
    out = subprocess.run([driver, "validate"], input=line.encode(), capture_output=True, check=True).stdout.split()
    return int(out[0]), int(out[1]), float.fromhex(out[2].decode()), float.fromhex(out[3].decode()), int(out[4])


def test_the_enum_values_are_the_abi_integers(driver):
    assert subprocess.run([driver, "enum"], capture_output=True, check=True).stdout.split() == [b"0", b"1", b"2", b"3"]


@pytest.mark.parametrize("flavour, want", [(-1, BAD_FLAVOUR), (0, NONE), (1, NONE), (2, NONE), (3, NONE), (4, BAD_FLAVOUR)])
def test_the_range_of_the_flavour(driver, flavour, want):
    assert validate(driver, flavour)[:2] == (want, flavour)


@pytest.mark.parametrize("w, want", [(-0.0, NONE), (0.0, NONE), (math.nextafter(1.0, 0.0), NONE), (1.0, CPD_PARAMS), (math.nan, CPD_PARAMS),
                                     (-math.ulp(0.0), CPD_PARAMS)])
def test_the_mixing_weight_at_its_edges(driver, w, want):
    err, kind, got_w, lam, _ = validate(driver, CPD, cp=(w, 2.0))
    assert (err, kind, lam) == (want, CPD, 2.0) and (math.isnan(got_w) if math.isnan(w) else got_w == w)
    assert math.copysign(1.0, got_w) == math.copysign(1.0, w) or math.isnan(w)


@pytest.mark.parametrize("lam, want", [(0.0, CPD_PARAMS), (math.ulp(0.0), NONE), (math.nan, CPD_PARAMS), (-1.0, CPD_PARAMS), (2.0, NONE)])
def test_lambda_at_its_edges(driver, lam, want):
    assert validate(driver, CPD, cp=(0.1, lam))[0] == want


@pytest.mark.parametrize("flavour", [CLOUD, SURFACE])
@pytest.mark.parametrize("iterations, want", [(0, ICP_PARAMS), (1, NONE), (-3, ICP_PARAMS)])
def test_the_iteration_count_at_its_edges(driver, flavour, iterations, want):
    assert validate(driver, flavour, ip=iterations)[0] == want


def test_only_the_pointer_of_the_kind_is_looked_at(driver):
    bad_cp, bad_ip = (1.5, -1.0), 0
    assert validate(driver, CPD, cp=None)[0] == CPD_PARAMS and validate(driver, CPD, ip=None)[0] == NONE
    assert validate(driver, CPD, ip=bad_ip)[0] == NONE
    for flavour in (CLOUD, SURFACE):
        assert validate(driver, flavour, ip=None)[0] == ICP_PARAMS and validate(driver, flavour, cp=None)[0] == NONE
        assert validate(driver, flavour, cp=bad_cp)[0] == NONE
    assert validate(driver, PAIRS, cp=None, ip=None)[0] == NONE and validate(driver, PAIRS, cp=bad_cp, ip=bad_ip)[0] == NONE
    # parameters the kind does not use are zero in the descriptor
    assert validate(driver, CLOUD)[2:4] == (0.0, 0.0) and validate(driver, CPD)[4] == 0 and validate(driver, PAIRS)[2:] == (0.0, 0.0, 0)
    assert validate(driver, CPD)[2:4] == (0.1, 2.0) and validate(driver, SURFACE)[4] == 10


def former_conditions(kind, reversed_, method, n_lm):
    """the expressions quoted in the module docstring, on the flags the entry points used to set"""
    icp, pairs, surface = kind != CPD, kind == PAIRS, kind == SURFACE
    return {
        "is_icp_schedule": icp and not pairs,
        "post_solve_sigma2_rule": 0 if not icp else 2 if pairs else 1,
        "needs_meshes": kind == SURFACE,
        "needs_gathered_fit": kind == 2 or (kind == 1 and reversed_),
        "exchanges_segment0": kind == 0,
        "exchanges_reversal_sums": kind in (1, 2) and reversed_,
        "uniform_weights": icp and not pairs and not surface and not reversed_ and n_lm == 0,
        "zero_one_weights": icp and not pairs and surface and not reversed_,
        "reversed_icp": icp and not pairs and reversed_,
        "memo_flavour_key": 0 if not icp else 3 if pairs else (2 if surface else 1) + 4 * method + 16 * (1 if reversed_ else 0),
    }


def facts(driver):
    names = ["is_icp_schedule", "post_solve_sigma2_rule", "needs_meshes", "needs_gathered_fit", "exchanges_segment0",
             "exchanges_reversal_sums", "uniform_weights", "zero_one_weights", "reversed_icp", "memo_flavour_key"]
    table = {}
    for line in subprocess.run([driver, "facts"], capture_output=True, check=True).stdout.decode().splitlines():
        key, values = line.split(":")
        table[tuple(int(v) for v in key.split())] = dict(zip(names, (int(v) for v in values.split())))
    return table


def test_every_derived_fact_over_the_full_grid(driver):
    table = facts(driver)
    grid = list(itertools.product(range(4), (0, 1), (0, 1), (0, 1)))
    assert sorted(table) == grid
    for kind, reversed_, method, n_lm in grid:
        want = {k: int(v) for k, v in former_conditions(kind, bool(reversed_), method, n_lm).items()}
        if kind in (CPD, PAIRS):     # the former key ignores method and direction there: so must the new one
            assert table[(kind, reversed_, method, n_lm)]["memo_flavour_key"] == table[(kind, 0, 0, 0)]["memo_flavour_key"]
        got = dict(table[(kind, reversed_, method, n_lm)])
        got.pop("memo_flavour_key"), want.pop("memo_flavour_key")
        assert got == want, (kind, reversed_, method, n_lm)


def test_the_memo_key_distinguishes_what_the_former_expression_distinguished(driver):
    table = facts(driver)
    for a, b in itertools.combinations(sorted(table), 2):
        same_before = former_conditions(a[0], bool(a[1]), a[2], a[3])["memo_flavour_key"] == former_conditions(b[0], bool(b[1]), b[2], b[3])["memo_flavour_key"]
        assert (table[a]["memo_flavour_key"] == table[b]["memo_flavour_key"]) == same_before, (a, b)
