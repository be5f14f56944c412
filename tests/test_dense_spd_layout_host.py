"""The workspace layout of the blocked SPD solve (gingr_amd/csrc/dense_spd.h: DenseSpdWork) against the offsets its users carved by
hand before there was one type for it: launch_posterior_solve and the two systems of launch_posterior_logpdf (right-hand-side border),
launch_posterior_factor (identity border, factor only) and launch_binv (identity border with the product).  A wrong size or offset
here is a write past a device allocation, so the old expressions are written out below and every offset must equal them.  Host
arithmetic only: tests/c/dense_spd_layout.cpp is built with the plain C++ compiler, no device and no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKS = [16, 112, 128, 256, 304, 400, 512]  # padded ranks: below one block, 64-multiples and the ones in between, the largest


def _round_up(a, b):
    return (a + b - 1) // b * b


def _hand_carved(rp):
    """The expressions of the launchers and size functions as they stood, in doubles from the start of `work`."""
    Mp = _round_up(rp, 64)
    nb = Mp // 64
    solve = {"Mp": Mp, "rows": Mp + 64, "aw": 0, "linv": (Mp + 64) * Mp, "w": (Mp + 64) * Mp + nb * 64 * 64,
             "flag": (Mp + 64) * Mp + nb * 64 * 64 + 3 * Mp, "doubles": (Mp + 64) * Mp + nb * 4096 + 3 * Mp + 2}
    factor = {"Mp": Mp, "rows": 2 * Mp, "aw": 0, "lt": Mp * Mp, "linv": 2 * Mp * Mp, "flag": 2 * Mp * Mp + (Mp // 64) * 64 * 64,
              "doubles": 2 * Mp * Mp + (Mp // 64) * 64 * 64 + 1}
    binv = {"Mp": Mp, "rows": 2 * Mp, "aw": 0, "lt": Mp * Mp, "c": 2 * Mp * Mp, "linv": 3 * Mp * Mp,
            "doubles": 3 * Mp * Mp + (Mp // 64) * 64 * 64}
    return {"solve": solve, "factor": factor, "binv": binv}


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dense_spd") / "dense_spd_layout"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "dense_spd_layout.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)] + [str(r) for r in RANKS], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        use, rp, *fields = line.split()
        table[(use, int(rp))] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return table


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("rp", RANKS)
def test_offsets_equal_the_hand_carved_ones(layout, rp):
    for use, want in _hand_carved(rp).items():
        got = dict(layout[(use, rp)])
        assert got.pop("static") == want["doubles"], (use, rp)
        assert got == want, (use, rp)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("rp", RANKS)
def test_parts_do_not_overlap_and_fit(layout, rp):
    """Each part ends where the next begins or before, the last inside doubles(); the second system of the transition density
    (at doubles() of the first) starts 16-byte aligned."""
    Mp = _round_up(rp, 64)
    linv_doubles = (Mp // 64) * 4096
    s, f, b = layout[("solve", rp)], layout[("factor", rp)], layout[("binv", rp)]
    assert s["aw"] + s["rows"] * Mp <= s["linv"] and s["linv"] + linv_doubles <= s["w"] and s["w"] + 3 * Mp <= s["flag"] < s["doubles"]
    assert s["doubles"] % 2 == 0
    assert f["lt"] + Mp * Mp == f["aw"] + f["rows"] * Mp <= f["linv"] and f["linv"] + linv_doubles <= f["flag"] < f["doubles"]
    assert b["aw"] + b["rows"] * Mp <= b["c"] and b["c"] + Mp * Mp <= b["linv"] and b["linv"] + linv_doubles <= b["doubles"]
