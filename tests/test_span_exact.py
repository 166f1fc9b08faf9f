"""CPU: csrc/span_row.h -- the exact run of covered columns that k_tile_vis.hip's span walk computes for one bbox row --
against the per-pixel inside test (every column of every row of >= 10^6 i32-class triangles set up by csrc/tri_setup.h:
vertices anywhere, on pixel centres and on bin corners, horizontal and vertical edges, long slivers, boxes clipped by the
bin and by the viewport, edge values near the class limit).  The row bounds come from an f32 estimate settled by one
integer evaluation, so the check is repeated with the reciprocal 1 ulp off either way (v_rcp_f32's error bound), and a
reciprocal 3 % off must be caught."""
import subprocess

import pytest

from tests import cpp_build


RCP = {
    "exact": "(1.0f/(x))",
    "ulp_up": "std::nextafter(1.0f/(x),INFINITY)",
    "ulp_down": "std::nextafter(1.0f/(x),-INFINITY)",
}


def _build(tmp_path, name, rcp):
    return cpp_build.build("span_exact", tmp_path, cpp_build.BARE, extra=["-ffp-contract=off", f"-DMTR_SPAN_RCP(x)={rcp}", "-include", "cmath"],
                           exe=f"span_exact_{name}")


@pytest.mark.parametrize("name", sorted(RCP))
def test_span_of_row_matches_inside_test(tmp_path, name):
    exe = _build(tmp_path, name, RCP[name])
    out = subprocess.run([exe, "1000000", "20261016"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    tris, rows, nonempty, inner, bad = (int(v) for v in out.stdout.split())
    assert tris >= 1000000 and bad == 0
    # the check has teeth: half the triangles are wound the way that covers nothing, and most of the other half's runs end
    # inside their bbox row, where a bound one column off changes the covered set
    assert nonempty > rows // 8 and inner > nonempty // 2, out.stdout


def test_inexact_reciprocal_is_caught(tmp_path):
    exe = _build(tmp_path, "coarse", "(1.03f/(x))")
    out = subprocess.run([exe, "200000", "7"], capture_output=True, text=True)
    assert out.returncode == 1 and int(out.stdout.split()[4]) > 0, out.stdout
