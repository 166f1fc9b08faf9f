"""CPU: the premises of tests/test_gpu_frame_shapes.py, from the float64 reference (tests/ideal_renderer.py) and the oracle
alone.  The scenes of tests/frame_shape_scenes.py are fit for the comparison of tests/ideal_compare.py on every long shape,
the oracle agrees with the reference on them, mutants of the reference fail there, the crop property holds on the oracle,
and each shape is in its list for the reason given next to the assertion.

Measured, oracle against the reference (CPU) and HIP against the reference (MI355X; both tile kernels, both bin-queue
builders): the HIP figures equal the oracle's to the digits shown on every row ("="), as they must, the two agreeing bit
for bit.  Coverage and identity disagreements outside the ambiguous pixels, bytes outside their interval: 0 on every row,
for both.  "dec%" decision-ambiguous share of the textured pixels, "bil" / "blend" the largest share of its margin a byte
uses (inexact / exact sources), as in tests/test_ideal_vs_oracle.py.

    scene                  tris  ambig%   tie% compared   d/tol   dec%    bil  blend   HIP
    16384x1 ids             194    0.73  0.000    16265   0.579      -      -      -   =
    16384x1 tex             194    0.73  0.000    16265   0.579   0.00  0.062  0.000   =
    16384x1 alpha           194    0.73  0.006    16265   0.579   0.00  0.060  0.000   =
    1x16384 ids             194    0.76  0.000    16260   0.638      -      -      -   =
    1x16384 tex             194    0.76  0.000    16260   0.638   0.00  0.086  0.000   =
    1x16384 alpha           194    0.76  0.006    16260   0.638   0.00  0.068  0.000   =
    16384x16 ids            194    0.06  0.003   261992   0.596      -      -      -   =
    16384x16 tex            194    0.06  0.003   261992   0.596   0.00  0.161  0.000   =
    16384x16 alpha          194    0.06  0.003   261992   0.596   0.00  0.994  0.000   =
    16x16384 ids            194    0.06  0.004   261983   0.620      -      -      -   =
    16x16384 tex            194    0.06  0.004   261983   0.620   0.00  0.108  0.000   =
    16x16384 alpha          194    0.06  0.003   261983   0.620   0.00  0.995  0.000   =
    16381x3 ids             194    0.23  0.008    49028   0.697      -      -      -   =
    16381x3 tex             194    0.23  0.008    49028   0.697   0.00  0.133  0.000   =
    16381x3 alpha           194    0.23  0.006    49028   0.697   0.00  0.110  0.000   =
    5x16383 ids             194    0.17  0.001    81774   0.619      -      -      -   =
    5x16383 tex             194    0.17  0.001    81774   0.619   0.00  0.423  0.000   =
    5x16383 alpha           194    0.17  0.001    81774   0.619   0.00  0.128  0.000   =
    8200x40 ids             194    0.06  0.005   327815   0.621      -      -      -   =
    8200x40 tex             194    0.06  0.005   327815   0.621   0.00  0.221  0.000   =
    8200x40 alpha           194    0.06  0.005   327815   0.621   0.00  0.995  0.000   =
    lattice 64x64           180    1.05  0.049     2641   0.003      -      -      -   =
    lattice 16384x16       2160    0.15  0.000    11669   0.001      -      -      -   =
    lattice 16x16384       2160    0.17  0.009    14915   0.002      -      -      -   =

Compared pixels per level of the 7-level chain / by the linear filter (variant ``tex``), and winner changes along the long
axis (``ids``): 16384x1 [0, 0, 0, 11953, 2157, 2155, 0] / 5269, 50; 1x16384 [0, 0, 0, 11952, 2155, 2153, 0] / 5267, 50;
16384x16 [34713, 46282, 34719, 38418, 34711, 34719, 0] / 123217, 50; 16x16384 the same within 7; 16381x3 [0, 22341, 6499,
7190, 6500, 6494, 0] / 15879, 50; 5x16383 [0, 37283, 10836, 11984, 10827, 10843, 0] / 26483, 50; 8200x40 [43437, 57922,
43415, 48084, 43432, 43432, 0] / 154217, 50.  On the frames one pixel thick the first strip never samples below level 3:
the product across the frame, 60 texels over 7.58 px, comes from the quad partner outside the frame.  bil near 1 on the
``alpha`` rows is the lower layer's one-byte uncertainty carried through ``(1 - a)``, as on the two-layer scenes there.

Mutants against the oracle: z_perspective_weights depth 1777 x tol (16384x16) and 1887 x (16x16384), 1157 and 1074 wrong
winners; uv_affine 112355 and 107973 bytes outside their interval (the fragment rule: tests/ideal_renderer.py applies the
mutant to the per-fragment coordinates too); no_y_flip on 16x16384 depth 171231 x tol, 73093 wrong winners.

What did not work, and why the scenes are as they are.  Random triangles in NDC on a 16384 x 1 frame put the oracle 227 x
the winner's tol off at one pixel, and that is no rendering bug: ``near_ties`` weighs the gap between the two nearest
fragments against the WINNER's tolerance only, and on a frame one pixel tall the loser's depth changes by about 1 over
half a pixel, so its snapping error alone decides the winner where the rule sees a clear lead.  The rule stays as it is;
the ribbon keeps z and clip w functions of the long-axis coordinate.  Two copies of the lattice triangles cover 1 % of a
16384 x 16 frame, under the 2 % the caps and the comparison ask for: the long lattice frames hold twelve.
"""
import functools

import numpy as np
import pytest

from tests import frame_shape_scenes as fs
from tests import ideal_compare as cmp
from tests.helpers import render_oracle

LONG_CASES = [(w, h, v) for (w, h) in fs.LONG for v in fs.VARIANTS]


def shape_id(case):
    return f"{case[0]}x{case[1]}" + "".join(f"-{c}" for c in case[2:])


@functools.lru_cache(maxsize=None)
def oracle_ribbon(w, h, variant):
    return render_oracle(w, h, fs.ribbon(w, h, variant))


@functools.lru_cache(maxsize=None)
def oracle_lattice(w, h, far):
    return render_oracle(w, h, fs.lattice(w, h, far))


# -------------------------------------------------------------------------------------------------------------------
# fitness: from the reference alone
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LONG_CASES, ids=shape_id)
def test_ribbon_is_fit_on_every_long_shape(case):
    """2 % ambiguous, 1 % near ties; textured variants: 2 % decision-ambiguous, and the linear filter and at least three
    levels of the 7-level chain win at least 20 compared pixels each"""
    w, h, variant = case
    ideal = fs.ribbon_ideal(w, h, variant)
    cmp.assert_scene_caps(ideal, shape_id(case))
    if variant != "ids":
        assert cmp.expected(ideal).decision_share <= cmp.DECISION_CAP
        wins, linear = fs.level_wins(ideal)
        print(f"{shape_id(case)}: compared pixels per level of the 7-level chain {wins.tolist()}, linear {linear}")
        assert int((wins >= 20).sum()) >= 3, wins.tolist()
        assert linear >= 20, linear


@pytest.mark.parametrize("shape,far", fs.LATTICE_FRAMES, ids=lambda a: shape_id(a) if isinstance(a, tuple) else str(a))
def test_lattice_is_fit(shape, far):
    cmp.assert_scene_caps(fs.lattice_ideal(*shape, far), f"lattice {shape_id(shape)}")


# -------------------------------------------------------------------------------------------------------------------
# the oracle against the reference
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LONG_CASES, ids=shape_id)
def test_oracle_ribbon_against_exact_arithmetic(case):
    w, h, variant = case
    rep = cmp.compare(oracle_ribbon(w, h, variant), fs.ribbon_ideal(w, h, variant))
    print(f"{shape_id(case)}: {rep.line()}")
    if variant != "ids":
        print(f"{shape_id(case)}: {rep.fragment_line()}")
    assert rep.ok, (case, rep.failures)
    assert rep.compared > 0.02 * w * h


@pytest.mark.parametrize("shape,far", fs.LATTICE_FRAMES, ids=lambda a: shape_id(a) if isinstance(a, tuple) else str(a))
def test_oracle_lattice_against_exact_arithmetic(shape, far):
    w, h = shape
    rep = cmp.compare(oracle_lattice(w, h, far), fs.lattice_ideal(w, h, far))
    print(f"lattice {shape_id(shape)}: {rep.line()}")
    assert rep.ok, (shape, rep.failures)
    assert rep.compared > 0.02 * w * h


# -------------------------------------------------------------------------------------------------------------------
# teeth
# -------------------------------------------------------------------------------------------------------------------
MUTANT_CASES = [("z_perspective_weights", 16384, 16, "ids"), ("z_perspective_weights", 16, 16384, "ids"),
                ("uv_affine", 16384, 16, "tex"), ("uv_affine", 16, 16384, "tex"), ("no_y_flip", 16, 16384, "ids")]


@pytest.mark.parametrize("mutate,w,h,variant", MUTANT_CASES, ids=[f"{m[0]}-{m[1]}x{m[2]}" for m in MUTANT_CASES])
def test_mutant_reference_fails_on_a_long_frame(mutate, w, h, variant):
    rep = cmp.compare(oracle_ribbon(w, h, variant), fs.ribbon_ideal(w, h, variant, mutate))
    print(f"{mutate} on {w}x{h}: {rep.line()}; {rep.fragment_line() if variant != 'ids' else ''}")
    assert not rep.ok, f"the comparison does not notice {mutate} on the {w}x{h} ribbon"


# -------------------------------------------------------------------------------------------------------------------
# the crop property
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small,large,far", fs.CROPS, ids=[f"{shape_id(s)}-of-{shape_id(l)}" for s, l, _ in fs.CROPS])
def test_oracle_small_frame_is_the_crop_of_a_larger_one(small, large, far):
    """vertices on the 1/256 px lattice snap back to it whatever the frame's size: colour and depth bits are equal"""
    (w, h), (W, H) = small, large
    c, d, st = oracle_lattice(w, h, far)
    C, D, _ = oracle_lattice(W, H, far)
    assert (c == C[:h, :w]).all(), int((c != C[:h, :w]).any(axis=-1).sum())
    assert (d.view(np.uint32) == D[:h, :w].view(np.uint32)).all()
    assert st["tris_in"] == fs.LATTICE_TRIS * (fs.LATTICE_COPIES if far else 1)
    assert (d < 1.0).any(), "the crop holds no geometry"
    if far:  # the last copy is in the crop: geometry within 80 px of the long axis's far end
        assert (d[-80:, -80:] < 1.0).any()


# -------------------------------------------------------------------------------------------------------------------
# each shape is there for a reason
# -------------------------------------------------------------------------------------------------------------------
def test_shard_widths_take_every_copy_path():
    widths = [w for w, _ in fs.SHARD]
    assert any(w % 16 == 0 for w in widths), "uint4 path, whole bins"
    assert any(w % 4 == 0 and w % 16 != 0 for w in widths), "uint4 path, ragged right edge"
    assert any(w % 2 == 1 and w > 4096 for w in widths), "scalar path at a large odd width"
    assert any((w + 15) // 16 * ((h + 15) // 16) < 3 for w, h in fs.SHARD), "fewer bins than a world of 3 has ranks"


def test_grid_needs_several_scan_rounds_at_the_widest_bin_row():
    (w, h), = fs.GRID
    nbx, nby = (w + 15) // 16, (h + 15) // 16
    assert nbx == 1024 and nbx * nby > 1024 and nbx * nby == 17 * 1024


def test_shapes_span_the_limits():
    assert (1, 1) in fs.TINY and all(w < 64 and h < 64 for w, h in fs.TINY)
    assert any(min(s) < 16 for s in fs.TINY) and max(max(s) for s in fs.LONG) == 16384
    assert {min(s) for s in fs.LONG} >= {1, 3, 5, 16}
    assert all(max(s) > 3840 for s in fs.LONG + fs.GRID)


@pytest.mark.parametrize("shape", fs.LONG, ids=shape_id)
def test_ribbon_changes_winner_along_the_long_axis(shape):
    changes, ids = fs.winner_changes(fs.ribbon_ideal(*shape, "ids"))
    print(f"{shape_id(shape)}: {changes} winner changes")
    assert ids >= set(fs.IDS), ids
    assert changes >= 40, changes


@pytest.mark.parametrize("shape", [s for s in fs.LONG if s[0] % 16 or s[1] % 16], ids=shape_id)
def test_ragged_long_frames_are_covered_in_their_last_column_and_row(shape):
    ideal = fs.ribbon_ideal(*shape, "ids")
    assert ideal.covered[:, -1].any() and ideal.covered[-1, :].any()
