"""CPU: the oracle against an independent float64 renderer (tests/ideal_renderer.py) under derived tolerances
(tests/ideal_compare.py, SPEC.md "Accuracy against exact arithmetic").

The bit-exact GPU suite checks HIP == oracle; this module checks oracle == the operation, so that an error the oracle and
the kernels have in common (wrong interpolation weights, a swapped vertex, a wrong divisor, a product the wrong way round)
does not pass.  Every mutant of the ideal renderer must FAIL the comparison with the oracle on the scene named next to it:
that is what proves the rule has teeth.

Measured maxima, oracle against the ideal (CPU) and HIP against the ideal (MI355X; both tile kernels, both bin-queue
builders).  The two columns of figures are identical to the digits shown, as they must be: the oracle and the HIP path
agree bit for bit.  "2 terms" is the depth error over the first two terms of tol alone (snapping and the SPEC 6
roundings), to show what the third term, the rounding of the vertex stage carried to the pixel, is there for.  Coverage
and identity disagreements outside the ambiguous pixels: 0 on every scene, for both.

    scene                       size     tris  ambig%  tie%  depth/tol  2 terms  uv/bound  vertex/e
    capsule_12x20_160x96        160x 96    480   0.24  0.01      0.184     0.37         -     0.116
    capsule_24x40_320x200       320x200   1920   0.30  0.00      0.242     0.49         -     0.166
    capsule_30x48_333x171       333x171   2880   0.47  0.00      0.193     0.46         -     0.150
    capsule_60x100_640x360      640x360  12000   0.41  0.01      0.109     0.34         -     0.171
    capsule_short_palette       160x 96    480   0.16  0.00      0.138     0.45         -     0.150
    headline_12x20_480x270      480x270   9600   1.04  0.16      0.197     0.52         -     0.150
    lattice_poses_tree          192x112   5120   0.77  0.08      0.185     0.49         -     0.036
    lattice_poses_multi_root    192x112   5120   0.77  0.02      0.081     0.47         -     0.030
    floor_ceiling_capsule       320x200    484   0.66  0.01      0.242     5.38         -     0.378
    ramp_strip_w_range          320x200     25   0.07  0.00      0.361     0.42     0.499     0.418
    assembly_rules              192x112    384   0.30  0.00      0.309     0.45         -     0.388
    capsule_cull_none           320x200   1920   0.51  0.00      0.136     0.41         -     0.166
    capsule_cull_front          320x200   1920   0.22  0.00      0.136     0.41         -     0.166
    format_pos1x3_uv2x2_s16     160x 96    504   0.42  0.00      0.260     0.42     0.497     0.359
    format_pos5x3_uv10x4_s12    160x 96    504   0.43  0.00      0.198     0.37     0.500     0.992
    format_pos5x1_uv9x1_s6      160x 96    504   0.36  0.00      0.126     0.28     0.499     0.845
    format_pos9x3_uv10x1_s7     160x 96    504   0.38  0.00      0.493     0.62     0.498     0.992
    format_pos9x4_uv13x3_s8     160x 96    504   0.38  0.00      0.493     0.62     0.498     0.992
    format_pos2x2_uv5x1_s10     160x 96    504   0.35  0.00      0.155     0.29     0.498     0.860
    format_pos10x4_uv1x3_s19    160x 96    504   0.45  0.00      0.297     0.45     0.500     0.194
    format_pos1x3_uv5x3_s20     160x 96    504   0.42  0.00      0.260     0.42     0.500     0.860
    format_pos11x1_uv2x2_s8     160x 96    504   0.45  0.00      0.250     0.35     0.500     0.547

Palettes from poses (host routine on the CPU, k_pose on the MI355X) over their bound: 0.400 (tree_parents_after), 0.418
(multi_root).  The floor is 5.4 x over the first two terms on 78 % of its pixels (worst 3.4e-6): its clip-space z and w are
-39 and 61 at the vertices, one binary32 rounding of those is up to 3.8e-6, and a pixel sees it through
sum |lambda_i| (one or two of a triangle's vertices lie behind the eye, so the lambdas cancel); with the third term it sits at 0.26
of it.  vertex/e near 1 on the normalised formats is the single correctly rounded decode division of a texture coordinate
against its own half-ulp bound.  uv/bound of 0.5 is the half texel between the nearest filter and ``256 u - 0.5``.

The fragment stage (SPEC 7, 8, 10; scenes ``frag_*`` rendered with every fragment kept).  The figures are the oracle's against
the ideal, on the CPU; tests/test_gpu_ideal.py holds the HIP path (both tile kernels, both bin-queue builders, block-compressed
textures decoded at upload and block-resident) to the same rule on the same scenes.  No byte outside its interval on any scene.  "comp" compared pixels, "tex" textured
ones among them, "dec%" left out as decision-ambiguous (of the textured pixels), "1cand%" nearest samples with a single
candidate texel, "1byte%" bytes from exact sources whose interval is one byte, "bil" / "blend" the largest share of its
margin a byte uses (inexact / exact sources: distance from the centre of the real interval to the values that round to
the byte, over the interval's radius).

    scene                          size     tris  ambig%  tie%    comp     tex   dec%  1cand%  1byte%      bil   blend  depth/tol  vertex/e
    frag_magnified_patch           192x112     2   0.03  0.00   21498   13026   0.00   100.0   100.0    0.133   0.000   0.170   0.243
    frag_minified_no_mips          192x112     2   0.01  0.00   21463    7833   0.48    97.7   100.0    0.133   0.000   0.309   0.168
    frag_mip_chain                 192x112    20   0.09  0.00   21311   11729   1.46    98.6   100.0    0.000   0.000   0.253   0.379
    frag_layers_alpha              192x112    48   0.46  0.02   21401   12556   0.00   100.0   100.0    0.000   0.000   0.356   0.423
    frag_layers_off                192x112    48   0.46  0.02   21401   12556   0.00   100.0   100.0    0.000   0.000   0.356   0.423
    frag_layers_add                192x112    50   0.48  0.02   21396   17890   0.00   100.0   100.0    0.000   0.000   0.356   0.423
    frag_layers_mixed              192x112    50   0.48  0.02   21396   17890   0.00   100.0   100.0    0.000   0.000   0.356   0.423
    frag_depth_states              192x112    52   0.48  0.07   21384   17878   0.00   100.0   100.0    0.000   0.000   0.346   0.423
    frag_translucent_over_linear   192x112     4   0.07  0.00   21490   14718   0.00   100.0   100.0    0.971   0.000   0.275   0.388
    frag_bc_chains                 192x112    26   0.17  0.00   21408   14712   0.40    99.3   100.0    0.849   0.000   0.273   0.277
    frag_small_triangles_161x97    161x 97  4800   0.80  0.00   15462    1737   1.70    99.3   100.0    0.000   0.000   0.593   0.430
    frag_skinned_mips              160x 96   672   0.33  0.03   15259    2827   1.64    99.5   100.0    0.390   0.000   0.143   0.126
    frag_near_plane_translucent    192x112    24   0.04  0.00   21483    7467   0.16    99.5   100.0    0.258   0.000   0.503   0.418

blend 0.000 with 100 % one-byte intervals: on these scenes no exact value lies within the binary32 margin (1.8e-4 of a byte)
of ``k + 1/2``, and the oracle stores exactly the byte the exact chain rounds to.  bil near 1 on the two-layer scenes is the
lower layer's one-byte uncertainty carried through ``(1 - a)``, not the bilinear radius (0.13 on the single layer of
frag_magnified_patch).  Every level of the 100 x 60 chain wins 74 .. 4333 compared pixels; the clamp to ``L - 1`` decides 2691.

Fragment mutants, bytes outside their interval against the oracle: linear_no_half_texel 12075, wrap_not_clamp 8827,
coarse_derivatives 6, filter_x_only 944, level_from_min_product 7570, level_plus_one 8964, level_unclamped 2688,
level_size_no_max 78, add_without_alpha 10164, alpha_premultiplied 8803, alpha_blended 12339, dst_unquantised 515,
store_truncates 11254, no_prefix_minima 5758, depth_write_off_ignored 1192 (depth 13488 x tol), depth_test_off_ignored 4472
(depth 8852 x tol).

Mutants against the oracle: z_perspective_weights depth 2.2 x tol; uv_affine uv 159 x bound; flip_winding depth 310 x;
snorm16_div_32768 vertex stage 21 x e (the frame does not see it: 0.003 px); weights_div_256 132 coverage disagreements,
depth 19 x; joint_clamp_n 10 disagreements, depth 13 x; instance_model_times_vp 3044 disagreements; pose_child_on_left
palette 1.6e5 x bound; no_y_flip 2356 disagreements, 47522 wrong winners; clip_attr_from_outside uv 67 x bound.
"""
import os
import re

import pytest

from oracle import oracle as orc
from tests import ideal_compare as cmp
from tests import ideal_renderer
from tests import ideal_scenes as scenes
from tests.helpers import render_oracle

ALL = list(scenes.SCENES)


@pytest.mark.parametrize("name", ALL)
def test_scene_is_fit(name):
    """at most 2 % ambiguous pixels and 1 % near ties -- from the ideal renderer alone"""
    cmp.assert_scene_caps(scenes.ideal_of(name), name)
    if name in scenes.CONDITIONS:
        scenes.CONDITIONS[name](scenes.ideal_of(name))


@pytest.mark.parametrize("name", ALL)
def test_oracle_frame_against_exact_arithmetic(name):
    w, h, draws = scenes.scene_of(name)
    rep = cmp.compare(render_oracle(w, h, draws), scenes.ideal_of(name))
    print(f"{name}: {rep.line()}")
    if name in scenes.FRAGMENT_SCENES:
        print(f"{name}: {rep.fragment_line()}")
    assert rep.ok, (name, rep.failures)
    assert rep.compared > 0.02 * w * h


def oracle_vertex_ratio(name, mutate=None):
    """worst |oracle - ideal| / e over every vertex of every primitive of every draw of the scene"""
    ideal = scenes.ideal_of(name, mutate)
    cases = scenes.vertex_cases(name)
    worst, models = 0.0, {}
    for (di, inst, pr, clip, uv, e_clip, e_uv) in ideal.vertex:
        md, M, pal = cases[di]
        om = models.setdefault(id(md), orc.OracleModel(md))
        oc, ou = om.vertex_stage(pr, M, pal)
        worst = max(worst, cmp.vertex_stage_ratio(oc, ou, clip, uv, e_clip, e_uv))
    return worst


@pytest.mark.parametrize("name", ALL)
def test_oracle_vertex_stage_within_the_forward_error_bound(name):
    worst = oracle_vertex_ratio(name)
    print(f"{name}: vertex stage |err| / e = {worst:.3f}")
    assert worst <= 1.0, (name, worst)


def host_palette_ratio(name, mutate=None):
    d = scenes.scene_of(name)[2][0]
    parents, imats = d["skeleton"]
    pal, pabs, depth = ideal_renderer.palettes_from_poses(parents, imats, d["poses"], mutate)
    return cmp.palette_ratio(d["palettes"], pal, pabs, depth)


@pytest.mark.parametrize("name", ["lattice_poses_tree", "lattice_poses_multi_root"])
def test_host_palettes_against_float64_products(name):
    """mtr_rmodel_palette (what k_pose must equal bit for bit) against plain products, parent on the left"""
    worst = host_palette_ratio(name)
    print(f"{name}: palette |err| / bound = {worst:.3f}")
    assert worst <= 1.0, (name, worst)


# mutant -> (scene, the comparison that must catch it: frame / vertex / palette)
MUTANT_CASES = {
    "z_perspective_weights": ("capsule_24x40_320x200", "frame"),
    "uv_affine": ("ramp_strip_w_range", "frame"),
    "flip_winding": ("capsule_12x20_160x96", "frame"),
    # a 3e-5 relative change of the positions is about 0.003 px: under the snapping bound of the frame comparison, far over
    # the 1.4e-6 relative bound of the vertex stage
    "snorm16_div_32768": ("capsule_24x40_320x200", "vertex"),
    "weights_div_256": ("capsule_24x40_320x200", "frame"),
    "joint_clamp_n": ("capsule_short_palette", "frame"),
    "instance_model_times_vp": ("lattice_poses_tree", "frame"),
    # the poses bend by a few hundredths: the wrong order moves the surface by less than a frame can show, and the palette
    # elements by thousands of their bound
    "pose_child_on_left": ("lattice_poses_tree", "palette"),
    "no_y_flip": ("floor_ceiling_capsule", "frame"),
    "clip_attr_from_outside": ("ramp_strip_w_range", "frame"),
    # the fragment stage: every one is caught by the blend / texel line of the frame comparison
    "linear_no_half_texel": ("frag_magnified_patch", "frame"),
    "wrap_not_clamp": ("frag_magnified_patch", "frame"),
    "coarse_derivatives": ("frag_minified_no_mips", "frame"),
    "filter_x_only": ("frag_minified_no_mips", "frame"),
    "level_from_min_product": ("frag_mip_chain", "frame"),
    "level_plus_one": ("frag_mip_chain", "frame"),
    "level_unclamped": ("frag_mip_chain", "frame"),
    "level_size_no_max": ("frag_mip_chain", "frame"),
    "add_without_alpha": ("frag_layers_add", "frame"),
    "alpha_premultiplied": ("frag_layers_alpha", "frame"),
    "alpha_blended": ("frag_layers_alpha", "frame"),
    "dst_unquantised": ("frag_layers_alpha", "frame"),
    "store_truncates": ("frag_layers_alpha", "frame"),
    "no_prefix_minima": ("frag_layers_alpha", "frame"),
    "depth_write_off_ignored": ("frag_depth_states", "frame"),
    "depth_test_off_ignored": ("frag_depth_states", "frame"),
}


def test_every_mutant_has_a_case():
    assert set(MUTANT_CASES) == set(ideal_renderer.MUTANTS)


@pytest.mark.parametrize("mutate", list(ideal_renderer.MUTANTS))
def test_mutant_reference_fails_against_the_oracle(mutate):
    name, by = MUTANT_CASES[mutate]
    if by == "frame":
        w, h, draws = scenes.scene_of(name)
        rep = cmp.compare(render_oracle(w, h, draws), scenes.ideal_of(name, mutate))
        print(f"{mutate} on {name}: {rep.line()}")
        assert not rep.ok, f"the frame comparison does not notice {mutate} on {name}"
    elif by == "vertex":
        worst = oracle_vertex_ratio(name, mutate)
        print(f"{mutate} on {name}: vertex stage |err| / e = {worst:.1f}")
        assert worst > 1.0, f"the vertex-stage comparison does not notice {mutate} on {name}"
    else:
        worst = host_palette_ratio(name, mutate)
        print(f"{mutate} on {name}: palette |err| / bound = {worst:.1f}")
        assert worst > 1.0, f"the palette comparison does not notice {mutate} on {name}"


def test_the_ideal_renderer_stands_alone():
    """nothing compiled, no oracle, no api: only numpy, mt_renderer_amd.scene and the palette table"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ideal_renderer.py")).read()
    mods = set(re.findall(r"^\s*(?:from|import)\s+([\w.]+)", src, flags=re.M))
    assert mods <= {"__future__", "math", "numpy", "mt_renderer_amd", "tests.pixel_scenes"}, mods
    assert re.findall(r"^\s*from mt_renderer_amd import (.+)$", src, flags=re.M) == ["scene"]
    assert "ctypes" not in src and "oracle." not in src.replace("the oracle", "")
