"""CPU: the premises of tests/test_gpu_vertex_decode.py.

1. The reference decode tables of tests/vertex_decode_cases.py (integer arithmetic) equal the IEEE division as numpy does it,
   for every code, and the F16 table equals numpy's widening for every pattern that is no NaN; the oracle's vertex stage
   equals the reference on every exhaustive model (words equal, NaN by class), and the vectorised expectation under the
   identity equals the exact shade() of tests/vertex_edge_cases.py on a sample that holds every edge code.  So the GPU tests
   rest on three independent agreements.
2. Every model contains what it claims, read back from its bytes: each code in each component, each address residue of
   its placement, primitives of unequal sizes that are no multiple of 64, and in the skinned model every (weight byte,
   slot) in a coherent block and in one that is not.
3. The clip scenes: at least half of the triangles that reach set-up take the clipper's path in the near-plane view (0.56 to
   0.79 as generated), some do in the guard-band view (0.34 to 0.77), none in the plain view; every clip coordinate is
   finite, w is 1, a chunk of a list cannot exceed the record bound of SPEC 5.3, and the oracle renders every view.
"""
import numpy as np
import pytest

from mt_renderer_amd import scene
from oracle import oracle as orc
from tests import vertex_decode_cases as vd
from tests import vertex_edge_cases as vx
from tests.helpers import render_oracle

EXHAUSTIVE = [(p, r, pl) for p in vd.PAIRS for r in vd.ROLES for pl in vd.PLACEMENTS]


def _ieee(num: np.ndarray, d: float, clamp: bool) -> np.ndarray:
    q = num.astype(np.float32) / np.float32(d)
    return (np.maximum(q, np.float32(-1.0)) if clamp else q).view(np.uint32)


def test_reference_tables_equal_the_ieee_division():
    assert (vd.U8N_BITS == _ieee(np.arange(256), 255.0, False)).all()
    assert (vd.S8N_BITS == _ieee(np.arange(256).astype(np.uint8).view(np.int8), 127.0, True)).all()
    assert (vd.S16N_BITS == _ieee(np.arange(65536).astype(np.uint16).view(np.int16), 32767.0, True)).all()
    s10 = np.arange(1024)
    assert (vd.SCMP_BITS == _ieee(np.where(s10 >= 512, s10 - 1024, s10), 511.0, True)).all()
    # the one code each clamp exists for, and its neighbour, which needs none
    for tab, lo in ((vd.S8N_BITS, 0x80), (vd.S16N_BITS, 0x8000), (vd.SCMP_BITS, 0x200)):
        assert tab[lo] == tab[lo + 1] == vd.NEG_ONE and tab[lo - 1] == vd.ONE and tab[0] == 0
    assert vd.S16N_BITS[0x8000] == vx.snorm16_bits(-32768) and (vd.U8N_BITS == np.array(vx.UNORM8, dtype=np.uint32)).all()


def test_f16_table_equals_numpy_widening():
    h = np.arange(65536, dtype=np.uint16).view(np.float16)
    wide = h.astype(np.float32).view(np.uint32)
    nan = np.isnan(h)
    assert int(nan.sum()) == 2046
    assert (vd.F16_BITS[~nan] == wide[~nan]).all()               # subnormals, signed zeros and infinities included
    assert ((vd.F16_BITS[nan] & 0x7FFFFFFF) > vd.INF).all()      # NaN -> some NaN
    assert vd.F16_BITS[0x8000] == 0x80000000 and vd.F16_BITS[0x0001] == 0x33800000 and vd.F16_BITS[0x7BFF] == 0x477FE000


def _fields_in_memory(md, prim: int, el) -> np.ndarray:
    """the raw fields of element `el` of every vertex of a primitive, read back from the model's bytes alone"""
    f = scene.unpack_primitive(md.prims[prim])
    pair = next(p for p in vd.PAIRS.values() if (p.fmt, p.cnt) == (el[1], el[2]))
    addr = f["vertex_base"] + np.arange(f["vertex_num"]) * f["vertex_stride"] + el[3]
    raw = md.vertex_buf[addr[:, None] + np.arange(pair.nbytes)[None, :]].astype(np.uint32)
    if pair.bits == 8:
        return raw[:, :pair.ncomp], addr
    if pair.bits == 16:
        return (raw[:, 0:2 * pair.ncomp:2] | (raw[:, 1:2 * pair.ncomp:2] << 8)), addr
    w = raw[:, 0::4] | (raw[:, 1::4] << 8) | (raw[:, 2::4] << 16) | (raw[:, 3::4] << 24)
    if pair.bits == 32:
        return w, addr
    return np.stack([(w[:, 0] >> s) & 0x3FF for s in (0, 10, 20)], axis=1), addr


@pytest.mark.parametrize("pair,role,placement", EXHAUSTIVE, ids=lambda v: v)
def test_exhaustive_models_hold_every_code_at_every_residue(pair, role, placement):
    c = vd.exhaustive_case(pair, role, placement)
    sem = scene.SEM_POSITION if role == "position" else scene.SEM_TEXCOORD
    fields, addrs = [], []
    for prim in range(len(c.prims)):
        el = next(e for e in c.md.layouts[prim] if e[0] == sem)
        assert (el[1], el[2]) == (c.pair.fmt, c.pair.cnt) and len(el) == (5 if c.pair.flags else 4)
        f, a = _fields_in_memory(c.md, prim, el)
        fields.append(f)
        addrs.append(a)
    fields, addrs = np.concatenate(fields), np.concatenate(addrs)
    assert (fields == c.exp.codes).all()
    want = set(vd.F32_LIST) if c.pair.fmt == scene.IEF_F32 else set(range(c.pair.ncodes))
    for comp in range(c.pair.ncomp):
        assert want <= set(fields[:, comp].tolist()), (c.name, comp)
    assert all(len(set(row)) == len(row) for row in fields[:: max(1, len(fields) // 997)].tolist())  # rotated: no two components alike
    assert set((addrs & 3).tolist()) == vd.PLACEMENT_RESIDUES[placement]
    sizes = [n for _, n in c.prims]
    assert len(set(sizes)) == len(sizes) == 3 and all(n % 64 for n in sizes) and sum(sizes) == len(c.exp.codes) and max(sizes) <= 0xFFFF
    assert len(c.exp.sample) >= 256 and set(vd.edge_codes(c.pair)) <= set(c.exp.codes[c.exp.sample].reshape(-1).tolist())
    # the bytes between the elements are the fill, not zero
    assert int((c.md.vertex_buf == 0xA5).sum() + (c.md.vertex_buf == 0x5A).sum()) >= len(fields)


def test_placements_cover_every_residue_and_both_alignment_flags():
    assert set().union(*vd.PLACEMENT_RESIDUES.values()) == {0, 1, 2, 3}
    for placement in vd.PLACEMENTS:
        base, off, other, stride = vd.place(8, 2, placement)
        assert (((base | off | other | stride) & 3) == 0) == (placement == "aligned")
    assert vd.place(4, 2, "half")[1] == 2 and vd.place(4, 2, "half")[3] % 4 == 2
    assert vd.place(4, 2, "odd")[0] % 2 == 1 and vd.place(4, 2, "odd")[3] % 2 == 1
    assert vd.place(4, 2, "base3")[0] % 4 == 3 and vd.place(4, 2, "base3")[1] % 2 == 1


@pytest.mark.parametrize("pair,role,placement", EXHAUSTIVE, ids=lambda v: v)
def test_oracle_vertex_stage_equals_the_reference(pair, role, placement):
    c = vd.exhaustive_case(pair, role, placement)
    om = orc.OracleModel(c.md)
    for prim, (v0, n) in enumerate(c.prims):
        oc, ou = om.vertex_stage(prim, vd.IDENTITY_M)
        for what, got, ref in (("clip", oc, c.exp.clip[v0:v0 + n]), ("uv", ou, c.exp.uv[v0:v0 + n])):
            ok = vd.same_words(got, ref, nan_by_class=not (what == "uv" and c.uv_is_bits))
            assert ok.all(), vd.describe_difference(c, f"oracle {what}, prim {prim}", v0, ok, got, ref)
    if role == "position" and placement == "aligned":  # a matrix with no zero in it, on the sample: exactly shade()
        got = np.concatenate([om.vertex_stage(prim, vx.HEADLINE_M)[0] for prim in range(len(c.prims))])[c.exp.sample]
        assert vd.same_words(got, vd.headline_clip(pair)).all()


@pytest.mark.parametrize("pair", list(vd.PAIRS))
@pytest.mark.parametrize("role", vd.ROLES)
def test_identity_expectation_equals_the_exact_model_on_the_sample(pair, role):
    e = vd.expected(pair, role)
    exact = vd.shade_words(e.pos_bits, vd.IDENTITY_M, e.sample)
    assert vd.same_words(e.clip[e.sample], exact).all()
    if role == "position":
        p = vd.PAIRS[pair]
        assert (e.clip[:, 3] == vd.ONE).all() or p.fmt in (scene.IEF_F16, scene.IEF_F32)
        assert p.ncomp == 3 or (e.clip[:, 2] & 0x7FFFFFFF == 0).all() or p.fmt == scene.IEF_F16  # F16: NaN where x or y is not finite
        if p.fmt == scene.IEF_F16:
            fin = (e.pos_bits & 0x7FFFFFFF < vd.INF).all(axis=1)
            assert (e.clip[fin, 2] == 0).all() and int(fin.sum()) >= 65536 - 4 * 1024
    else:
        if vd.PAIRS[pair].fmt in (scene.IEF_F16, scene.IEF_F32):  # the only formats with a -0: it reaches the output untouched
            assert int((e.uv == 0x80000000).sum()) >= 2


def test_weight_model_meets_both_kinds_of_block():
    c = vd.weight_case()
    pats = np.concatenate([np.array(c.patterns(p)) for p in range(len(c.prims))])
    coherent = pats == "coherent"
    assert coherent.sum() >= 512 and (~coherent).sum() >= 512
    slot = c.weights.argmax(axis=1)
    byte = c.weights.max(axis=1)
    assert ((c.weights != 0).sum(axis=1) <= 1).all()
    for kind in (coherent, ~coherent):
        seen = set(zip(byte[kind].tolist(), slot[kind].tolist()))
        assert all((b, s) in seen for b in range(1, 256) for s in range(4))
    assert (byte == 0).sum() >= 2 and coherent[byte == 0].any() and (~coherent)[byte == 0].any()
    sizes = [n for _, n in c.prims]
    assert all(n % 64 for n in sizes) and len(set(sizes)) == 3
    assert (vd.weight_clip(1)[:, 0] == vd.U8N_BITS[byte]).all()  # one identity matrix: clip.x is the decoded weight
    assert (vd.weight_clip(1)[:, 1:] == np.array([0, 0, vd.ONE], dtype=np.uint32)).all()
    om = orc.OracleModel(c.md)
    for npal in vd.WEIGHT_NPALS:
        got = np.concatenate([om.vertex_stage(p, vd.IDENTITY_M, c.pal[:npal])[0] for p in range(len(c.prims))])
        assert vd.same_words(got, vd.weight_clip(npal)).all(), npal


# ---------------------------------------------------------------------------------------------
# clip scenes
# ---------------------------------------------------------------------------------------------
def clip_path_counts(clip: np.ndarray, idx: np.ndarray, W: int, H: int):
    """(triangles that take the clipper's path, triangles that reach set-up or the clipper) from clip coordinates alone: SPEC
    5 steps 1 to 3 -- not trivially rejected, and some vertex with z < 0, w <= 0 or outside the guard band"""
    x, y, z, w = (clip[:, k].astype(np.float32) for k in range(4))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iw = np.float32(1.0) / w
        xf = ((x * iw).astype(np.float64) * (W / 2) + W / 2).astype(np.float32)
        yf = ((-(y * iw)).astype(np.float64) * (H / 2) + H / 2).astype(np.float32)
    ok = (w > 0) & (np.abs(xf) <= 2.0 ** 20) & (np.abs(yf) <= 2.0 ** 20)
    t = idx.reshape(-1, 3).astype(np.int64)
    rejected = np.zeros(len(t), dtype=bool)
    for out in (x < -w, x > w, y < -w, y > w, z < 0, z > w):
        rejected |= out[t].all(axis=1)
    clipped = ~rejected & ((z < 0)[t].any(axis=1) | ~ok[t].all(axis=1))
    return int(clipped.sum()), int((~rejected).sum())


@pytest.mark.parametrize("name", vd.CLIP_SCENE_NAMES)
def test_clip_scenes_take_the_clip_path_and_stay_inside_the_spec(name):
    s = vd.clip_scene(name)
    md = s.md
    f = scene.unpack_primitive(md.prims[0])
    assert vd.CLIP_W <= 256 and vd.CLIP_H <= 160 and md.nprims == 1 and f["topology"] == scene.TOPO_LIST
    assert 300 <= len(md.index_buf) // 3 <= 600 and int(md.index_buf.max()) < f["vertex_num"]
    # a list chunk of 62 index positions completes at most 21 triangles, each a fan of at most 6: within the 124 records
    assert 21 * 6 <= 126 and (62 // 3 + 1) * 6 - 2 <= 124
    # both elements are the pair, and every edge code is in every component of both
    pos_el, uv_el = md.layouts[0]
    assert pos_el[0] == scene.SEM_POSITION and uv_el[0] == scene.SEM_TEXCOORD and pos_el[1:3] == uv_el[1:3] == (s.pair.fmt, s.pair.cnt)
    klass = name.rsplit("-", 1)[1]
    for el in (pos_el, uv_el):
        fields, addr = _fields_in_memory(md, 0, el)
        for comp in range(s.pair.ncomp):
            assert set(vd.frame_edges(s.pair)) <= set(fields[:, comp].tolist())
        used = fields[np.unique(md.index_buf)]
        assert all(set(vd.frame_edges(s.pair)) <= set(used[:, comp].tolist()) for comp in range(s.pair.ncomp))
        assert set((addr & 3).tolist()) == ({0} if klass == "aligned" else {0, 1, 2, 3})
        if s.pair.fmt not in vd.FRAME_FLOAT_EDGES:  # the whole range: both halves of it, in every component
            assert all((fields[:, comp] >= s.pair.ncodes // 2).sum() > 100 and (fields[:, comp] < s.pair.ncodes // 2).sum() > 100
                       for comp in range(s.pair.ncomp))
    om = orc.OracleModel(md)
    shares = {}
    for view in ("plain", "near", "guard"):
        clip, uv = om.vertex_stage(0, s.views[view])
        assert np.isfinite(clip).all() and np.isfinite(uv).all() and (clip[:, 3] == 1.0).all(), (name, view)
        shares[view] = clip_path_counts(clip, md.index_buf, vd.CLIP_W, vd.CLIP_H)
        _, depth, stats = render_oracle(vd.CLIP_W, vd.CLIP_H, s.draws(view))
        assert stats["tris_setup"] > 0 and int((depth < 1.0).sum()) >= 256, (name, view, stats)
    print(name, {v: f"{a} / {b}" for v, (a, b) in shares.items()})
    assert shares["plain"][0] == 0 and shares["plain"][1] == len(md.index_buf) // 3
    assert 2 * shares["near"][0] >= shares["near"][1] > 0
    assert shares["guard"][0] > 0
    # the guard-band view does leave the band, and on both sides
    clip, _ = om.vertex_stage(0, s.views["guard"])
    xf = clip[:, 0].astype(np.float64) * vd.CLIP_W / 2 + vd.CLIP_W / 2
    assert (xf > 2.0 ** 20).sum() >= 16 and (xf < -2.0 ** 20).sum() >= 16
