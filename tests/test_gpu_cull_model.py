"""-m gpu: geometry culling against its float64 model (tests/cull_model.py), chunk by chunk.

Every draw of every scene of tests/cull_scenes.py is rendered alone in a frame, as each rank of each ownership map, and
the frame's ``chunks_culled`` must be the number the model predicts -- not a bound on it.  The scenes are placed so
that the model has no ambiguous decision (tests/test_cull_model_premises.py), so a kernel whose margin, slack, row
reduction, tail mask, box loop, straddler stride or chunk-box lookup is off by anything that matters reports another
number.  On a failure the model's decision for every instance and chunk is printed next to the count.

Then: the straddler-hint sequence of one persistent batch (also with MTR_GEOM_SLOTS=1), all draws of a scene in one
frame (the per-draw offsets into the culling buffers), the interval of geom_cull.h against the real vertex stage, and
soundness (same owned pixels and set-up counts with culling off) on the same scenes.
"""
import numpy as np
import pytest

from mt_renderer_amd import sharding
from tests import cull_model as cm
from tests import cull_scenes as cs
from tests import vertex_edge_cases as vx

pytestmark = pytest.mark.gpu

W, H = cs.W, cs.H
SCENES_OF = {f: [n for n, s in cs.scenes().items() if s.family == f] for f in cs.FAMILIES}


class Resident:
    """the models and persistent batches of a draw list on a device"""

    def __init__(self, dev, draws):
        from mt_renderer_amd import api
        self.dev, self.draws, self.models, self.batches = dev, draws, {}, {}
        for i, d in enumerate(draws):
            md = d["md"]
            if id(md) not in self.models:
                m = api.Model.new(dev, md)
                if "parts_disp" in d:
                    m.set_parts_disp(d["parts_disp"])
                self.models[id(md)] = m
            if "model_mats" in d:
                self.batches[i] = api.Batch(dev, self.models[id(md)], d["model_mats"], d.get("palettes"))

    def frame(self, which, map_name, world, rank, cull=True, pixels=False):
        """one frame of the draws `which`, as `rank` of `world` under the map (cs.WORLD1: unsharded, all-frames culling)"""
        from mt_renderer_amd import api
        shard = cs.shard_of(map_name, world, rank)
        self.dev.set_culling(api.GEOM_CULL_OFF if not cull else (api.GEOM_CULL_ALL_FRAMES if shard is None else api.GEOM_CULL_SHARDED))
        fr = api.Frame(self.dev, W, H)
        try:
            if shard is not None:
                fr.set_shard(*shard)
            for i in which:
                d = self.draws[i]
                if i in self.batches:
                    fr.draw_batch(self.batches[i], d["vp"])
                else:
                    m = self.models[id(d["md"])]
                    m.set_palette(d.get("palette"))
                    m.render(fr, d["M"])
            fr.end()
            st = fr.stats()
            return (fr.color(), fr.depth().view(np.uint32), st) if pixels else st
        finally:
            fr.close()
            self.dev.set_culling(api.GEOM_CULL_SHARDED)

    def close(self):
        for b in self.batches.values():
            b.close()
        for m in self.models.values():
            m.close()


def _check_draw(res, scene_name, di, cfg, what=""):
    p = cm.predict(res.draws[di], W, H, cs.shard_of(*cfg))
    assert p.n_ambiguous == 0 and p.culled_lo == p.culled_hi
    st = res.frame([di], *cfg)
    print(f"{scene_name} draw {di} {cfg}{what}: chunks {st['chunks']}, culled {st['chunks_culled']}, predicted {p.culled_lo}")
    assert st["chunks"] == p.chunks, (scene_name, di, cfg, st["chunks"], p.chunks)
    assert st["chunks_culled"] == p.culled_lo, f"{scene_name} draw {di} as {cfg}{what}: the GPU culled {st['chunks_culled']}, the model\n{p.describe()}"
    return st


@pytest.mark.parametrize("map_name", cs.MAP_NAMES)
@pytest.mark.parametrize("family", cs.FAMILIES)
def test_every_draw_culls_exactly_what_the_model_predicts(gpu_device, family, map_name):
    """one frame per draw, rank and world of the map; with culling off the count is 0"""
    gpu_device.set_binning(True)
    for name in SCENES_OF[family]:
        s = cs.scenes()[name]
        res = Resident(gpu_device, s.draws)
        try:
            for di in range(len(s.draws)):
                for cfg in cs.configs(s.all_ranks, map_name):
                    _check_draw(res, name, di, cfg)
                off = res.frame([di], *cs.configs(s.all_ranks, map_name)[-1], cull=False)
                assert off["chunks_culled"] == 0 and off["chunks"] == cm.predict(s.draws[di], W, H, None).chunks
        finally:
            res.close()


BINNING_CFGS = [("bands", 4, 1), ("supertiles4", 2, 0), (cs.WORLD1, 1, 0)]


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_the_count_does_not_depend_on_the_queue_builder(gpu_device, family):
    """the exact two-pass queues and the single-pass bounded ones: the same predicted count"""
    try:
        for name in SCENES_OF[family]:
            s = cs.scenes()[name]
            res = Resident(gpu_device, s.draws)
            try:
                for single_pass, binning in ((False, 2), (True, 1)):
                    gpu_device.set_binning(single_pass)
                    for di in range(len(s.draws)):
                        for cfg in BINNING_CFGS:
                            st = _check_draw(res, name, di, cfg, f" binning {binning}")
                            assert st["binning"] == binning
            finally:
                res.close()
    finally:
        gpu_device.set_binning(True)


SEQ_CFGS = [("bands", cs.D_WORLD, cs.D_RANK), ("bands", cs.D_WORLD, 0), ("bands", 2, 1)]


def _run_sequence(dev):
    """four frames with two straddlers, then one with 20, on one api.Batch: every frame's count"""
    from mt_renderer_amd import api
    few, many = cs.scenes()["d_sequence"].draws
    out = []
    model = api.Model.new(dev, few["md"])
    try:
        for cfg in SEQ_CFGS:
            batch = api.Batch(dev, model, few["model_mats"])
            try:
                for k, d in enumerate((few, few, few, few, many)):
                    batch.update(model_mats=d["model_mats"])
                    fr = api.Frame(dev, W, H)
                    fr.set_shard(*cs.shard_of(*cfg))
                    fr.draw_batch(batch, d["vp"])
                    fr.end()
                    st = fr.stats()
                    fr.close()
                    p = cm.predict(d, W, H, cs.shard_of(*cfg))
                    print(f"sequence {cfg} frame {k}: culled {st['chunks_culled']}, predicted {p.culled_lo}")
                    assert st["chunks"] == p.chunks
                    assert st["chunks_culled"] == p.culled_lo == p.culled_hi, f"frame {k} of the sequence as {cfg}: the GPU culled {st['chunks_culled']}, the model\n{p.describe()}"
                    out.append(st["chunks_culled"])
            finally:
                batch.close()
    finally:
        model.close()
    return out


def test_the_straddler_hint_sequence_is_predicted_frame_by_frame(gpu_device, monkeypatch):
    """k_cull_chunks sizes its rows by the straddlers a recent frame of the batch reported: after four frames with two
    of them the fifth has 20, more than the rows launched, and the kernel strides.  The same on a device whose geometry
    launch covers one instance slot at full rate (MTR_GEOM_SLOTS=1, read once at device creation)."""
    from mt_renderer_amd import api
    gpu_device.set_culling(api.GEOM_CULL_SHARDED)
    gpu_device.set_binning(True)
    ref = _run_sequence(gpu_device)
    monkeypatch.setenv("MTR_GEOM_SLOTS", "1")
    dev = api.Device(0)
    monkeypatch.delenv("MTR_GEOM_SLOTS")
    try:
        assert _run_sequence(dev) == ref
    finally:
        dev.close()


FRAME_CFGS = [("bands", 4, 1), ("bands-uneven", 4, 2), ("bands-uneven", 5, 4), ("supertiles1", 5, 4), ("supertiles4", 2, 0), (cs.WORLD1, 1, 0)]


@pytest.mark.parametrize("name", list(cs.scenes()))
def test_all_draws_in_one_frame_cull_the_sum_and_change_no_pixel(gpu_device, name):
    """all draws of a scene in one frame: the count is the sum of the per-draw predictions (every draw has its own
    offsets into the four culling buffers).  And soundness on the same frame: the pixels the rank owns, tris_setup and
    bin_entries are those of the frame rendered with culling off."""
    gpu_device.set_binning(True)
    s = cs.scenes()[name]
    res = Resident(gpu_device, s.draws)
    which = list(range(len(s.draws)))
    try:
        for cfg in FRAME_CFGS:
            shard = cs.shard_of(*cfg)
            preds = [cm.predict(d, W, H, shard) for d in s.draws]
            on = res.frame(which, *cfg, pixels=True)
            off = res.frame(which, *cfg, cull=False, pixels=True)
            want = sum(p.culled_lo for p in preds)
            print(f"{name} {cfg}: culled {on[2]['chunks_culled']} of {on[2]['chunks']}, predicted {want}")
            assert on[2]["chunks"] == sum(p.chunks for p in preds)
            assert on[2]["chunks_culled"] == want, (name, cfg, [p.culled_lo for p in preds])
            assert off[2]["chunks_culled"] == 0
            own = np.ones((H, W), dtype=bool) if shard is None else sharding.owner_map(W, H, shard[1], shard[2], shard[3], shard[4]) == shard[0]
            assert (on[0][own] == off[0][own]).all() and (on[1][own] == off[1][own]).all(), (name, cfg)
            assert on[2]["tris_setup"] == off[2]["tris_setup"] and on[2]["bin_entries"] == off[2]["bin_entries"], (name, cfg)
    finally:
        res.close()


# ---------------------------------------------------------------------------------------------
# the bound against the real vertex stage
# ---------------------------------------------------------------------------------------------
def _assert_inside(what, clip, boxes, M16, pal):
    s = cm.margin_fraction(clip, boxes, cm.mat4(M16), pal)
    if s is None:
        return 0.0  # an interval that is not finite: the chunk is kept, NaN outputs are allowed
    finite = np.isfinite(np.asarray(clip)[:, [0, 1, 3]]).all(axis=1)
    assert finite.all(), f"{what}: the model bounds the chunk, vertex {int(np.nonzero(~finite)[0][0])} is not finite"
    assert (s <= 1.0).all(), f"{what}: vertex {int(s.argmax())} lies {float(s.max()):.3f} margins outside the interval of its chunk"
    return float(s.max())


def test_the_interval_holds_for_the_vertex_stage_on_the_skinned_scenes(gpu_device):
    """every clip x, y, w that Model.vertex_stage returns for the skinned draws of family c lies inside the model's
    interval for each chunk the vertex belongs to"""
    from mt_renderer_amd import api
    worst = 0.0
    for di, d in enumerate(cs.scenes()["c_single"].draws):
        m = api.Model.new(gpu_device, d["md"])
        try:
            m.set_palette(d["palette"])
            b = cm.bounds(d["md"])
            base = 0
            for prim in range(d["md"].nprims):
                clip, _ = m.vertex_stage(prim, d["M"])
                ids = cm.chunk_vertex_ids(d["md"], prim)
                for k, vids in enumerate(ids):
                    ch = b.chunks[base + k]
                    if ch.whole is None or (ch.skinnable and ch.unbounded):
                        continue  # no box, too many joints for the table or weights that do not sum to 255: kept
                    boxes = ch.joints if ch.skinnable else [ch.whole]
                    worst = max(worst, _assert_inside(f"c_single draw {di} prim {prim} chunk {k}", clip[vids], boxes, d["M"], d["palette"] if ch.skinnable else None))
                base += len(ids)
        finally:
            m.close()
    print(f"largest |value - v| - rad of the vertex stage on the skinned scenes: {worst:.4f} m")


@pytest.mark.parametrize("name", [c.name for c in vx.cases()])
def test_the_interval_holds_for_the_vertex_stage_at_the_numeric_edges(gpu_device, name):
    """the cases of tests/vertex_edge_cases.py, vertices with normalised weights, in blocks of 62 + 2 vertex ids that
    stand in for chunks (the case models index three vertices only): cancellation, subnormals, signed zeros, joints past
    the palette.  NaN and inf outputs only where the interval itself is not finite."""
    from mt_renderer_amd import api
    c = next(c for c in vx.cases() if c.name == name)
    m = api.Model.new(gpu_device, c.md)
    worst = 0.0
    try:
        for npal in vx.NPALS:
            pal = vx.palette_of(c, npal)
            m.set_palette(pal)
            for prim in range(len(c.prims)):
                clip, _ = m.vertex_stage(prim, c.M)
                for vids, boxes in cm.case_blocks(c, prim, npal is not None):
                    worst = max(worst, _assert_inside(f"{name} npal {npal} prim {prim} vertices {vids[0]}..", clip[vids], boxes, c.M, pal))
    finally:
        m.close()
    print(f"{name}: largest |value - v| - rad of the vertex stage: {worst:.4f} m")
