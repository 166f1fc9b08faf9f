"""CPU: the premises of tests/test_gpu_vis_waves.py -- that each scene of tests/vis_wave_scenes.py puts its content into the
passes, and so (in queues that keep the submission order) before the wave and the iteration, its docstring names -- computed from the
scenes' integers at 2, 4 and 8 waves per bin; and the integer model against the oracle: every triangle is set up, and the
pixels the model says are covered are exactly those whose depth the oracle wrote.

The oracle frames are kept in FRAMES, so the GPU file (same process, same scenes) renders none of them a second time."""
import numpy as np
import pytest

from tests import tile_path_scenes as tp
from tests import vis_wave_scenes as vs
from tests.helpers import render_oracle

FRAMES = {}
BUILDERS = {
    "pipeline_edges": vs.pipeline_edges,
    "walks_per_iteration": vs.walks_per_iteration,
    "big_boxes_second_iteration": vs.big_boxes_second_iteration,
    "lists_from_every_wave": vs.lists_from_every_wave,
    "list_overflow_across_waves": vs.list_overflow_across_waves,
    "dominated_across_waves": vs.dominated_across_waves,
}


def frame(name, W, *args, h=None, clear_depth=1.0):
    """(scene, draws, oracle frame) of a scene, built and rendered once per process"""
    key = (name, W, args, h, clear_depth)
    if key not in FRAMES:
        if name == "resolve_pairs":
            sc = vs.resolve_pairs(*args)
        else:
            sc = BUILDERS[name](W, *args, **({} if h is None else {"h": h}))
        draws = sc.draws()
        FRAMES[key] = (sc, draws, render_oracle(sc.w, sc.h, draws, clear_depth=clear_depth))
    return FRAMES[key]


def cases(W):
    """(name, args) of every scene that is built for W waves"""
    out = [("pipeline_edges", (N,)) for N in vs.pipeline_edge_sizes(W)]
    out += [("walks_per_iteration", (wave, first)) for wave in (0, W - 1) for first in range(3)]
    out += [("big_boxes_second_iteration", (64,)), ("big_boxes_second_iteration", (31,)), ("big_boxes_second_iteration", (31, "split"))]
    out += [("lists_from_every_wave", ()), ("list_overflow_across_waves", (9,)), ("list_overflow_across_waves", (12,)), ("dominated_across_waves", ())]
    return out


def case_id(c):
    return "-".join([c[0]] + [str(a) for a in c[1]])


RESOLVE_CASES = [(w, h, mixed) for w, h in vs.RESOLVE_TARGETS for mixed in (False, True)]


def in_order(sc):
    """the bin under test holds every triangle of the scene, in submission order: entry i is triangle i, pass i div 64"""
    e = sc.bin_entries()
    assert len(e) == len(sc.tris) and all(a is b for a, b in zip(e, sc.tris))
    return {id(t): i for i, t in enumerate(e)}


def premise_pipeline_edges(sc, W, N):
    S = 64 * W
    assert N in (1, 65, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 1) and N <= 1537
    idx = in_order(sc)
    assert len(idx) == N
    assert all(1 <= len(t.pixels(sc.w, sc.h)) <= 3 and not t.large for t in sc.tris)
    hits = sc.bin_hits()
    npass = (N + 63) // 64
    # every (wave, iteration) that exists at this N holds some pixel's winner
    won = {idx[id(vs.winner(v))] // 64 for v in hits.values()}
    assert won == set(range(npass))
    assert {vs.pass_of(W, k) for k in won} == {(w, i) for w in range(W) for i in range((N + S - 1) // S) if (i * W + w) * 64 < N}
    # ties for a pixel's smallest z, between passes of two waves and between two iterations of one wave; the tied triangles
    # differ in colour, so taking the earlier one shows
    two_waves = two_iterations = False
    for v in hits.values():
        w = vs.winner(v)
        for t in v:
            if t is not w and t.z == w.z and t.cid != w.cid:
                (wa, ia), (wb, ib) = vs.pass_of(W, idx[id(t)] // 64), vs.pass_of(W, idx[id(w)] // 64)
                two_waves |= wa != wb
                two_iterations |= wa == wb and ia != ib
    assert two_waves == (N >= 65) and two_iterations == (N > S)
    zs = [t.z for t in sc.tris]
    assert N < 3 or (len(set(zs)) < len(zs) and zs != sorted(zs) and zs != sorted(zs, reverse=True))
    # the partial last pass and the wave it lands on; the waves that own no pass
    last = vs.pass_of(W, npass - 1)
    idle = [w for w in range(W) if w * 64 >= N]
    if N == 1:
        assert idle == list(range(1, W)) and last == (0, 0)
    if N == 65:
        assert idle == list(range(2, W)) and last == (1, 0) and N - 64 == 1
    if N % 64 == 1 and N > 65:
        assert last == (0, N // S) and idle == []  # a pass of one entry, wave 0's second, third or fourth iteration
    if N == S - 1:
        assert last == (W - 1, 0) and N % 64 == 63  # the partial pass lands on the last wave
    return dict(passes=npass, idle_waves=idle, last_pass=last)


def walk_of(sc, entries):
    """the `spans` rule of k_tile_vis.hip: of the i32-class triangles with a box in the bin, are those over four pixels half?"""
    cand = [t for t in entries if not t.large and sc.box_pixels(t, sc.bx, sc.by) > 0]
    over4 = sum(sc.box_pixels(t, sc.bx, sc.by) > 4 for t in cand)
    return ("span" if cand and over4 * 2 >= len(cand) else "pair"), over4, len(cand)


def premise_walks_per_iteration(sc, W, wave, first):
    assert wave in (0, W - 1) and first in (0, 1, 2)
    idx = in_order(sc)
    ps = sc.passes(sc.bx, sc.by)
    kinds = vs.walk_passes(W, wave, first)
    assert sorted(kinds) == [wave, wave + W, wave + 2 * W] and len(ps) == wave + 2 * W + 1 and all(len(p) == 64 for p in ps)
    assert [vs.pass_of(W, k) for k in sorted(kinds)] == [(wave, 0), (wave, 1), (wave, 2)]
    assert [kinds[k] for k in sorted(kinds)][0] == vs.WALK_KINDS[first] and sorted(kinds.values()) == sorted(vs.WALK_KINDS)
    hits = sc.bin_hits()
    won = {idx[id(vs.winner(v))] // 64 for v in hits.values()}
    for k, p in enumerate(ps):
        walk, over4, ncand = walk_of(sc, p)
        if k not in kinds:
            assert not any(t.large for t in p) and all(sc.box_pixels(t, sc.bx, sc.by) == 1 for t in p) and walk == "pair"
            continue
        assert [t.large for t in p] == [False] * 31 + [True] + [False] * 32 and ncand == 63
        assert all(sc.box_pixels(t, sc.bx, sc.by) == 1 or sc.box_pixels(t, sc.bx, sc.by) >= 9 for t in p if not t.large)
        assert (walk, over4) == {"span": ("span", vs.SPAN_PASS), "pair": ("pair", vs.PAIR_PASS), "large": ("pair", 0)}[kinds[k]]
        big = p[31]
        assert max(big.X) - min(big.X) > tp.CLASS_LIMIT
        assert len([q for q in big.pixels(sc.w, sc.h) if q[0] // tp.BIN == sc.bx]) > 128
        assert k in won  # the pass shows in the frame
    return dict(passes=len(ps), walks={k: kinds[k] for k in sorted(kinds)})


def pair_walk_rounds(box):
    """the round of each candidate of a pair-walk pass: a round stages the longest prefix of the remaining candidates whose
    box pixels sum to 4096 at the most (k_tile_vis.hip: `take = cand && inc <= 4096`)"""
    out, r, acc = [], 0, 0
    for b in box:
        if acc + b > 4096:
            r, acc = r + 1, 0
        acc += b
        out.append(r)
    return out


def premise_big_boxes(sc, W, nfill, layout="front"):
    idx = in_order(sc)
    ps = sc.passes(sc.bx, sc.by)
    assert [len(p) for p in ps] == [64] * (W + 1) + [7] and vs.pass_of(W, W) == (0, 1)
    assert not any(t.large for t in sc.tris)
    for k, p in enumerate(ps):
        if k != W:
            assert all(sc.box_pixels(t, sc.bx, sc.by) == 1 for t in p)
    box = [sc.box_pixels(t, sc.bx, sc.by) for t in ps[W]]
    bigs = [i for i, b in enumerate(box) if b == 256]
    assert sorted(box) == [1] * (64 - nfill) + [256] * nfill
    walk, over4, ncand = walk_of(sc, ps[W])
    pairs, rows = sum(box), 16 * nfill + (64 - nfill)
    rnd = pair_walk_rounds(box)
    rounds = rnd[-1] + 1
    hits = sc.bin_hits()
    won = {idx[id(vs.winner(v))] - 64 * W for v in hits.values() if idx[id(vs.winner(v))] // 64 == W}
    if nfill == 64:
        # 64 boxes over four pixels of 64 candidates: by the `spans` rule this pass takes the SPAN walk, at its bound of 64 x 16
        # rows.  (Its 16384 pairs would be four rounds of the pair walk, which no pass reaches: see below.)
        assert (walk, over4, ncand, pairs, rows, rounds) == ("span", 64, 64, 16384, 1024, 4) and layout == "front"
        assert {k // 16 for k in won} == {0, 1, 2, 3}  # winners from every sixteen of the pass
    else:
        # the pair walk needs fewer than half of the candidates over four pixels: 31 of 64 at the most, so a pass holds at most
        # 31 x 256 + 33 x 4 = 8068 pairs.  A round that is not the last was closed by a box that did not fit, of 256 pixels at the
        # most, so it holds 4096 - 255 = 3841 pairs or more; three such rounds would be 11523.  So: three rounds at the most --
        # two closed ones and the rest -- and the split layout (15 big + 1 small = 3841, twice, then the rest) needs them
        assert (walk, over4, ncand, pairs) == ("pair", 31, 64, 31 * 256 + 33) and 2 * (nfill + 1) >= 64
        assert rounds == {"front": 2, "split": 3}[layout]
        if layout == "split":
            assert [box[:16], box[16:32], box[32:]] == [[256] * 15 + [1], [256] * 15 + [1], [256] + [1] * 31]
            assert [rnd[:16], rnd[16:32], rnd[32:]] == [[0] * 16, [1] * 16, [2] * 32]
            assert sum(box[:16]) == sum(box[16:32]) == 3841 and 3841 + 256 > 4096
        assert {rnd[k] for k in won if box[k] == 256} == set(range(rounds))  # a big triangle of every round wins pixels
        assert {rnd[k] for k in won if box[k] == 1} >= {rounds - 1}          # and so do one-pixel ones of the last round
    # the big triangles come nearer in turn, but for one run of equal depths: a winner ties with an earlier winner-to-be of
    # another colour -- and, in the pair-walk layouts that have the tie, of another round
    zs = [ps[W][i].z for i in bigs]
    assert all(b <= a for a, b in zip(zs, zs[1:]))
    assert sum(a == b for a, b in zip(zs, zs[1:])) == (0 if (nfill, layout) == (31, "front") else 4)
    if (nfill, layout) != (31, "front"):
        late = bigs[30] if layout == "split" else bigs[34]
        early = bigs[26] if layout == "split" else bigs[30]
        a, b = ps[W][early], ps[W][late]
        assert a.z == b.z and a.cid != b.cid and any(vs.winner(v) is b and a in v for v in hits.values())
        assert layout == "front" or rnd[early] != rnd[late]
    return dict(walk=walk, pairs=pairs, rows=rows, pair_rounds=rounds)


def q_fragments(sc):
    hits = sc.bin_hits()
    return hits, hits[(vs.QX, vs.QY)]


def premise_list_scene(sc, W, nfrag):
    """what the three order-list scenes share: fragment k of pixel Q lies in pass k, the filler stays within the lists"""
    idx = in_order(sc)
    hits, q = q_fragments(sc)
    assert len(q) == nfrag and [idx[id(t)] // 64 for t in q] == list(range(nfrag))
    assert all(t.mat == "trans" and len(t.pixels(sc.w, sc.h)) == 1 for t in q)
    assert sum(t.mat is None for t in sc.tris) == 1 and all(t.mat in (None, "trans") for t in sc.tris) and sc.mixed
    others = [v for p, v in hits.items() if p != (vs.QX, vs.QY)]
    assert len(others) == 255 and max(len(v) for v in others) <= (2 if nfrag <= 9 else 3) <= tp.STAIR_K
    second = [(v[1].z > v[0].z) - (v[1].z < v[0].z) for v in others if len(v) > 1]
    assert {-1, 0, 1} <= set(second)  # a second fragment nearer than, level with and farther than the first
    where = [vs.pass_of(W, k) for k in range(nfrag)]
    assert {w for w, _ in where} == set(range(min(W, nfrag))) and {i for _, i in where} == set(range((nfrag + W - 1) // W))
    return q, where


def premise_lists_from_every_wave(sc, W):
    q, where = premise_list_scene(sc, W, tp.STAIR_K)
    # none is dominated by an earlier one (that needs an earlier, STRICTLY nearer fragment), so all are listed whatever the
    # timing: exactly STAIR_K, no overflow, the bin resolves from its lists
    assert all(b.z < a.z for a, b in zip(q, q[1:])) and len(q) == tp.STAIR_K == 8
    return dict(fragments=where)


def premise_list_overflow(sc, W, nfrag):
    q, where = premise_list_scene(sc, W, nfrag)
    assert all(b.z < a.z for a, b in zip(q, q[1:])) and len(q) > tp.STAIR_K  # all listed: the bin goes to the ordered kernel
    return dict(fragments=where)


def premise_dominated(sc, W):
    q, where = premise_list_scene(sc, W, 12)
    assert all(b.z > a.z for a, b in zip(q, q[1:]))
    # each of fragments 1..11 is dominated by fragment 0 if a key of fragment 0 (or of a nearer, earlier one: there is none)
    # was in place when it arrived: between 1 fragment listed (all saw fragment 0) and 12 (none did: over STAIR_K, the bin
    # then goes to the ordered kernel).  The pixel is fragment 0 over the clear colour either way: the others fail the test
    return dict(listed=(1, 12), fragments=where)


def pixel_kind(sc, v):
    if not v:
        return "clear"
    assert all(b.z <= a.z for a, b in zip(v, v[1:]))  # nothing dominated: a list is as long as the pixel's fragments are many
    if len(v) == 1 and v[0].mat != "trans":
        return "solid" if v[0].mat is None else v[0].mat
    assert all(t.mat == "trans" for t in v)
    return "list%d" % len(v)


def premise_resolve_pairs(sc, w, h, mixed):
    in_order(sc)
    assert (sc.bx, sc.by) == (1, 0) and sc.mixed == mixed and sc.textured
    hits = sc.bin_hits()
    vw, vh = min(tp.BIN, w - tp.BIN), min(tp.BIN, h)
    cut = (w, h) == (24, 12)
    assert (vw < tp.BIN and vh < tp.BIN) == cut
    kinds = vs.RESOLVE_KINDS[mixed]
    pairs, below = set(), set()
    for ly in range(8):
        for lx in range(vw):  # thread t = ly * 16 + lx of the 128 resolves pixel t and pixel t + 128 = (lx, ly + 8)
            a = pixel_kind(sc, hits.get((tp.BIN + lx, ly), []))
            if ly + 8 < vh:
                pairs.add((a, pixel_kind(sc, hits.get((tp.BIN + lx, ly + 8), []))))
            else:
                below.add(a)
    assert pairs == {(a, b) for a in kinds for b in kinds}
    if mixed:
        assert ("list8", "clear") in pairs and ("clear", "list8") in pairs
        assert any(len(v) == 4 and v[1].z == v[2].z for v in hits.values())  # level fragments: both pass LessEqual
    assert below == (set(kinds) if cut else set())  # the second pixel of the pair lies below the viewport
    return dict(pairs=len(pairs), first_only=sorted(below))


def check_premise(name, sc, W, *args):
    if name == "pipeline_edges":
        return premise_pipeline_edges(sc, W, *args)
    if name == "walks_per_iteration":
        return premise_walks_per_iteration(sc, W, *args)
    if name == "big_boxes_second_iteration":
        return premise_big_boxes(sc, W, *args)
    if name == "lists_from_every_wave":
        return premise_lists_from_every_wave(sc, W)
    if name == "list_overflow_across_waves":
        return premise_list_overflow(sc, W, *args)
    if name == "dominated_across_waves":
        return premise_dominated(sc, W)
    assert name == "resolve_pairs"
    return premise_resolve_pairs(sc, *args)


def model_against_oracle(sc, ref):
    color, depth, stats = ref
    assert sc.w <= 128 and sc.h <= 32
    assert stats["tris_setup"] == len(sc.tris)
    assert ((depth < 1.0) == sc.covered()).all()
    assert len(np.unique(color.reshape(-1, 4), axis=0)) > 3


ALL = [(W, c) for W in vs.WAVES for c in cases(W)]


@pytest.mark.parametrize("W,case", ALL, ids=["w%d-%s" % (W, case_id(c)) for W, c in ALL])
def test_premise_and_model(W, case):
    name, args = case
    sc, draws, ref = frame(name, W, *args)
    check_premise(name, sc, W, *args)
    if not (name == "pipeline_edges" and args[0] == 1):
        model_against_oracle(sc, ref)
    else:
        assert ref[2]["tris_setup"] == 1 and ((ref[1] < 1.0) == sc.covered()).all()


@pytest.mark.parametrize("w,h,mixed", RESOLVE_CASES, ids=["%dx%d-%s" % (w, h, "mixed" if m else "opaque") for w, h, m in RESOLVE_CASES])
def test_resolve_pairs_premise_and_model(w, h, mixed):
    sc, draws, ref = frame("resolve_pairs", 2, w, h, mixed)
    check_premise("resolve_pairs", sc, 2, w, h, mixed)
    model_against_oracle(sc, ref)


@pytest.mark.parametrize("W", vs.WAVES)
def test_dominated_pixel_is_its_first_fragment_over_the_clear_colour(W):
    sc, draws, ref = frame("dominated_across_waves", W)
    _, q = q_fragments(sc)
    opaque = [t for t in sc.tris if t.mat is None]
    alone = vs.WaveScene(sc.w, sc.h, [q[0]] + opaque)
    one = render_oracle(alone.w, alone.h, alone.draws())
    assert (ref[0][vs.QY, vs.QX] == one[0][vs.QY, vs.QX]).all() and (ref[0][vs.QY, vs.QX] != 255).any()
    assert ref[1][vs.QY, vs.QX] == one[1][vs.QY, vs.QX] == np.float32(float(q[0].z))


@pytest.mark.parametrize("W", vs.WAVES)
def test_two_bin_rows_hold_the_same_bin(W):
    """the scenes of the band-shard test on a 128 x 32 target: the bin under test is unchanged, the second row is empty"""
    for name, args in (("pipeline_edges", (3 * 64 * W + 1,)), ("lists_from_every_wave", ())):
        sc, draws, ref = frame(name, W, *args, h=32)
        check_premise(name, sc, W, *args)
        model_against_oracle(sc, ref)
        assert sc.h == 32 and (ref[1][16:] == 1.0).all()


@pytest.mark.parametrize("W", vs.WAVES)
def test_clear_depths_of_the_gpu_file(W):
    """pipeline_edges(W, 2S + 1) under a clear depth of 0.5 (zlim below 1): some of its pixels still pass, some now fail;
    under -1 (zlim_ok false) nothing passes and the frame is the clear colour and the clear depth"""
    N = 2 * 64 * W + 1
    full, half, none = (frame("pipeline_edges", W, N, clear_depth=cd)[2] for cd in (1.0, 0.5, -1.0))
    assert 0 < int((half[1] < 0.5).sum()) < int((full[1] < 1.0).sum())
    assert ((half[1] < 0.5) == (full[1] <= 0.5)).all() and (half[1][full[1] > 0.5] == 0.5).all()
    assert (none[1] == np.float32(-1.0)).all() and (none[0] == 255).all() and none[2]["tris_setup"] == N
