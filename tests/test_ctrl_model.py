"""CPU: the stated consequences of SPEC.md section 21 (controllers) on the numpy model (tests/ctrl_model.py) chained with the
player model (tests/player_model.py): 200 frames of 64 instances of a locomotion graph -- idle, walk and run on speed thresholds
with hysteresis, walk <-> run with SYNC, an any-state jump on a trigger parameter with INTERRUPT and CONSUME that returns on
ENDED.  And the generator's census: every branch is reached in at least three cases and every wrong reading changes one."""
import numpy as np
import pytest

from tests import ctrl_model as cm
from tests import player_model as pm

F = np.float32
N, FRAMES = 64, 200
TAB = cm.LOCO_TAB


def start(n=N):
    st, play = np.zeros(n, dtype=cm.STATE), np.zeros(n, dtype=pm.PLAY)
    st["user"] = np.arange(n) * 2654435761 % (1 << 32)
    play["speed"] = 1.0
    play["x_a"] = np.linspace(0, 29, n).astype(F)
    return st, play


def simulate(g, drive, frames=FRAMES, n=N):
    """the chain step -> advance for `frames` frames; drive(frame, params) edits the parameters before each step.  Returns the
    per-frame records: play and params before the step, states, commands and play after, the player's trace, the counts."""
    st, play = start(n)
    params = np.zeros((n, g["nparams"]), dtype=F)
    counts = np.zeros(len(g["trans"]), dtype=np.uint32)
    rec = []
    for f in range(frames):
        drive(f, params)
        before, given = play, params.copy()
        st, params, cmds, counts = cm.step(g, TAB, st, play, params, pm.DT, counts)
        tr = []
        play = pm.advance(play, pm.DT, TAB, cmds, trace=tr)[0]
        rec.append(dict(before=before, given=given, states=st, params=params.copy(), cmds=cmds, play=play, trace=tr[0]))
    return rec, counts


def crowd(seed, triggers=True):
    """speeds that wander across the thresholds, and now and then a trigger"""
    rng = np.random.default_rng(seed)
    speed = rng.uniform(0, 3, N).astype(F)

    def drive(f, params):
        speed[:] = np.clip(speed + rng.normal(0, 0.15, N).astype(F), 0, 3)
        params[:, cm.SPEED] = speed
        if triggers:
            params[rng.random(N) < 0.01, cm.TRIGGER] = 1.0
    return drive


_RUNS = {}


def run(interrupt):
    if interrupt not in _RUNS:
        _RUNS[interrupt] = simulate(cm.locomotion(interrupt), crowd(7))
    return _RUNS[interrupt]


def test_no_transition_passing_leaves_the_player_alone():
    def drive(f, params):
        params[:, cm.SPEED] = 0.5  # between the thresholds of idle
    rec, counts = simulate(cm.locomotion(), drive)
    _, play = start()
    for r in rec:
        play = pm.advance(play, pm.DT, TAB, None)[0]
        assert (r["cmds"]["instance"] == cm.NONE).all() and (r["states"]["fired"] == cm.NONE).all()
        assert pm.same_bits(r["play"], play).all()
    assert counts.sum() == 0 and (rec[-1]["states"]["node"] == cm.IDLE).all()
    # t has counted the frames in binary32, and user is kept
    t = F(0)
    for _ in range(FRAMES):
        t = F(t + F(pm.DT))
    assert (rec[-1]["states"]["t"] == t).all() and (rec[-1]["states"]["user"] == start()[0]["user"]).all()


def test_a_trigger_set_once_fires_exactly_once():
    who = np.arange(0, N, 5)

    def drive(f, params):
        params[:, cm.SPEED] = 0.5
        if f == 10:
            params[who, cm.TRIGGER] = 1.0
    rec, counts = simulate(cm.locomotion(), drive)
    fires = np.zeros(N, dtype=np.int64)
    for r in rec:
        fires += r["states"]["fired"] == 0
    assert (fires[who] == 1).all() and fires.sum() == len(who) and counts[0] == len(who)
    assert (rec[10]["states"]["fired"][who] == 0).all() and (rec[10]["params"][:, cm.TRIGGER] == 0).all()
    assert (rec[10]["cmds"][who] == np.array([(i, cm.JUMP, 0.0, 0.0) for i in who], dtype=pm.CMD)).all()


def test_without_interrupt_no_fade_is_interrupted():
    rec, _ = run(False)
    fired = fades = 0
    for r in rec:
        has = r["states"]["fired"] != cm.NONE
        assert not (has & (r["before"]["fade"] > 0)).any(), "a transition fired while a fade ran"
        assert not (r["trace"]["above"] | r["trace"]["below"]).any(), "a fade was interrupted"
        fired += int(has.sum())
        fades += int(r["trace"]["fade_start"].sum())
    assert fired > N and fades > N
    # with INTERRUPT the jump does cut into running fades: the contrast
    assert any(((r["states"]["fired"] == 0) & (r["before"]["fade"] > 0)).any() for r in run(True)[0])


def test_sync_between_32_and_16_keys_keeps_the_phase():
    P = {cm.WALK: F(32), cm.RUN: F(16)}
    seen = {3: 0, 4: 0}
    for r in run(True)[0]:
        for idx, (src, dst) in ((3, (cm.WALK, cm.RUN)), (4, (cm.RUN, cm.WALK))):
            m = r["states"]["fired"] == idx
            if not m.any():
                continue
            b = r["before"][m]
            assert (b["fade"] == 0).all() and (b["clip_a"] == src).all()
            assert ((r["cmds"]["x"][m] / P[dst]).view("<u4") == (b["x_a"] / P[src]).view("<u4")).all(), "the phase moved"
            assert (r["cmds"]["clip"][m] == dst).all()
            seen[idx] += int(m.sum())
    assert seen[3] > 0 and seen[4] > 0


def test_the_jump_returns_in_the_step_after_the_clamp():
    rec, _ = run(True)
    returns = 0
    for f in range(1, FRAMES):
        r, prev = rec[f], rec[f - 1]
        m = r["states"]["fired"] == 5
        b = r["before"]
        at_end = (prev["states"]["node"] == cm.JUMP) & (b["fade"] == 0) & (b["clip_a"] == cm.JUMP) & ((b["flags"] & pm.ENDED) != 0)
        # it fires exactly where the node is jump and the player has clamped the clip at its end ...
        assert (m == at_end).all()
        # ... which the advance of the frame before did: one step earlier the clip was still running
        pb = prev["before"][m]
        assert not (((pb["flags"] & pm.ENDED) != 0) & (pb["clip_a"] == cm.JUMP) & (pb["fade"] == 0)).any()
        assert (prev["trace"]["end_clamp"][m] | (b["x_a"][m] == 11)).all()
        returns += int(m.sum())
    assert returns > 5


def test_counts_equal_the_fired_words_seen():
    for interrupt in (True, False):
        rec, counts = run(interrupt)
        seen = np.zeros(len(counts), dtype=np.int64)
        for r in rec:
            f = r["states"]["fired"]
            np.add.at(seen, f[f != cm.NONE], 1)
        assert (seen == counts).all() and counts.sum() > N


def test_the_generator_reaches_every_branch_and_tells_every_wrong_reading():
    reach, changed = cm.census()
    assert len(cm.cases()) == 48 and len(cm.WRONG_VARIANTS) >= 8
    assert {c["n"] for c in cm.cases()} == {1, 5, 63, 64, 65, 257} and {c["graph"]["nparams"] for c in cm.cases()} == {0, 1, 5, 16}
    for k in cm.BRANCHES:
        assert reach[k] >= 3, f"{k} is reached in {reach[k]} cases"
    assert reach["p0_phase"] >= 1 and reach["p0_sync"] >= 1, "P_l = 0 under PHASE and under SYNC"
    for v in cm.WRONG_VARIANTS:
        assert changed[v] >= 1, f"{v} changes no case"
    # the figures SPEC.md section 21 records
    assert reach == dict(fire_any=24, fire_own=27, skip_fade=27, skip_self=21, interrupt=32, sync=37, consume=13, no_fire=42, p0_phase=2, p0_sync=5)
    assert changed == dict(last_passes=39, own_first=23, lead_a=27, t_first=4, t_kept=41, ne_nan_false=8, consume_evaluated=15, sync_ratio=26,
                           dtp_keeps_neg_zero=4)


def test_the_generator_holds_every_special_value():
    """parameters, t, x, fade and dt of NaN, +-inf, -0 and denormals, each in some case"""
    tiny = lambda a: ((np.abs(a) > 0) & (np.abs(a) < np.finfo(F).tiny)).any()
    negz = lambda a: ((a == 0) & np.signbit(a)).any()
    kinds = dict(nan=lambda a: np.isnan(a).any(), pinf=lambda a: (a == np.inf).any(), ninf=lambda a: (a == -np.inf).any(), negzero=negz, denormal=tiny)
    fields = dict(params=lambda c: c["params"], t=lambda c: c["states"]["t"], x_a=lambda c: c["play"]["x_a"], x_b=lambda c: c["play"]["x_b"],
                  fade=lambda c: c["play"]["fade"], dt=lambda c: np.array(c["dts"], dtype=F))
    for fname, get in fields.items():
        for kname, has in kinds.items():
            assert any(has(np.asarray(get(c), dtype=F)) for c in cm.cases() if np.asarray(get(c)).size), f"no {kname} in {fname}"
    # a denormal fade leads (it runs only where denormals are kept), and dt = -0 meets t = -0 where nothing fires
    assert any(((c["play"]["fade"] > 0) & (c["play"]["fade"] < np.finfo(F).tiny)).any() for c in cm.cases())
    assert any(negz(np.array(c["dts"][:1], dtype=F)) and negz(c["states"]["t"]) for c in cm.cases())


def test_every_bit_pattern_has_an_outcome():
    """nodes and clips past the tables are clamped before they index anything, and a step reads no play state field it may not"""
    for c in cm.cases():
        g = c["graph"]
        st, pr, cmds, _ = cm.step(g, c["tab"], c["states"], c["play"], c["params"], c["dts"][0])
        assert (st["node"] < len(g["nodes"])).all() and (st["user"] == c["states"]["user"]).all()
        has = st["fired"] != cm.NONE
        assert (cmds["instance"][has] == np.arange(c["n"])[has]).all() and (cmds["instance"][~has] == cm.NONE).all()
        assert (cmds["clip"] < len(c["tab"][0])).all() and (st["fired"][has] < len(g["trans"])).all()
