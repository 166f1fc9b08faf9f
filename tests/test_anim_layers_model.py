"""CPU: the numpy model of SPEC.md section 16 (tests/anim_layers_model.py) on the inputs the GPU tests use.  Two layers with
mask 0 and OVERRIDE are section 14's / 15's cross-fade bit for bit; every deliberately wrong reading of the section shows on
the inputs; every layer step lies within the section's per-step bound of the same step in float64; all outputs are finite;
and an additive layer made by anim_layers.delta_clip reproduces its source clip."""
import numpy as np
import pytest

from mt_renderer_amd import anim_layers
from tests import anim_layers_model as lm
from tests import anim_model as am
from tests import anim_tracks_model as tm

F = np.float32


def _clips(kind, rng, J):
    return am.random_clips(rng, J) if kind == "uniform" else tm.random_track_clips(rng, J)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.mark.parametrize("J", [1, 64, 65])
def test_two_override_layers_are_the_cross_fade_of_section_14(J):
    rng = np.random.default_rng(16)
    clips = am.random_clips(rng, J)
    st = am.random_states(rng, 256, tm.STATE)
    got = lm.sample(clips, lm.crossfade_layers(st), J)
    assert (_bits(got) == _bits(am.sample(clips, st, J))).all()
    # with a mask set present as well: mask 0 is the built-in one
    assert (_bits(lm.sample(clips, lm.crossfade_layers(st), J, lm.random_masks(rng, J))) == _bits(got)).all()


@pytest.mark.parametrize("J", [1, 40])
def test_two_override_layers_are_the_cross_fade_of_section_15(J):
    rng = np.random.default_rng(16)
    clips = tm.random_track_clips(rng, J)
    st = tm.track_states(rng, clips, J)
    got = lm.sample(clips, lm.crossfade_layers(st), J)
    assert (_bits(got) == _bits(tm.sample(clips, st, J))).all()


def test_a_layer_with_e_zero_leaves_the_joint_untouched_and_its_clip_unread():
    J = 8
    rng = np.random.default_rng(3)
    clips = am.random_clips(rng, J)
    ly = lm.layer_states(rng, clips, n=64, L=2)
    ly["mask"][:, 1] = 1
    ly["w"][:, 1] = 0.7
    masks = np.zeros((1, J), dtype=F)
    masks[0, 3] = 0.5
    base = lm.sample(clips, ly[:, :1], J)
    got = lm.sample(clips, ly, J, masks)
    assert (_bits(got[:, np.arange(J) != 3]) == _bits(base[:, np.arange(J) != 3])).all()
    assert (_bits(got[:, 3]) != _bits(base[:, 3])).any()
    # not read: poisoning the layer's clips where e == 0 changes nothing (every clip is poisoned but joint 3)
    bad = [(k.copy(), fl) for k, fl in clips]
    ly["clip"][:, 0] = 0
    for k, _ in bad[1:]:
        k[:, np.arange(J) != 3] = np.nan
    ly["clip"][:, 1] = rng.integers(1, len(clips), 64)
    assert (_bits(lm.sample(bad, ly, J, masks)) == _bits(lm.sample(clips, ly, J, masks))).all()


@pytest.mark.parametrize("kind", ["uniform", "tracks"])
@pytest.mark.parametrize("L", [2, 4, 8])
def test_every_wrong_reading_shows_on_the_inputs(kind, L):
    J = 64
    rng = np.random.default_rng(16 + L)
    clips = _clips(kind, rng, J)
    masks = lm.random_masks(rng, J)
    ly = lm.layer_states(rng, clips, L=L)
    ref = lm.sample(clips, ly, J, masks)
    assert np.isfinite(ref).all()
    for v in lm.WRONG_VARIANTS:
        inst = float((_bits(lm.sample(clips, ly, J, masks, variant=v)) != _bits(ref)).any(axis=(1, 2)).mean())
        print(f"{kind}, L = {L}: {v} differs in {inst:.3f} of the instances")
        assert inst >= 0.10, f"{v} must be visible"


@pytest.mark.parametrize("kind", ["uniform", "tracks"])
@pytest.mark.parametrize("J,L", [(64, 2), (64, 4), (64, 8), (256, 8)])
def test_every_layer_step_lies_within_the_bound_of_the_exact_step(kind, J, L):
    """|binary32 step - float64 step| <= k u sum|terms| with k of lm.K_STEP (SPEC.md section 16), nlerp calls with |d| < 8 u
    left out (under 1 % of the calls)."""
    rng = np.random.default_rng(J + L)
    clips = _clips(kind, rng, J)
    masks = lm.random_masks(rng, J)
    ly = lm.layer_states(rng, clips, L=L)
    assert np.isfinite(lm.sample(clips, ly, J, masks)).all()
    res = lm.step_exact(clips, ly, J, masks)
    assert {r["kind"] for r in res} == {lm.OVERRIDE, lm.ADDITIVE}
    for r in res:
        print(f"{kind}, J = {J}, L = {L}, {'ADDITIVE' if r['kind'] else 'OVERRIDE'}: {r['calls']} nlerp calls, {r['left_out']} with |d| < 8 u "
              f"(min |d| {r['min_d']:.3e}); largest |binary32 - exact| / ({r['k']} u sum|terms|) = {r['frac']:.4f}")
        assert r["left_out"] < 0.01 * r["calls"]
        assert r["frac"] <= 1.0


def test_an_additive_layer_of_deltas_reproduces_its_source_clip():
    J = 64
    rng = np.random.default_rng(5)
    (keys, _), (other, _) = am.random_clips(rng, J, shape=[(31, 0), (1, 0)])
    ref = other[0]
    delta = anim_layers.delta_clip(keys, ref)
    assert delta.dtype == F and delta.shape == keys.shape
    # the inverse, in float64: the source clip up to the deltas' rounding to binary32 (rotations up to sign)
    back = anim_layers.apply(ref, delta)
    sign = np.sign((back[..., 4:8] * keys[..., 4:8]).sum(axis=-1, keepdims=True))
    assert np.abs(back[..., 0:3] - keys[..., 0:3]).max() <= 2 * 2.0 ** -24 * 20.0
    assert np.abs(back[..., 4:8] * sign - keys[..., 4:8]).max() <= 4 * 2.0 ** -24
    assert np.abs(back[..., 8:11] / keys[..., 8:11] - 1).max() <= 2 * 2.0 ** -24
    # through the model: the reference pose under an ADDITIVE layer at e = 1 is the source clip, to binary32 rounding
    clips = [(ref[None], 0), (delta, 0), (keys, 0)]
    n = 31
    ly = np.zeros((n, 2), dtype=lm.LAYER)
    ly["clip"][:, 1], ly["x"][:, 1], ly["w"][:, 1], ly["mode"][:, 1] = 1, np.arange(n), 1.0, lm.ADDITIVE
    T, Q, S = lm.sample_tqs(clips, ly, J)
    for i in range(3):
        assert np.abs(T[i] - keys[..., i]).max() <= 4 * 2.0 ** -24 * 20.0
        assert np.abs(S[i] / keys[..., 8 + i] - 1).max() <= 8 * 2.0 ** -24
    q = np.stack(Q, axis=-1).astype(np.float64)
    sign = np.sign((q * keys[..., 4:8]).sum(axis=-1, keepdims=True))
    assert np.abs(q * sign - keys[..., 4:8]).max() <= 16 * 2.0 ** -24
