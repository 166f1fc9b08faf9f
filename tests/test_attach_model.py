"""CPU: properties of the numpy model of attachments (tests/attach_model.py, SPEC.md section 18) that need no GPU: the binary32
model stays within the section's bound of its float64 version; each deliberately wrong reading changes at least one record of
every generated case where it can show; attach.bind_offsets puts an object given relative to a joint where a float64 fold of
the skeleton puts it."""
import numpy as np
import pytest

from mt_renderer_amd.attach import bind_offsets
from tests import attach_model as am

CASES = am.cases()


def _finite_normal(case):
    """records whose offset has only zeros and normal finite numbers: the bound's premise (no underflow, no special value)"""
    o = case["recs"]["offset"]
    ok = np.isfinite(o) & ((o == 0) | (np.abs(o) >= np.finfo(np.float32).tiny)) & (np.abs(o) < 1e30)
    return ok.all(axis=1)


def test_generator_covers_the_plan():
    assert len(CASES) == len(am.N_SRC) * len(am.NPAL) * len(am.COUNTS)
    r = np.concatenate([c["recs"] for c in CASES if c["npal"] == 64 and c["n_src"] == 7])
    assert (r["src_instance"] >= 7).any() and (r["joint"] == am.NO_JOINT).any() and ((r["joint"] >= 64) & (r["joint"] != am.NO_JOINT)).any()
    assert (r["joint"] == 64).any(), "a joint index of exactly npal tells the clamp to npal from the clamp to npal - 1"
    assert ((r["flags"] & 1 == 1) & (r["flags"] >> 1 != 0)).any() and ((r["flags"] & 1 == 0) & (r["flags"] >> 1 != 0)).any()
    assert (r["flags"] == 1).any() and (r["flags"] == 0).any() and (r["pad"] != 0).any()
    o = r["offset"]
    assert np.isnan(o).any() and np.isinf(o).any() and ((o != 0) & (np.abs(o) < np.finfo(np.float32).tiny)).any()


def test_binary32_model_within_the_bound_of_float64():
    worst = 0.0
    for c in CASES:
        got = am.attach(c["M_src"], c["P_src"], c["recs"]).astype(np.float64)
        want = am.attach(c["M_src"], c["P_src"], c["recs"], dt=np.float64)
        b = am.bound(c["M_src"], c["P_src"], c["recs"])
        ok = _finite_normal(c)
        assert ok.sum() >= c["n"] - len(am.SPECIALS)
        with np.errstate(invalid="ignore"):
            err = np.abs(got - want)[ok]
        assert (err <= b[ok]).all(), c["name"]
        worst = max(worst, float((err / np.maximum(b[ok], 1e-300)).max()))
    print(f"largest fraction of the bound reached: {worst:.3f}")
    assert worst <= 1.0
    assert worst > 0.02, "a bound never approached would say nothing about the arithmetic"


# exemptions (am.can_show): a wrong reading is only asked to show where the case holds a record it can change
#   pal_left, assoc_right, clamp_npal, pos_from_msrc need a record with a joint (npal == 0 cases have none);
#   assoc_right needs one that is not position-only (A is replaced there, there is no second association);
#   clamp_npal needs a joint index >= npal and a source with more than one palette matrix to read instead;
#   pos_from_msrc needs a position-only record with a joint; flags_upper one with bit 0 set under junk bits.
@pytest.mark.parametrize("variant", am.WRONG_VARIANTS)
def test_wrong_readings_are_told_apart(variant):
    shown = changed = total = 0
    for c in CASES:
        if not am.can_show(variant, c):
            continue
        right = am.attach(c["M_src"], c["P_src"], c["recs"])
        wrong = am.attach(c["M_src"], c["P_src"], c["recs"], variant=variant)
        diff = ~am.same_bits(right, wrong).all(axis=1)
        assert diff.any(), f"{variant} changes no record of {c['name']}"
        shown += 1
        changed += int(diff.sum())
        total += c["n"]
    print(f"{variant}: {shown} of {len(CASES)} cases, {changed} of {total} records changed ({100.0 * changed / total:.0f} %)")
    assert shown >= len(CASES) // 4


def _fold_case(rng, J=24, n=40):
    """a skeleton of J joints (a chain with side branches), bind and animated locals, and n placements relative to joints"""
    parents = np.array([255] + [int(rng.integers(max(0, j - 3), j)) for j in range(1, J)])
    bind, pose = am.trs(rng, J, 1.0).astype(np.float64), am.trs(rng, J, 1.0).astype(np.float64)
    m = lambda a: a.reshape(-1, 4, 4).transpose(0, 2, 1)  # column-major [n, 16] -> mathematical [n][row][column]

    def worlds(loc):
        w = [None] * J
        for j in range(J):
            w[j] = loc[j] if parents[j] == 255 else w[parents[j]] @ loc[j]
        return np.stack(w)
    wb, wp = worlds(m(bind)), worlds(m(pose))
    imats = np.linalg.inv(wb).transpose(0, 2, 1).reshape(J, 16).astype(np.float32)  # what the model file would hold
    joints = rng.integers(0, J, size=n)
    local = am.trs(rng, n, 0.5)
    return imats, wp, joints, local, m


def test_bind_offsets_put_the_object_where_the_fold_puts_it():
    # measured over the 8 seeds below: the worst element error relative to the largest element of the expected matrix is
    # 7.1e-7 (binary32 imats of a skeleton up to 24 deep with scales 0.5 .. 2: inverse(imat) * imat is the identity only to
    # cond(imat) * 2^-24); the margin is 4 x that
    TOL = 4 * 7.1e-7
    worst = 0.0
    for seed in range(8):
        rng = np.random.default_rng(seed)
        imats, wp, joints, local, m = _fold_case(rng)
        off = bind_offsets(imats, joints, local)
        assert off.dtype == np.float32 and off.shape == (len(joints), 16)
        pal = wp @ m(imats.astype(np.float64))  # palette_j = world_j * imat_j
        got = pal[joints] @ m(off.astype(np.float64))
        want = wp[joints] @ m(local.astype(np.float64))
        rel = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
        worst = max(worst, float(rel.max()))
    print(f"bind_offsets: worst relative error {worst:.2e}")
    assert worst <= TOL
    one = bind_offsets(imats, joints, local[0])
    assert (one[3] == bind_offsets(imats, joints[3:4], local[0:1])[0]).all()
    with pytest.raises(ValueError):
        bind_offsets(imats, [len(imats)], local[:1])
