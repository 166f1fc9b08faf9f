"""A readable description of an event set (SPEC.md section 22) turned into the arrays mtr_anim_events_create takes, and the
records of a collected list taken apart.  Helpers, not part of the rule: the rule is what the arrays say.

    FOOT_L, FOOT_R, HIT = 0, 1, 2
    counts, markers = build({WALK: [(7.0, FOOT_L), (23.0, FOOT_R)], ATTACK: [(11.0, HIT)]}, nclips=4)
    events = api.AnimEvents(dev, nkeys, clip_flags, counts, markers, max_instances=n)
    ...
    for e in decode(list_from_the_gpu[:written]):
        e["instance"], e["id"], e["clip"], e["step"], e["backward"], e["w"]

Markers of one clip are sorted by position; markers at one position keep the order they were given in, which is the order
they fire in when the clip runs forward."""
import numpy as np

from . import api


def _bad(msg):
    return api.MtrError(api.MTR_E_INVALID, "anim events build: " + msg)


def build(markers, nclips):
    """{clip: [(x, id), ...]} -> (counts uint32 [nclips], EVENT_MARKER [sum of counts]), each clip's markers sorted stably by x"""
    counts = np.zeros(nclips, dtype=np.uint32)
    parts = []
    for c in sorted(markers):
        if not isinstance(c, (int, np.integer)) or c < 0 or c >= nclips:
            raise _bad(f"clip {c}: the set has clips 0 to {nclips - 1}")
        rows = list(markers[c])
        if any(len(r) != 2 for r in rows):
            raise _bad(f"clip {c}: a marker is (x, id)")
        m = np.zeros(len(rows), dtype=api.EVENT_MARKER)
        m["x"] = [r[0] for r in rows]
        m["id"] = [r[1] for r in rows]
        if np.isnan(m["x"]).any():
            raise _bad(f"clip {c}: a marker's position is NaN")
        parts.append(m[np.argsort(m["x"], kind="stable")])
        counts[c] = len(rows)
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=api.EVENT_MARKER)
    return counts, np.ascontiguousarray(out, dtype=api.EVENT_MARKER)


DECODED = np.dtype([("instance", "<u4"), ("id", "<u4"), ("clip", "<u4"), ("step", "<u4"), ("backward", "?"), ("w", "<f4")])


def decode(events):
    """EVENT records -> records with `where` split into clip, step and backward"""
    ev = np.asarray(events)
    if ev.dtype != api.EVENT:
        raise api.MtrError(api.MTR_E_INVALID, "anim events decode: an array of dtype EVENT")
    out = np.zeros(ev.shape, dtype=DECODED)
    out["instance"], out["id"], out["w"] = ev["instance"], ev["id"], ev["w"]
    out["clip"] = ev["where"] & 0xFFFFFF
    out["step"] = (ev["where"] >> 24) & 0x7F
    out["backward"] = (ev["where"] & api.EVENT_BACKWARD) != 0
    return out
