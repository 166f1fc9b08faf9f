"""A readable description of a controller (SPEC.md section 21) turned into the tables mtr_anim_ctrl_create takes.  A helper,
not part of the rule: the rule is what the tables say.

    nodes = [dict(name="idle", clip=0), dict(name="walk", clip=1), dict(name="jump", clip=3)]
    transitions = [
        dict(src="any", dst="jump", when=[("trigger", ">", 0.5)], flags=("interrupt", "consume")),
        dict(src="idle", dst="walk", when=[("speed", ">", 0.6)], seconds=0.2),
        dict(src="jump", dst="idle", when=[("ENDED", ">=", 1.0)], seconds=0.1),
    ]
    g = build(nodes, transitions)
    ctrl = api.AnimCtrl(dev, nkeys, clip_flags, g["nodes"], g["trans"], g["nany"], len(g["params"]))

Priority is the order of the list: the any-state transitions come first in the order given, then each node's own in the order
given.  Parameter names are numbered in order of first appearance (or as `params` lists them); TIME, POS, PHASE, ENDED and
FADING name the built-ins."""
import numpy as np

from . import api

OPS = {"<": api.OP_LT, "<=": api.OP_LE, ">": api.OP_GT, ">=": api.OP_GE, "==": api.OP_EQ, "!=": api.OP_NE}
FLAGS = {"interrupt": api.TR_INTERRUPT, "self": api.TR_SELF, "sync": api.TR_SYNC, "consume": api.TR_CONSUME}
BUILTINS = {"TIME": api.CTRL_TIME, "POS": api.CTRL_POS, "PHASE": api.CTRL_PHASE, "ENDED": api.CTRL_ENDED, "FADING": api.CTRL_FADING}


def _bad(msg):
    return api.MtrError(api.MTR_E_INVALID, "anim ctrl build: " + msg)


def build(nodes, transitions, params=None):
    """-> dict(nodes=CTRL_NODE [S], trans=CTRL_TRANS [T] sorted any-state first and then node by node, nany, params=[names],
    index={node name: index})"""
    index = {}
    for i, nd in enumerate(nodes):
        if set(nd) - {"name", "clip"} or "name" not in nd or "clip" not in nd or nd["name"] in index or nd["name"] == "any":
            raise _bad(f"node {i}: a unique name other than 'any', and a clip")
        index[nd["name"]] = i
    names = list(params or [])
    rows = []
    for i, t in enumerate(transitions):
        if set(t) - {"src", "dst", "when", "seconds", "x", "flags"} or "src" not in t or "dst" not in t:
            raise _bad(f"transition {i}: src and dst, optionally when, seconds, x and flags")
        if (t["src"] != "any" and t["src"] not in index) or t["dst"] not in index:
            raise _bad(f"transition {i}: src or dst names no node")
        when = list(t.get("when", ()))
        if len(when) > api.CTRL_MAX_COND:
            raise _bad(f"transition {i}: at most {api.CTRL_MAX_COND} conditions")
        r = np.zeros(1, dtype=api.CTRL_TRANS)[0]
        r["target"], r["seconds"], r["x"], r["ncond"] = index[t["dst"]], t.get("seconds", 0.0), t.get("x", 0.0), len(when)
        for fl in t.get("flags", ()):
            if fl not in FLAGS:
                raise _bad(f"transition {i}: flags are {sorted(FLAGS)}")
            r["flags"] |= FLAGS[fl]
        for k, cnd in enumerate(when):
            if len(cnd) != 3 or cnd[1] not in OPS or not isinstance(cnd[0], str):
                raise _bad(f"transition {i}: a condition is (parameter name, one of {sorted(OPS)}, value)")
            if cnd[0] in BUILTINS:
                p = BUILTINS[cnd[0]]
            else:
                if cnd[0] not in names:
                    if params is not None:
                        raise _bad(f"transition {i}: {cnd[0]} is not among the parameters")
                    names.append(cnd[0])
                p = names.index(cnd[0])
            r["cond"][k] = (p, OPS[cnd[1]], cnd[2])
        rows.append((-1 if t["src"] == "any" else index[t["src"]], r))
    order = sorted(range(len(rows)), key=lambda i: rows[i][0])  # stable: the given order within one source
    trans = np.array([rows[i][1] for i in order], dtype=api.CTRL_TRANS) if rows else np.zeros(0, dtype=api.CTRL_TRANS)
    src = np.array([rows[i][0] for i in order], dtype=np.int64)
    nany = int((src < 0).sum())
    out = np.zeros(len(nodes), dtype=api.CTRL_NODE)
    for i, nd in enumerate(nodes):
        mine = np.flatnonzero(src == i)
        out[i] = (nd["clip"], mine[0] if len(mine) else nany, len(mine), 0)
    return dict(nodes=out, trans=trans, nany=nany, params=names, index=index)
