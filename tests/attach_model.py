"""Attachments (SPEC.md section 18) in numpy, written from the section: the matrices `(M_src . P) . O` of a set of attachment
records against one source batch, in binary32 (what k_attach and csrc/attach_math.h must equal bit for bit) and in float64
(what section 18's accuracy statement is measured against), the generator of the cases every attachment test runs, and
seven deliberately wrong readings of the section (WRONG_VARIANTS).

Matrices are column-major [.., 16], element c * 4 + i = column c, row i.  Every product is section 12's chain: out[c][i] =
fmaf over k = 0..3 of A[k][i] * B[c][k], from 0, with the exact binary32 fma of tests/anim_ik_model.py."""
import numpy as np

from tests.anim_ik_model import fma32

F = np.float32
ATTACH = np.dtype([("src_instance", "<u4"), ("joint", "<u4"), ("flags", "<u4"), ("pad", "<u4"), ("offset", "<f4", 16)])
NO_JOINT = 0xFFFFFFFF
POSITION_ONLY = 1
WRONG_VARIANTS = ("offset_left", "pal_left", "assoc_right", "unfused", "clamp_npal", "pos_from_msrc", "flags_upper")

N_SRC = (1, 7)
NPAL = (0, 1, 64, 256)
COUNTS = (1, 3, 4, 5, 63, 64, 65, 257)  # the partial group of four, the wave boundary, the second workgroup


def mul(A, B, dt=F, fused=True):
    """A B on [n, 4 columns, 4 rows]"""
    r = np.zeros(A.shape, dtype=dt)
    for k in range(4):
        x, y = A[:, None, k, :], B[:, :, k, None]
        with np.errstate(all="ignore"):
            if dt != F:
                r = x * y + r
            elif fused:
                r = fma32(x, y, r)
            else:
                r = ((x * y).astype(F) + r).astype(F)
    return r


def attach(M_src, P_src, recs, variant=None, dt=F):
    """the matrices [n, 16] of `recs` (ATTACH [n]) against a source of instance matrices M_src [n_src, 16] and palettes P_src
    [n_src, npal, 16] (None or npal == 0: none)"""
    n_src = M_src.shape[0]
    npal = 0 if P_src is None else P_src.shape[1]
    n = recs.shape[0]
    fused = variant != "unfused"
    s = np.minimum(recs["src_instance"].astype(np.int64), n_src - 1)
    M = M_src[s].reshape(n, 4, 4).astype(dt)
    O = recs["offset"].reshape(n, 4, 4).astype(dt)
    joint = recs["joint"].astype(np.int64)
    has = (joint != NO_JOINT) & (npal > 0)
    A, P = M, None
    if npal:
        if variant == "clamp_npal":  # reads one matrix past the instance's palette (wrapped, to stay inside the array)
            flat = (s * npal + np.minimum(joint, npal)) % (n_src * npal)
            P = P_src.reshape(-1, 16)[flat]
        else:
            P = P_src[s, np.minimum(joint, npal - 1)]
        P = P.reshape(n, 4, 4).astype(dt)
        MP = mul(P, M, dt, fused) if variant == "pal_left" else mul(M, P, dt, fused)
        A = np.where(has[:, None, None], MP, M)
    flags = recs["flags"]
    pos = (flags == 1) if variant == "flags_upper" else (flags & 1) != 0
    T = M if variant == "pos_from_msrc" else A
    Apos = np.zeros((n, 4, 4), dtype=dt)
    Apos[:, 0, 0] = Apos[:, 1, 1] = Apos[:, 2, 2] = Apos[:, 3, 3] = 1
    Apos[:, 3, :3] = T[:, 3, :3]
    A = np.where(pos[:, None, None], Apos, A)
    out = mul(O, A, dt, fused) if variant == "offset_left" else mul(A, O, dt, fused)
    if variant == "assoc_right" and npal:
        alt = mul(M, mul(P, O, dt, fused), dt, fused)
        out = np.where((has & ~pos)[:, None, None], alt, out)
    return np.ascontiguousarray(out.reshape(n, 16))


def bound(M_src, P_src, recs):
    """section 18's bound per element, [n, 16]: gamma_8 (gamma_4 without a joint) times the same products on absolute values"""
    u = 2.0 ** -24
    absr = recs.copy()
    absr["offset"] = np.abs(recs["offset"])
    S = attach(np.abs(M_src), None if P_src is None else np.abs(P_src), absr, dt=np.float64)
    npal = 0 if P_src is None else P_src.shape[1]
    k = np.where((recs["joint"] != NO_JOINT) & (npal > 0), 8.0, 4.0)[:, None]
    return k * u / (1 - k * u) * S


def trs(rng, n, tmax=20.0):
    """n matrices [n, 16]: a rotation, per-axis scales 0.5 .. 2, a translation up to tmax per axis"""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.empty((n, 3, 3))  # [row][column]
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    sc = 2.0 ** rng.uniform(-1, 1, size=(n, 3))
    m = np.zeros((n, 4, 4))  # [column][row]
    m[:, :3, :3] = (R * sc[:, None, :]).transpose(0, 2, 1)
    m[:, 3, :3] = rng.uniform(-tmax, tmax, size=(n, 3))
    m[:, 3, 3] = 1
    return m.reshape(n, 16).astype(F)


SPECIALS = (1e-40, -3e-45, np.inf, -np.inf, np.nan, 3e38)  # denormals, infinities, NaN, a value whose products overflow


def records(rng, n, n_src, npal):
    """n records: indices in range, beyond range (the clamp) and NO_JOINT, both flag values with junk above bit 0, junk in
    pad, TRS offsets; from 63 records on, six whose offset holds a denormal, an infinity, a NaN or a huge element"""
    r = np.zeros(n, dtype=ATTACH)
    k = np.arange(n)
    r["src_instance"] = rng.integers(0, n_src, size=n)
    far = k % 7 == 3
    r["src_instance"][far] = np.where(rng.random(far.sum()) < 0.5, n_src + rng.integers(0, 3, size=far.sum()), 0xFFFFFFFF - rng.integers(0, 2, size=far.sum()))
    r["joint"] = rng.integers(0, max(npal, 1), size=n)
    r["joint"][k % 5 == 1] = NO_JOINT
    past = k % 5 == 4
    r["joint"][past] = np.where(rng.random(past.sum()) < 0.7, npal + rng.integers(0, 3, size=past.sum()), 0xFFFFFFFE)
    r["flags"] = (k % 4 == 2).astype(np.uint32)
    junk = k % 3 == 0
    r["flags"][junk] |= (rng.integers(1, 1 << 31, size=junk.sum()) << 1).astype(np.uint32)
    r["pad"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    r["offset"] = trs(rng, n, 2.0)
    if n >= 63:
        for t, v in enumerate(SPECIALS):
            r["offset"][10 + t, (5 * t + 3) % 16] = v
    return r


def cases():
    """every (n_src, npal, count) of the section's test plan: dicts of name, M_src, P_src (None when npal == 0), recs"""
    out = []
    for n_src in N_SRC:
        for npal in NPAL:
            for n in COUNTS:
                rng = np.random.default_rng(1000 * n_src + 10 * npal + n)
                M = trs(rng, n_src)
                P = trs(rng, n_src * npal, 5.0).reshape(n_src, npal, 16) if npal else None
                out.append(dict(name=f"src{n_src}_pal{npal}_n{n}", n_src=n_src, npal=npal, n=n, M_src=M, P_src=P, recs=records(rng, n, n_src, npal)))
    return out


def can_show(variant, case):
    """whether a wrong reading can change a record of the case at all; the reasons are the exemptions of
    tests/test_attach_model.py"""
    r, npal = case["recs"], case["npal"]
    has = (r["joint"] != NO_JOINT) & (npal > 0)
    pos = (r["flags"] & 1) != 0
    if variant in ("offset_left", "unfused"):
        return True
    if variant == "pal_left":  # needs a palette matrix
        return bool(has.any())
    if variant == "assoc_right":  # needs both products of a record: a joint, and an A that is not replaced
        return bool((has & ~pos).any())
    if variant == "clamp_npal":  # needs a joint index past the palette, and a second palette matrix to read instead
        return bool((has & (r["joint"] >= npal)).any()) and case["n_src"] * npal > 1
    if variant == "pos_from_msrc":  # needs a position-only record whose A is not M_src itself
        return bool((has & pos).any())
    if variant == "flags_upper":  # needs bit 0 set under junk (bit 0 clear under junk reads 'not position-only' either way)
        return bool((pos & (r["flags"] >> 1 != 0)).any())
    raise KeyError(variant)


def same_bits(a, b):
    """per element: equal bits, or NaN in both (payloads are free)"""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
