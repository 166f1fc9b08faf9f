#!/usr/bin/env python3
"""CPU-side counts behind k_tile_vis.hip's span walk, on the headline scene: for every bin-clipped (triangle, bin) entry,
the bbox pixels the pair walk visits, the pixel centres the triangle covers (SPEC.md's inside test with the top-left rule),
the bbox rows the span walk visits and how many of them cover a centre -- per class of bbox size.  Analysis only (uses the
oracle's vertex stage, the way tools/raster_stats.py does).   usage: python tools/span_stats.py"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mt_renderer_amd import scene
from oracle import oracle as orc

W, H, BIN = 1920, 1080, 16
NBX = (W + BIN - 1) // BIN
md = scene.headline_model()
om = orc.OracleModel(md)
M = scene.to_f32_colmajor(scene.headline_transform(W, H))
pal = scene.bone_palette()
keys, covered, rowkey = [], [], []
ntri = 0
for p in range(md.nprims):
    f = scene.unpack_primitive(md.prims[p])
    clip, _ = om.vertex_stage(p, M, pal)
    w = clip[:, 3]
    X = np.rint((clip[:, 0] / w * 0.5 + 0.5) * W * 256).astype(np.int64)
    Y = np.rint((0.5 - clip[:, 1] / w * 0.5) * H * 256).astype(np.int64)
    idx = md.index_buf[f["index_ofs"]: f["index_ofs"] + f["index_num"]].astype(np.int64)
    i0, i1, i2 = idx[:-2], idx[1:-1], idx[2:]
    ok = (i0 != 0xFFFF) & (i1 != 0xFFFF) & (i2 != 0xFFFF)
    par = np.zeros(len(i0), dtype=bool)
    q = 0
    for k, v in enumerate(idx):  # parity within strips
        if v == 0xFFFF: q = 0; continue
        q += 1
        if q >= 3: par[k - 2] = ((q - 3) & 1) != 0
    a, b, c = i0, np.where(par, i2, i1), np.where(par, i1, i2)
    a, b, c = a[ok], b[ok], c[ok]
    A2 = (X[c] - X[a]) * (Y[b] - Y[a]) - (X[b] - X[a]) * (Y[c] - Y[a])
    fr = A2 > 0
    xs = np.stack([X[a[fr]], X[b[fr]], X[c[fr]]]); ys = np.stack([Y[a[fr]], Y[b[fr]], Y[c[fr]]])
    px0 = np.maximum((xs.min(0) + 127) >> 8, 0); px1 = np.minimum((xs.max(0) - 128) >> 8, W - 1)
    py0 = np.maximum((ys.min(0) + 127) >> 8, 0); py1 = np.minimum((ys.max(0) - 128) >> 8, H - 1)
    keep = (px0 <= px1) & (py0 <= py1)
    xs, ys, px0, px1, py0, py1 = xs[:, keep], ys[:, keep], px0[keep], px1[keep], py0[keep], py1[keep]
    bw, bh = px1 - px0 + 1, py1 - py0 + 1
    n = bw * bh
    # every pixel of every bbox: triangle t, pixel (x, y)
    t = np.repeat(np.arange(len(n)), n)
    k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    x = px0[t] + k % bw[t]
    y = py0[t] + k // bw[t]
    Px, Py = x * 256 + 128, y * 256 + 128
    inside = np.ones(len(t), dtype=bool)
    for i in range(3):
        ia, ib = (i + 1) % 3, (i + 2) % 3
        dx, dy = xs[ib] - xs[ia], ys[ib] - ys[ia]
        tl = ((dy > 0) | ((dy == 0) & (dx < 0))).astype(np.int64)
        E = dy[t] * (Px - xs[ia][t]) - dx[t] * (Py - ys[ia][t]) + (tl[t] - 1)
        inside &= E >= 0
    tg = t + ntri
    ntri += len(n)
    keys.append(tg * (NBX * ((H + BIN - 1) // BIN)) + (y // BIN) * NBX + x // BIN)
    covered.append(inside)
    rowkey.append(y)
key = np.concatenate(keys); cov = np.concatenate(covered); yy = np.concatenate(rowkey)
ent, inv = np.unique(key, return_inverse=True)
npx = np.bincount(inv)
ncov = np.bincount(inv, weights=cov).astype(np.int64)
# rows: distinct (entry, y); non-empty rows: distinct (entry, y) with a covered centre
rk = inv.astype(np.int64) * 2048 + yy
ur, rinv = np.unique(rk, return_inverse=True)
row_cov = np.bincount(rinv, weights=cov) > 0
row_ent = ur // 2048
nrows = np.bincount(row_ent, minlength=len(ent))
nrows_ne = np.bincount(row_ent, weights=row_cov, minlength=len(ent)).astype(np.int64)
print("| bbox pixels per bin-clipped entry | entries | bbox pairs walked | covered pairs | bbox rows (non-empty) |")
print("|---|---|---|---|---|")
for name, lo, hi in (("<= 4", 1, 4), ("5-16", 5, 16), ("17-64", 17, 64), ("> 64", 65, 1 << 30), ("all", 1, 1 << 30)):
    m = (npx >= lo) & (npx <= hi)
    print("| %s | %d | %d | %d (%.1f %%) | %d (%d) |" % (name, m.sum(), npx[m].sum(), ncov[m].sum(), 100.0 * ncov[m].sum() / max(1, npx[m].sum()),
                                                    nrows[m].sum(), nrows_ne[m].sum()))
