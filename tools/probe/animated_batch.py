"""Animated instance batches: ms per frame for C3 (128 instances of mesh50k, 1080p) and a C5-size batch (1 024 instances x
64 joints, 4K, untextured), each static, with host poses before every frame (Batch.set_poses(numpy): copy + k_pose on the
copy stream) and with device poses before every frame (Batch.set_poses(torch tensor): k_pose on torch's current stream).
Frames are submitted without waiting, through api.FrameLoop; a timed region is `--frames` frames bracketed by a device
synchronise, repeated `--reps` times per mode with the modes alternating, and the median is reported.
Extra modes: device_side_stream (device poses from a non-default torch stream), poses_only (device poses, no frames);
anim (host animation states before every frame: Batch.animate(numpy), 24 bytes per instance + k_anim on the copy stream),
anim_device (states in a torch tensor: k_anim on torch's current stream), anim_only (device states, no frames); tracks,
tracks_device, tracks_only: the same three from a track set (SPEC.md section 15) that mt_renderer_amd.anim_tracks.compress
made of the same clips (--tol: its three tolerances; the encoded and the uniform size are printed and recorded).
Layers (SPEC.md section 16): layers2 (Batch.animate_layers(numpy) with two OVERRIDE layers on mask 0 that say what anim's
states say: the same two clips, positions and weight), layers2_tracks (the same over the track set), layers2_device (the
layers in a torch tensor), layers4 (two more layers on top: a masked OVERRIDE and an ADDITIVE layer of a delta clip that
anim_layers.delta_clip made), layers2_only / layers4_only (device layers, no frames: k_anim_layers alone).  The clip
set (four clips of 120 / 60 / 31 / 2 keys, small bends about z) and the states are generated from --seed.
Inverse kinematics (SPEC.md section 17): anim_ik (Batch.animate_ik(numpy, numpy): three layers -- a base, an OVERRIDE and a
masked OVERRIDE -- and two chains per instance, a TWO_BONE reach with a pole on joints (61, 62, 63) and an AIM at joint 63, at
weight 1), anim_ik_device (layers and targets in torch tensors), ik_only (device records, no frames: k_anim_ik alone) and
layers_only (the same three layers without the chains, no frames: k_anim_layers alone, the yardstick in the same run).
--skeleton chain (the 64-joint chain: both chains walk a path of 62 / 64 joints) or shallow (four chains of 16 joints: paths
of at most 16).
    python tools/probe/animated_batch.py [--only c3|c5] [--frames N] [--reps R] [--modes static,host,anim] [--seed S] [--json OUT]
                                         [--skeleton chain|shallow]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from mt_renderer_amd import anim_layers, anim_tracks, api, scene

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--modes", default="static,host,device,device_side_stream,poses_only")
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--json", default=None)
ap.add_argument("--tol", type=float, default=1e-4)
ap.add_argument("--skeleton", default="chain", choices=("chain", "shallow"))
args = ap.parse_args()
modes = args.modes.split(",")
CHAIN = [255] + list(range(63))  # mesh50k's 64 bones run along the capsule: a chain
if args.skeleton == "shallow":   # four chains of 16: no path longer than 16 joints
    CHAIN = [255 if j % 16 == 0 else j - 1 for j in range(64)]
IK_MODES = ("anim_ik", "anim_ik_device", "ik_only", "layers_only")


def poses(rng, n, k):
    """k pose sets [n, 64, 16]: small bends about z per joint (column-major local matrices)"""
    out = np.zeros((k, n, 64, 16), dtype=np.float32)
    a = rng.uniform(-0.04, 0.04, size=(k, n, 64))
    c, s = np.cos(a), np.sin(a)
    out[..., 0], out[..., 1], out[..., 4], out[..., 5] = c, s, -s, c
    out[..., 10] = out[..., 15] = 1.0
    return out


def clips(rng):
    """(keys [nkeys, 64, 12], flags) per clip: rotations about z within +-0.04 rad, small translations, unit scale"""
    out = []
    for nk, fl in ((120, api.CLIP_LOOP), (60, api.CLIP_LOOP), (31, 0), (2, api.CLIP_LOOP)):
        a = rng.uniform(-0.04, 0.04, size=(nk, 64))
        k = np.zeros((nk, 64, 12), dtype=np.float32)
        k[..., 0:3] = rng.uniform(-0.01, 0.01, size=(nk, 64, 3))
        k[..., 6], k[..., 7] = np.sin(a / 2), np.cos(a / 2)
        k[..., 8:11] = 1.0
        out.append((k, fl))
    return out


def states(rng, n, k):
    """k state sets [n]: every instance somewhere in some clip, three quarters of them cross-fading into another"""
    st = np.zeros((k, n), dtype=api.ANIM_STATE)
    st["clip_a"], st["clip_b"] = rng.integers(0, 4, (k, n)), rng.integers(0, 4, (k, n))
    st["x_a"], st["x_b"] = rng.uniform(0, 240, (k, n)), rng.uniform(0, 240, (k, n))
    st["w"] = np.where(rng.random((k, n)) < 0.25, 0.0, rng.uniform(0, 1, (k, n)))
    return st


def layers(st, L, rng):
    """layer stacks [k, n, L] that say what the states say with their first two layers (OVERRIDE, mask 0); for L = 4 a masked
    OVERRIDE of another clip and an ADDITIVE layer of the delta clip (clip 4) on top"""
    ly = np.zeros(st.shape + (L,), dtype=api.ANIM_LAYER)
    ly["clip"][..., 0], ly["x"][..., 0] = st["clip_a"], st["x_a"]
    ly["clip"][..., 1], ly["x"][..., 1], ly["w"][..., 1] = st["clip_b"], st["x_b"], st["w"]
    if L == 4:
        ly["clip"][..., 2], ly["x"][..., 2] = rng.integers(0, 4, st.shape), rng.uniform(0, 240, st.shape)
        ly["w"][..., 2], ly["mask"][..., 2] = rng.uniform(0.2, 1, st.shape), 1
        ly["clip"][..., 3], ly["x"][..., 3] = 4, rng.uniform(0, 30, st.shape)
        ly["w"][..., 3], ly["mask"][..., 3], ly["mode"][..., 3] = rng.uniform(0.2, 1, st.shape), 2, api.LAYER_ADDITIVE
    return ly


dev = api.Device(0)
results = []
for name, nx, ny, W, H in (("c3", 16, 8, 1920, 1080), ("c5", 32, 32, 3840, 2160)):
    if args.only and args.only != name:
        continue
    md = scene.mesh50k()
    mats, pals = scene.instance_lattice(nx, ny)
    n = nx * ny
    model = api.Model.new(dev, md)
    model.set_skeleton(CHAIN, np.tile(np.eye(4, dtype=np.float32).reshape(16), (64, 1)))
    batch = api.Batch(dev, model, mats, pals)
    rng = np.random.default_rng(args.seed)
    host = poses(rng, n, 8)
    devp = [torch.tensor(p, device="cuda:0") for p in host]
    uniform_clips = clips(rng)
    anim = api.Anim(dev, 64, uniform_clips)
    with_ik = any(m in IK_MODES for m in modes)
    with_layers = with_ik or any(m.startswith("layers") for m in modes)
    sizes = None
    if any(m.startswith("tracks") or m == "layers2_tracks" for m in modes):
        track_clips = [anim_tracks.compress(k, fl, args.tol, args.tol, args.tol) for k, fl in uniform_clips]
        tracks = api.AnimTracks(dev, 64, track_clips)
        sizes = dict(uniform_bytes=sum(anim_tracks.uniform_bytes(k.shape[0], 64) for k, _ in uniform_clips),
                     track_bytes=sum(anim_tracks.encoded_bytes(c) for c in track_clips), track_keys=int(sum(c[3].size for c in track_clips)), tol=args.tol)
        print(json.dumps(dict(config=name, clip_set=sizes)), flush=True)
    host_st = states(rng, n, 8)
    dev_st = [torch.from_numpy(s.view(np.uint8).reshape(n, 24).copy()).to("cuda:0") for s in host_st]
    if with_layers:  # after everything the other modes draw from rng: their inputs stay what they were
        layer_clips = uniform_clips + [(anim_layers.delta_clip(uniform_clips[2][0], uniform_clips[0][0][0]), 0)]
        lanim = api.Anim(dev, 64, layer_clips)
        mw = np.zeros((2, 64), dtype=np.float32)
        mw[0, 32:], mw[1] = np.linspace(0.0, 1.0, 32), rng.uniform(0.0, 1.0, 64)
        lmasks = api.AnimMasks(dev, 64, mw)
        host_ly = {L: layers(host_st, L, rng) for L in (2, 4)}
        dev_ly = {L: [torch.from_numpy(x.view(np.uint8).reshape(n, L * 16).copy()).to("cuda:0") for x in host_ly[L]] for L in (2, 4)}
    if with_ik:
        chains = np.zeros(2, dtype=api.ANIM_IK_CHAIN)
        chains["kind"], chains["flags"] = [api.IK_TWO_BONE, api.IK_AIM], [api.IK_POLE, 0]
        chains["joint"], chains["axis"][1] = [(61, 62, 63), (63, 0, 0)], (0.0, 1.0, 0.0)
        iks = api.AnimIK(dev, CHAIN, chains)
        host_ly3 = [np.ascontiguousarray(x[:, :3]) for x in host_ly[4]]
        dev_ly3 = [torch.from_numpy(x.view(np.uint8).reshape(n, 48).copy()).to("cuda:0") for x in host_ly3]
        host_tg = np.zeros((8, n, 2), dtype=api.ANIM_IK_TARGET)
        host_tg["pos"], host_tg["pole"], host_tg["w"] = rng.uniform(-1, 1, (8, n, 2, 3)), rng.uniform(-2, 2, (8, n, 2, 3)), 1.0
        dev_tg = [torch.from_numpy(x.view(np.uint8).reshape(n, 64).copy()).to("cuda:0") for x in host_tg]
    loop = api.FrameLoop(dev, W, H, batch=batch, view_proj=scene.to_f32_colmajor(scene.reference_view_proj(W, H)))

    side = torch.cuda.Stream()

    def region(mode, nframes):
        for k in range(nframes):
            if mode == "host":
                batch.set_poses(host[k % 8])
            elif mode == "device":
                batch.set_poses(devp[k % 8])
            elif mode == "device_side_stream":  # the same from a non-default torch stream
                with torch.cuda.stream(side):
                    batch.set_poses(devp[k % 8])
            elif mode == "anim":
                batch.animate(anim, host_st[k % 8])
            elif mode == "anim_device":
                batch.animate(anim, dev_st[k % 8])
            elif mode == "anim_only":  # device states and no frames: k_anim alone on the GPU
                batch.animate(anim, dev_st[k % 8])
                continue
            elif mode == "tracks":
                batch.animate(tracks, host_st[k % 8])
            elif mode == "tracks_device":
                batch.animate(tracks, dev_st[k % 8])
            elif mode == "tracks_only":  # device states and no frames: k_anim_tracks alone on the GPU
                batch.animate(tracks, dev_st[k % 8])
                continue
            elif mode in ("layers2", "layers4"):
                batch.animate_layers(lanim, host_ly[int(mode[6])][k % 8], lmasks)
            elif mode == "layers2_tracks":
                batch.animate_layers(tracks, host_ly[2][k % 8], lmasks)
            elif mode == "layers2_device":
                batch.animate_layers(lanim, dev_ly[2][k % 8], lmasks)
            elif mode in ("layers2_only", "layers4_only"):  # device layers and no frames: k_anim_layers alone on the GPU
                batch.animate_layers(lanim, dev_ly[int(mode[6])][k % 8], lmasks)
                continue
            elif mode == "anim_ik":
                batch.animate_ik(lanim, host_ly3[k % 8], iks, host_tg[k % 8], lmasks)
            elif mode == "anim_ik_device":
                batch.animate_ik(lanim, dev_ly3[k % 8], iks, dev_tg[k % 8], lmasks)
            elif mode == "ik_only":  # device records and no frames: k_anim_ik alone on the GPU
                batch.animate_ik(lanim, dev_ly3[k % 8], iks, dev_tg[k % 8], lmasks)
                continue
            elif mode == "layers_only":  # the same three layers without the chains: k_anim_layers alone on the GPU
                batch.animate_layers(lanim, dev_ly3[k % 8], lmasks)
                continue
            elif mode == "poses_only":  # device poses and no frames: k_pose alone on the GPU
                batch.set_poses(devp[k % 8])
                continue
            loop.run(1)

    def timed(mode):
        dev.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        region(mode, args.frames)
        dev.synchronize(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.frames * 1e3

    for mode in modes:
        region(mode, 30)  # warm-up: code objects, the batch's version ring, the staging buffer
    ms = {m: [] for m in modes}
    for _ in range(args.reps):
        for mode in modes:
            ms[mode].append(timed(mode))
    for mode in modes:
        r = dict(config=name, instances=n, joints=64, width=W, height=H, mode=mode, frames=args.frames, skeleton=args.skeleton,
                 ms_per_frame=round(float(np.median(ms[mode])), 4), ms_all=[round(v, 4) for v in ms[mode]])
        if sizes and mode.startswith("tracks"):
            r["clip_set"] = sizes
        results.append(r)
        print(json.dumps(r), flush=True)
    batch.close()
    anim.close()
    if with_ik:
        iks.close()
    if with_layers:
        lmasks.close()
        lanim.close()
    if sizes:
        tracks.close()
    model.close()
dev.close()
if args.json:
    json.dump(results, open(args.json, "w"), indent=1)
