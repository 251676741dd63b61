"""Timing probe (not product): config-2 frames (synth-room 1.2 M points, 800x800, SR 64) at one
precision; prints one JSON line with per-stage HIP-event medians.  Usage:
    python tools/agg_time.py [f32|f16] [frames]
SGN_ROT=1: the same frames with a rotation per point (Rw2c from a four-matrix palette: the rotated kernels;
sgn_sample_viewdirs runs between the "query" and "proj" marks, so its time is in the query stage)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import sgnerf_amd  # noqa: E402,F401
from sgnerf_amd import scene  # noqa: E402
from sgnerf_amd.opts import HotPathOpts  # noqa: E402
from sgnerf_amd.render import HipRenderer, PointTables  # noqa: E402
from sgnerf_amd.weights import init_mlp  # noqa: E402

prec = sys.argv[1] if len(sys.argv) > 1 else "f32"
nf = int(sys.argv[2]) if len(sys.argv) > 2 else 8
dev = "cuda:0"
pc = scene.synth_room(1_200_000, seed=0)
mlp = init_mlp(0, bias_std=0.01)
mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 50.0
rw2c = None
if os.environ.get("SGN_ROT", "0") == "1":
    def _axis(a, deg):
        a = np.asarray(a, np.float64) / np.linalg.norm(a)
        k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        return np.eye(3) + np.sin(np.deg2rad(deg)) * k + (1 - np.cos(np.deg2rad(deg))) * (k @ k)
    pal = np.stack([np.eye(3), _axis((0, 0, 1), 40.0), _axis((1, 2, 3), 75.0), _axis((-1, 1, 0.5), 170.0)]).astype(np.float32)
    rw2c = torch.from_numpy(pal[np.random.default_rng(5).integers(0, 4, pc.xyz.shape[0])])
r = HipRenderer(PointTables(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, dev, rot=rw2c), mlp,
                HotPathOpts(SR=64, precision=prec), dev)
# SGN_RAY_ORDER=B (B > 0): rays fed in B x B pixel blocks (block-major) instead of row-major
blk = int(os.environ.get("SGN_RAY_ORDER", "0"))
perm = None
if blk > 0:
    yy, xx = np.meshgrid(np.arange(800), np.arange(800), indexing="ij")
    key = ((yy // blk) * (800 // blk) + (xx // blk)) * (blk * blk) + (yy % blk) * blk + (xx % blk)
    perm = torch.from_numpy(np.argsort(key.reshape(-1), kind="stable"))
views = []
for i in range(3 + nf):
    yaw, pitch = scene.spiral_yaw_pitch(i % 120, 120)
    v = scene.room_view(800, 800, yaw=yaw + 15.0, pitch=pitch - 5.0)
    rd = torch.from_numpy(v.raydir)
    if perm is not None:
        rd = rd[perm].contiguous()
    views.append((torch.from_numpy(v.campos).to(dev), torch.from_numpy(v.camrotc2w).to(dev),
                  rd.to(dev), v.near, v.far))
ev = []


def mark(n):
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    ev[-1][n] = e


for i, (c, rot, rd, ne, fa) in enumerate(views):
    if i >= 3:
        ev.append({})
    r.render(c, rot, rd, ne, fa, marks=mark if i >= 3 else None, check_range=False)
torch.cuda.synchronize()
names = ["query", "proj", "agg_rows", "agg_color", "composite", "end"]
res = {n: float(np.median([e[n].elapsed_time(e[names[j + 1]]) for e in ev])) for j, n in enumerate(names[:-1])}
res["frame"] = float(np.median([e["query"].elapsed_time(e["end"]) for e in ev]))
res["prec"] = prec
res["lib"] = os.environ.get("SGN_VARIANT", "base")
res["ray_block"] = blk
res["rot"] = rw2c is not None
print(json.dumps(res), flush=True)
