"""Timing probe (not product): config-2 frames (synth-room 1.2 M points, 800x800, SR 64) of the viewmlp
without block3 (shading_feature_mlp_layer3 = 0) on the plain-fp32 kernels, beside the stock network forced
onto the same path (HipRenderer.exact = True) for the same frames.  Prints one JSON line per network with
per-stage HIP-event medians and rays/s.  Usage:
    python tools/agg_time_nb3.py [frames] [bpnet_layers bpnet_dim] [--rows_gemm | --rows_fused]
--rows_fused: three paths alternated frame by frame on the same frames, one JSON line each with the median, minimum
and maximum of rows + colour ("agg") over the frames: the network without block3 on the row GEMMs (rows_gemm = 1,
path "rows-gemm"), on the fused row kernel (rows_fused = 1, path "rows-fused"), and the stock network on its own
split-fp16 kernels (path "stock-split": k_rows16 + k_color16 with all four row layers).
--rows_gemm: also the network without block3 on the split-fp16 row GEMMs (opts.rows_gemm = 1; path "rows-gemm"), on
the same frames; its "agg" stage is the lists, every window's launches and the colour MLP.
On the plain-fp32 path sgn_aggregate_exact[_nb3] launches the row kernel and the colour kernel from one call, so the
"agg" stage is their sum; k_color_exact is the same kernel for both networks, and a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/agg_time_nb3.py) splits the two."""
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

argv = [a for a in sys.argv[1:] if a not in ("--rows_gemm", "--rows_fused")]
rows_gemm = "--rows_gemm" in sys.argv[1:]
rows_fused = "--rows_fused" in sys.argv[1:]
nf = int(argv[0]) if len(argv) > 0 else 6
nl, dim = (int(argv[1]), int(argv[2])) if len(argv) > 2 else (0, 0)
dev = "cuda:0"
pc = scene.synth_room(1_200_000, seed=0)
if dim:
    pc = scene.with_semantics(pc, seed=1)
views = []
for i in range(2 + nf):
    yaw, pitch = scene.spiral_yaw_pitch(i % 120, 120)
    v = scene.room_view(800, 800, yaw=yaw + 15.0, pitch=pitch - 5.0)
    views.append((torch.from_numpy(v.campos).to(dev), torch.from_numpy(v.camrotc2w).to(dev),
                  torch.from_numpy(v.raydir).to(dev), v.near, v.far))
names = ["query", "proj", "agg_rows", "agg_color", "composite", "end"]
kw = {}
if dim:   # labels all 0 pass the semantic filter
    kw = dict(point_labels=torch.zeros(pc.xyz.shape[0], dtype=torch.int32, device=dev),
              ray_labels=torch.zeros(800 * 800, dtype=torch.int32, device=dev), seconds=5)


def renderer(block3, **knobs):
    mlp = init_mlp(0, bias_std=0.01, bpnet_layers=nl, bpnet_dim=dim, block3_layers=block3)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 50.0
    o = HotPathOpts(SR=64, shading_feature_mlp_layer3=block3, shading_feature_mlp_layer2_bpnet=nl,
                    predict_semantic=1 if dim else 0, semantic_guidance=1 if dim else 0, **knobs)
    tab = PointTables(pc.xyz, pc.embedding, pc.color if block3 else None, pc.dir if block3 else None, pc.conf, dev,
                      bpnet=pc.bpnet if dim else None)
    return HipRenderer(tab, mlp, o, dev)


if rows_fused:
    paths = [("rows-gemm", renderer(0, rows_gemm=1)), ("rows-fused", renderer(0, rows_fused=1)), ("stock-split", renderer(2))]
    evs = {p: [] for p, _ in paths}
    for i, (c, rot, rd, ne, fa) in enumerate(views):
        for p, r in paths:   # alternated per frame
            if i >= 2:
                evs[p].append({})

            def mark(n, p=p):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                evs[p][-1][n] = e
            r.render(c, rot, rd, ne, fa, marks=mark if i >= 2 else None, check_range=False, **kw)
    torch.cuda.synchronize()
    for p, r in paths:
        ev = evs[p]
        res = {n: float(np.median([e[n].elapsed_time(e[names[j + 1]]) for e in ev])) for j, n in enumerate(names[:-1])}
        agg = [e["agg_rows"].elapsed_time(e["composite"]) for e in ev]
        res.update(agg=float(np.median(agg)), agg_min=float(min(agg)), agg_max=float(max(agg)))
        res["frame"] = float(np.median([e["query"].elapsed_time(e["end"]) for e in ev]))
        res["rays_per_s"] = 800 * 800 / res["frame"] * 1e3
        res.update(bpnet=[nl, dim], frames=nf, path=p, on_path=not r.exact and (r._rows_frame if r.rows is not None else
                                                                                r._fused_frame if r.fused else True))
        print(json.dumps(res), flush=True)
    sys.exit(0)

for block3, rows in [(0, 0)] + ([(0, 1)] if rows_gemm else []) + [(2, 0)]:
    r = renderer(block3, rows_gemm=rows)
    if not rows:
        r.exact = True   # the stock network: the plain-fp32 path from the first frame
    ev = []

    def mark(n):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        ev[-1][n] = e

    for i, (c, rot, rd, ne, fa) in enumerate(views):
        if i >= 2:
            ev.append({})
        r.render(c, rot, rd, ne, fa, marks=mark if i >= 2 else None, check_range=False, **kw)
    torch.cuda.synchronize()
    res = {n: float(np.median([e[n].elapsed_time(e[names[j + 1]]) for e in ev])) for j, n in enumerate(names[:-1])}
    res["agg"] = res.pop("agg_rows") + res.pop("agg_color")   # one call launches both kernels
    res["frame"] = float(np.median([e["query"].elapsed_time(e["end"]) for e in ev]))
    res["rays_per_s"] = 800 * 800 / res["frame"] * 1e3
    res.update(block3_layers=block3, bpnet=[nl, dim], frames=nf, path="rows-gemm" if rows else "plain-fp32")
    if rows:
        res.update(window_items=r.rows.ci, items=int(r.rows.counts[0]), rows=int(r.rows.counts[1]), on_path=r._rows_frame)
    print(json.dumps(res), flush=True)
