"""GPU time per training step of the viewmlp without block3 (opts.train_rows = 1, train_f32.F32StepNb3) next to
the stock fp32 step, on bench.py's config-5 batches (NOT product): 4096 random rays of a random spiral pose, SR 24,
K 8, synth-room with 1.2 M points.  Every HipTrainer.step between two HIP events; prints one JSON line per network
with the median ms per step.  For the per-kernel split run one network under `rocprofv3 --kernel-trace --stats`.
    python tools/train_nb3_step_time.py [steps] [warmup] [base|bp352|stock ...]"""
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from bench import pose_view  # noqa: E402  (config 5's spiral poses: bench.py's public workload definition)
from sgnerf_amd import scene  # noqa: E402
from sgnerf_amd.opts import HotPathOpts  # noqa: E402
from sgnerf_amd.querier import LightningFastQuerier  # noqa: E402
from sgnerf_amd.train import PointParams  # noqa: E402
from sgnerf_amd.train_hip import HipTrainer  # noqa: E402
from sgnerf_amd.weights import init_mlp  # noqa: E402

sys_args = sys.argv[1:]
steps = int(sys_args[0]) if len(sys_args) > 0 else 20
warmup = int(sys_args[1]) if len(sys_args) > 1 else 5
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
POINTS, H, W, RAYS = 1_200_000, 800, 800, 4096   # bench.py --train's workload (config 5)
SG = dict(shading_feature_mlp_layer2_bpnet=1, predict_semantic=1, semantic_guidance=1)
NB3 = dict(shading_feature_mlp_layer3=0, train_rows=1)
pc = scene.with_semantics(scene.synth_room(POINTS, seed=0), seed=1, n_classes=20, cell=0.5)


def ray_labels(o, campos, raydir):
    """A stand-in for BPNet's per-pixel labels, as bench.py --sg makes it: the label of the first neighbour of each
    ray's first occupied sample under the plain query; (point_labels, ray_labels, seconds)."""
    q = LightningFastQuerier(dev, dataclasses.replace(o, semantic_guidance=0)).query_samples(
        torch.from_numpy(pc.xyz).to(dev), campos, raydir, 0.1, 8.0)
    S, R = q.n_samples(), raydir.shape[0]
    pl = torch.from_numpy(pc.labels).to(dev)
    ok = q.samp_nnb[:S] > 0
    first = torch.full((R,), S, dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, q.samp_ray[:S].long()[ok], torch.arange(S, device=dev)[ok], reduce="amin")
    has = first < S
    rl = torch.zeros(R, dtype=torch.int32, device=dev)
    rl[has] = pl[q.pidx[first[has] * o.K].long()]
    return pl, rl.contiguous(), 12


def run(name, opts, block3, sg):
    mlp = init_mlp(0, bias_std=0.01, bpnet_layers=1 if sg else 0, bpnet_dim=96 if sg else 0, block3_layers=block3)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + 50.0
    points = PointParams(pc.xyz, pc.embedding, pc.color, pc.dir, pc.conf, dev)
    tr = HipTrainer(points, mlp, opts, dev, bpnet=pc.bpnet if sg else None, precision="f32")
    g = torch.Generator().manual_seed(1)
    batches = []
    for _ in range(warmup + steps):
        v = pose_view(int(torch.randint(0, 120, (1,), generator=g)), H, W)
        idx = torch.randint(0, H * W, (RAYS,), generator=g)
        gt = torch.rand(RAYS, 3, generator=g)
        b = tuple(x.to(dev) for x in (torch.from_numpy(v.campos), torch.from_numpy(v.camrotc2w),
                                      torch.from_numpy(v.raydir)[idx], gt))
        lab = ray_labels(opts, b[0], b[2]) if sg else None
        batches.append((b, lab))
    tr.querier = None
    ev = []
    for i, ((c, r, d, gt), lab) in enumerate(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        parts, _, _ = tr.step(c, r, d, 0.1, 8.0, gt, labels=lab)
        e1.record()
        if i >= warmup:
            ev.append((e0, e1))
    torch.cuda.synchronize()
    tr.check_touched()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    print(json.dumps({"step": name, "rays": RAYS, "steps": steps, "warmup": warmup,
                      "gpu_ms_per_step_median": ms[len(ms) // 2], "gpu_ms_per_step_min": ms[0],
                      "gpu_ms_per_step_max": ms[-1], "loss_total_last": float(parts["total"])}), flush=True)
    del tr, points
    torch.cuda.empty_cache()


RUNS = {"base": ("train_rows base (no block3)", HotPathOpts(SR=24, is_train=1, **NB3), 0, False),
        "bp352": ("train_rows bp352 (no block3, block2_bpnet on 352 inputs)", HotPathOpts(SR=24, is_train=1, **NB3, **SG), 0, True),
        "stock": ("stock f32 (block3)", HotPathOpts(SR=24, is_train=1), 2, False)}
for which in sys_args[2:] or list(RUNS):
    run(*RUNS[which])
