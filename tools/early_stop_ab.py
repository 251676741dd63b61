"""A/B of early ray termination on config-2 frames (the room, 1.2 M points, 800x800, SR 64,
init_mlp(0, bias_std=0.01)): one process renders the same frame with early_stop = 0 and early_stop = EPS,
alternating, for alpha-bias offsets 0, 50, 500 and 5000.  At offset 0 nothing terminates: that line is the
pure cost of tiering.  Per offset: the share of work items skipped, ms per frame of both runs (median and
min of HIP-event times), the tier kernels' time per frame (the frame's sgn_early_stop_tier calls replayed
alone between two events) and max |rgb - full|.

Usage (GPU box): python tools/early_stop_ab.py [--rounds 12] [--eps 1e-3] [--slots 4,8,16] [--precision f32]
                                               [--offsets 0,50,500,5000] [--out bench_out/early_stop_ab.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sgnerf_amd  # noqa: E402,F401
from sgnerf_amd import _lib, scene  # noqa: E402
from sgnerf_amd.opts import HotPathOpts  # noqa: E402
from sgnerf_amd.render import HipRenderer, PointTables  # noqa: E402
from sgnerf_amd.weights import init_mlp  # noqa: E402


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def tier_kernels_ms(r, campos, rot, R, q):
    """The frame's sgn_early_stop_tier calls alone, replayed on the renderer's buffers (idempotent: the same
    work lists, zeros and counters are written again)."""
    o = r.opts
    cp = _lib.CompositeParams()
    cp.SR, cp.vsize_z, cp.raydist_mode_unit = o.SR, float(o.vsize[2]), o.raydist_mode_unit
    work, counters, stop_slot, _ = r.es
    qo = q.abi()
    L, st = _lib.lib(), _lib.stream_handle()

    def run():
        for t, (lo, hi) in enumerate(o.early_stop_tiers):
            _lib.check(L.sgn_early_stop_tier(ctypes.byref(cp), _lib.ptr(campos), _lib.ptr(rot), R, ctypes.byref(qo),
                                             _lib.ptr(r.feat), lo, hi, float(o.early_stop), R * o.SR, _lib.ptr(work),
                                             _lib.ptr(counters[t]), _lib.ptr(counters[t - 1]) if t else None,
                                             _lib.ptr(stop_slot), st), "sgn_early_stop_tier")
    run()
    return statistics.median(timed(run)[0] for _ in range(5))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--slots", default="4,8,16")
    ap.add_argument("--precision", default="f32", choices=["f32", "f16"])
    ap.add_argument("--offsets", default="0,50,500,5000")
    ap.add_argument("--points", type=int, default=1_200_000)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(os.environ.get("SGN_OUT", "bench_out"), "early_stop_ab.txt"))
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    slots = tuple(int(x) for x in args.slots.split(",") if x)
    base = HotPathOpts(SR=64, precision=args.precision)
    on = HotPathOpts(SR=64, precision=args.precision, early_stop=args.eps, early_stop_slots=slots)
    pc = scene.synth_room(args.points, seed=0)
    tab = PointTables.from_cloud(pc, dev)
    yaw, pitch = scene.spiral_yaw_pitch(0, 120)
    v = scene.room_view(args.hw, args.hw, yaw=yaw + 15.0, pitch=pitch - 5.0)
    cam = (torch.from_numpy(v.campos).to(dev), torch.from_numpy(v.camrotc2w).to(dev), torch.from_numpy(v.raydir).to(dev))
    R = cam[2].shape[0]
    lines = [f"early_stop A/B: room {args.points} points, {args.hw}x{args.hw} rays, SR 64, precision {args.precision}, "
             f"eps {args.eps:g}, slots {slots}, {args.rounds} alternating rounds (median / min ms per frame)"]
    print(lines[0], flush=True)
    for off in (float(x) for x in args.offsets.split(",")):
        mlp = init_mlp(0, bias_std=0.01)
        mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + off
        ra, rb = HipRenderer(tab, mlp, base, dev), HipRenderer(tab, mlp, on, dev)
        frame = lambda r: r.render(*cam, v.near, v.far, want_opacity=False, check_range=False)   # noqa: E731
        for r in (ra, rb, ra, rb):
            frame(r)
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(lambda: frame(ra))[0])
            ms, out = timed(lambda: frame(rb))
            tb.append(ms)
        full = frame(ra).rgb.clone()
        out = frame(rb)
        torch.cuda.synchronize()
        items = int(out.query.counters[1])
        tiers = out.tiers.cpu().numpy()
        err = float((out.rgb - full).abs().max())
        tk = tier_kernels_ms(rb, cam[0], cam[1], R, out.query)
        line = (f"alpha bias +{off:g}: {items} work items, skipped {int(out.skipped)} ({100.0 * int(out.skipped) / max(items, 1):.1f} %), "
                f"items per tier {tiers[:, 1].tolist()}; full {statistics.median(ta):.2f} / {min(ta):.2f} ms, "
                f"early_stop {statistics.median(tb):.2f} / {min(tb):.2f} ms, tier kernels {tk:.3f} ms, "
                f"max |rgb - full| {err:.2e}")
        print(line, flush=True)
        lines.append(line)
        del ra, rb
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
