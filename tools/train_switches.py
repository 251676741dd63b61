"""Config-5 training step time under a set of frozen point tensors (opt.feat_grad / color_grad / dir_grad /
conf_grad = 0): bench.py's --train workload (its train_main, untouched) with the switches set on the
HotPathOpts it builds.  DESIGN.md §3.5's frozen rows come from here.

    python tools/train_switches.py --frozen dir --precision f32 [--steps 30 --warmup 5] [--sg]
    --frozen: comma list of feat, color, dir, conf (empty: all trained, the same run as bench.py --train)

Prints one JSON line: frozen, precision, ms_per_step, final_loss."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from sgnerf_amd.opts import HotPathOpts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frozen", default="")
    ap.add_argument("--precision", choices=["f32", "f16"], default="f32")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sg", action="store_true")
    a = ap.parse_args()
    frozen = [k for k in a.frozen.split(",") if k]
    off = {k + "_grad": 0 for k in frozen}
    # train_main builds its options as bench.HotPathOpts(...): that name is replaced by a factory that adds the
    # switches.  Should train_main ever build them another way, the check after the run fails instead of timing
    # an all-trained step under a frozen label.
    made = []

    def with_switches(**kw):
        made.append(HotPathOpts(**kw, **off))
        return made[-1]
    bench.HotPathOpts = with_switches
    args = argparse.Namespace(steps=a.steps, warmup=a.warmup, train_precision=a.precision, sg=a.sg, train_torch=False,
                              points=1_200_000, h=800, w=800, train_rays=4096)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = bench.train_main(args, 1, 0, dev, False)
    if not made or any(getattr(made[-1], k) != 0 for k in off):
        raise SystemExit("bench.train_main did not build its options through bench.HotPathOpts: the switches were not set")
    loss = res.get("final_loss")
    print(json.dumps({"frozen": frozen, "precision": a.precision, "sg": a.sg, "ms_per_step": res["ms_per_step"],
                      "final_loss": None if loss is None else float(loss)}))


if __name__ == "__main__":
    main()
