"""bench.py's own plumbing: the --dump-outputs files and the plain / --full split of the result line."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import bench


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """Arrays within their share of the byte budget are written whole (as float32); a larger one is cut
    to a row sample that is the same in every call, rows in ascending order."""
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    big = torch.rand(1000, 8, generator=torch.Generator().manual_seed(0))   # 32,000 B, over any share
    arrays = {"big": big, "mask": torch.arange(10, dtype=torch.int8), "scalar": torch.tensor(2.5, dtype=torch.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "mask.npy", "scalar.npy"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 4000
    assert np.array_equal(got["mask"], np.arange(10, dtype=np.float32))
    assert got["scalar"].reshape(-1).tolist() == [2.5]
    # every dumped row is a row of the input, taken in ascending order (first column: distinct values)
    assert got["big"].shape[1:] == (8,) and 100 <= got["big"].shape[0] < 1000
    col = big[:, 0].numpy()
    rows = [int(np.flatnonzero(col == v)[0]) for v in got["big"][:, 0]]
    assert rows == sorted(set(rows))
    assert np.array_equal(got["big"], big.numpy()[rows])
    for n in arrays:
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy"))


def test_options_default_to_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out_dir"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out_dir"


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, monkeypatch, capsys):
    """A plain run on a small frame: the result line holds the headline fields and none of --full's, the
    timed step count is --steps, and the last step's four outputs are written in float32."""
    h, w, sr = 48, 40, 64
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--h", str(h),
                                      "--w", str(w), "--points", "50000", "--dump-outputs", str(tmp_path / "d")])
    bench.main()
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["metric"] == bench.METRIC and res["unit"] == "rays/s" and res["higher_is_better"] is True
    assert res["steps"] == 3 and res["warmup"] == 1 and res["dtype"].startswith("f32")
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(h * w / (res["ms_per_step"] * 1e-3), rel=1e-6)
    assert set(res["stages_ms"]) == {"query", "proj", "agg_rows", "agg_color", "composite"}
    for k in ("roofline", "roofline_query", "occupancy", "grid_rebuild_ms", "f16_mode", "train_config5", "lego",
              "cpu_baseline"):
        assert k not in res, k
    R = h * w
    shapes = {"rgb": (R, 3), "ray_mask": (R,), "bg_transmission": (R,), "coarse_point_opacity": (R, sr)}
    assert sorted(os.listdir(tmp_path / "d")) == sorted(n + ".npy" for n in shapes)
    out = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in shapes}
    for n, a in out.items():
        assert a.dtype == np.float32 and a.shape == shapes[n] and np.isfinite(a).all(), n
    assert set(np.unique(out["ray_mask"])) <= {0.0, 1.0} and out["ray_mask"].sum() > 0
    # colours are sigmoid(x) * 1.002 - 0.001, blended with weights that sum to one (white background)
    assert out["rgb"].min() >= -2e-3 and out["rgb"].max() <= 1.0 + 2e-3
    assert out["coarse_point_opacity"].max() > 0.0
