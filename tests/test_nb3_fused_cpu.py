"""The viewmlp without block3 on the fused split-fp16 row kernel (opts.rows_fused = 1), the parts that need no
GPU: the option and its refusals, from_opt, the command-line flags, the trainer's options, and the new entries'
sizes and argument checks."""
import argparse
import ctypes
import dataclasses

import pytest

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib
from sgnerf_amd.opts import HotPathOpts

NB3 = dict(shading_feature_mlp_layer3=0)


# ---- the option ------------------------------------------------------------------------------------------
def test_option_defaults_to_off():
    assert HotPathOpts().rows_fused == 0 and HotPathOpts(**NB3).rows_fused == 0
    HotPathOpts().check_supported()
    HotPathOpts(**NB3).check_supported()
    assert HotPathOpts(**NB3, rows_fused=1).check_supported().rows_fused == 1


@pytest.mark.parametrize("kw", [dict(rows_fused=1), dict(rows_fused=1, shading_feature_mlp_layer3=2),
                                dict(rows_fused=1, precision="f16", **NB3), dict(rows_fused=1, is_train=1, **NB3),
                                dict(rows_fused=1, rows_gemm=1, **NB3),
                                dict(rows_fused=2, **NB3), dict(rows_fused=-1, **NB3), dict(rows_fused=True, **NB3),
                                dict(rows_fused=1.0, **NB3), dict(rows_fused="1", **NB3)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_refusals_name_the_option(kw):
    """1 only for the viewmlp without block3, in f32, rendering, and not beside rows_gemm = 1; anything but the
    integers 0 / 1 is refused."""
    with pytest.raises(NotImplementedError, match="rows_fused"):
        HotPathOpts(**kw).check_supported()


def test_off_changes_no_refusal():
    """With 0 the other refusals read as before (no mention of the option), rows_gemm's among them."""
    assert HotPathOpts(**NB3).rows_fused == 0
    for kw in (dict(precision="f16", **NB3), dict(rows_gemm=1, is_train=1, **NB3), dict(rows_gemm=2, **NB3)):
        with pytest.raises(NotImplementedError) as e:
            HotPathOpts(**kw).check_supported()
        assert "rows_fused" not in str(e.value)


def test_from_opt():
    base = dict(shading_feature_mlp_layer3=0, SR=24)
    assert HotPathOpts.from_opt(argparse.Namespace(**base)).rows_fused == 0           # absent
    assert HotPathOpts.from_opt(argparse.Namespace(**base, rows_fused=None)).rows_fused == 0
    assert HotPathOpts.from_opt(argparse.Namespace(**base, rows_fused=0)).rows_fused == 0
    o = HotPathOpts.from_opt(argparse.Namespace(**base, rows_fused=1))
    assert o.rows_fused == 1 and o.check_supported() is o
    assert HotPathOpts.from_opt(argparse.Namespace(**base), rows_fused=1).rows_fused == 1   # an override
    with pytest.raises(NotImplementedError, match="rows_fused"):
        HotPathOpts.from_opt(argparse.Namespace(**base, rows_fused=1), is_train=1).check_supported()


def test_command_line_switches(monkeypatch):
    import torch
    from sgnerf_amd import render_vid
    from sgnerf_amd.model import HipPointsVolumetricModel
    p = HipPointsVolumetricModel.modify_commandline_options(argparse.ArgumentParser(), is_train=False)
    assert p.parse_args([]).sgn_rows_fused == 0 and p.parse_args(["--sgn_rows_fused", "1"]).sgn_rows_fused == 1
    assert p.parse_args([]).sgn_rows_gemm == 0                                       # its neighbour stays

    # render_vid: main() is run up to the options it builds from its own flags (no device is touched)
    class Stop(Exception):
        pass
    seen = []

    def opts(**kw):
        seen.append(kw)
        raise Stop
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(render_vid, "HotPathOpts", opts)
    for argv, want in (([], 0), (["--mlp_layer3", "0", "--rows_fused", "1"], 1), (["--rows_fused", "0"], 0)):
        with pytest.raises(Stop):
            render_vid.main(argv)
        assert seen[-1]["rows_fused"] == want and seen[-1]["rows_gemm"] == 0
    assert HotPathOpts(**{**seen[-2], "SR": 24}).check_supported().rows_fused == 1
    with pytest.raises(SystemExit):
        render_vid.main(["--rows_fused", "2"])


def test_plugin_reads_the_flag_and_the_namespace(tmp_path):
    """--sgn_rows_fused and a bare rows_fused in the driver's namespace both reach the renderer's options."""
    from sgnerf_amd.model import HipPointsVolumetricModel
    for kw, want in ((dict(sgn_rows_fused=1), 1), (dict(rows_fused=1), 1), (dict(), 0), (dict(sgn_rows_fused=0), 0)):
        m = HipPointsVolumetricModel()
        m.initialize(argparse.Namespace(SR=24, K=8, shading_feature_mlp_layer3=0, checkpoints_dir=str(tmp_path), **kw))
        assert m.opts.rows_fused == want and m.opts.is_train == 0
    # a training driver: the rendering options keep the knob (is_train = 0 there), the trainer's drop it
    m = HipPointsVolumetricModel()
    m.initialize(argparse.Namespace(SR=24, K=8, shading_feature_mlp_layer3=0, checkpoints_dir=str(tmp_path), is_train=True,
                                    rows_fused=1, train_rows=1))
    assert m.opts.rows_fused == 1 and m.opts.train_rows == 1 and m.is_train


def test_trainer_options_carry_rows_fused_0():
    """The plugin builds the trainer's options with rows_fused = 0 (as with rows_gemm): rendering options with the
    knob on turn into training options that check_supported accepts, and only with it cleared (the plugin's own
    trainer is held to rows_fused = 0 on the GPU, test_nb3_fused_gpu.py)."""
    o = HotPathOpts(**NB3, rows_fused=1, train_rows=1).check_supported()
    t = dataclasses.replace(o, is_train=1, rows_gemm=0, rows_fused=0).check_supported()
    assert t.rows_fused == 0 and t.is_train == 1 and t.train_rows == 1
    with pytest.raises(NotImplementedError, match="rows_fused"):
        dataclasses.replace(o, is_train=1).check_supported()


# ---- the C entries ---------------------------------------------------------------------------------------
NEW = ("sgn_mlp_packed_bytes_f32_nb3", "sgn_mlp_pack_f32_nb3", "sgn_point_project_f32_nb3", "sgn_aggregate_f32_nb3")


def test_entries_exported_and_abi():
    """Additions only: the new symbols exist with the stock entries' signatures, and the ABI number stays."""
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in _lib.SIGNATURES and hasattr(raw, n), n
    assert _lib.SIGNATURES["sgn_aggregate_f32_nb3"] == _lib.SIGNATURES["sgn_aggregate_f32"]
    assert _lib.SIGNATURES["sgn_point_project_f32_nb3"] == _lib.SIGNATURES["sgn_point_project_f32"]
    assert _lib.SIGNATURES["sgn_mlp_pack_f32_nb3"] == _lib.SIGNATURES["sgn_mlp_pack_exact_nb3"]
    assert _lib.lib().sgn_abi_version() == _lib.ABI_VERSION == 23


def test_packed_bytes():
    """The three variants share the stock layout (unused sections stay zero); an unknown variant has no blob."""
    L = _lib.lib()
    for nl, dim in ((0, 0), (1, 0), (1, 96)):
        n = int(L.sgn_mlp_packed_bytes_f32_nb3(nl, dim))
        assert n > 0 and n % 16 == 0 and n == int(L.sgn_mlp_packed_bytes_f32(nl, dim))
    assert int(L.sgn_mlp_packed_bytes_f32_nb3(2, 0)) == 0 and int(L.sgn_mlp_packed_bytes_f32_nb3(1, 32)) == 0


def test_argument_errors_are_reported_before_any_hip_call():
    """Pointers are never dereferenced: the checks come first (addresses that nothing could read)."""
    L = _lib.lib()
    A = 4096
    p = ctypes.c_void_p(A)
    pt = _lib.PointTables()
    for k in ("xyz", "embedding", "conf", "campos", "camrotc2w", "raydir"):   # colour and dir stay NULL
        setattr(pt, k, A)
    pt.n_points = 8
    qo = _lib.QueryOut()
    for k, _ in qo._fields_:
        setattr(qo, k, A)
    P, Q = ctypes.byref(pt), ctypes.byref(qo)

    def refused(rc, what, *words):
        assert rc != 0, what
        msg = L.sgn_last_error().decode()
        assert "invalid argument" in msg and all(w in msg for w in words), f"{what}: {msg}"

    ws = int(L.sgn_aggregate_workspace_bytes_f32(64))
    agg = L.sgn_aggregate_f32_nb3

    def call(nl=0, dim=0, bp=None, proj=p, pts=P, q=Q, S=64, K=8, packed=p, feat=p, wsp=p, nb=ws, stages=3):
        return agg(nl, dim, bp, proj, pts, q, S, K, packed, feat, None, None, wsp, nb, stages, None)

    for kw in (dict(proj=None), dict(pts=None), dict(q=None), dict(packed=None), dict(feat=None), dict(wsp=None)):
        refused(call(**kw), f"null {list(kw)[0]}", "null")
    refused(call(nl=2), "two block2_bpnet layers", "block2_bpnet")
    refused(call(nl=1, dim=32), "bpnet_dim 32", "block2_bpnet")
    refused(call(nl=1, dim=96), "no BPNet table", "bpnet_dim")
    refused(call(K=0), "K = 0", "K = 1 .. 8")
    refused(call(K=9), "K = 9", "K = 1 .. 8")
    refused(call(stages=0), "stages = 0", "stages")
    refused(call(stages=4), "stages = 4", "stages")
    pt.pers = pt.samp_pers = A
    refused(call(), "pers", "pers", "without block3")
    pt.pers = pt.samp_pers = None
    pt.rot = pt.samp_viewdir = A
    refused(call(), "rot", "rot", "without block3")
    pt.rot = pt.samp_viewdir = None
    refused(call(wsp=ctypes.c_void_p(A + 4)), "misaligned workspace", "alignment")
    refused(call(nb=int(L.sgn_aggregate_workspace_bytes_f32(32)) - 1072), "workspace under 32 items", "workspace too small")
    refused(call(stages=1, nb=int(L.sgn_aggregate_workspace_bytes_f32(32))), "stage 1 alone on a partial workspace",
            "stages 1 and 2 called separately")

    proj = L.sgn_point_project_f32_nb3
    refused(proj(None, p, None, None, p, None), "no tables", "null")
    refused(proj(P, None, None, None, p, None), "no blob", "null")
    refused(proj(P, p, None, None, None, None), "no projection buffer", "null")
    refused(proj(P, p, p, None, p, None), "list without count", "d_idx and d_count")
    refused(proj(P, p, None, None, ctypes.c_void_p(A + 4), None), "alignment", "alignment")
    pt.conf = None
    refused(proj(P, p, None, None, p, None), "no conf", "point tables")
    pt.conf = A
    # the stock entry still wants colour and dir
    refused(L.sgn_point_project_f32(P, p, None, None, p, None), "stock projection without colour / dir", "color")

    pack = L.sgn_mlp_pack_f32_nb3
    w8 = (ctypes.c_void_p * 8)(*([A] * 8))
    w7 = (ctypes.c_void_p * 8)(*([A] * 7 + [None]))
    refused(pack(0, 0, None, w8, p, None), "no weights", "null")
    refused(pack(0, 0, w8, w8, None, None), "no blob", "null")
    refused(pack(2, 0, w8, w8, p, None), "variant", "block2_bpnet")
    refused(pack(1, 0, w7, w8, p, None), "no block2_bpnet.0", "null layer")
