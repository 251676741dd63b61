"""The viewmlp without block3 on the split-fp16 row GEMMs (opts.rows_gemm = 1), the parts that need no GPU: the
option and its refusals, from_opt, the window planner as a pure function, and the new entries' argument checks."""
import argparse
import ctypes

import pytest

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib, rows_gemm as rg
from sgnerf_amd.opts import HotPathOpts

NB3 = dict(shading_feature_mlp_layer3=0)


# ---- the option ------------------------------------------------------------------------------------------
def test_option_defaults_to_off():
    assert HotPathOpts().rows_gemm == 0 and HotPathOpts(**NB3).rows_gemm == 0
    HotPathOpts().check_supported()
    HotPathOpts(**NB3).check_supported()
    assert HotPathOpts(**NB3, rows_gemm=1).check_supported().rows_gemm == 1


@pytest.mark.parametrize("kw", [dict(rows_gemm=1), dict(rows_gemm=1, shading_feature_mlp_layer3=2),
                                dict(rows_gemm=1, precision="f16", **NB3), dict(rows_gemm=1, is_train=1, **NB3),
                                dict(rows_gemm=2, **NB3), dict(rows_gemm=-1, **NB3), dict(rows_gemm=True, **NB3),
                                dict(rows_gemm=1.0, **NB3), dict(rows_gemm="1", **NB3)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_refusals_name_the_option(kw):
    """1 only for the viewmlp without block3, in f32, rendering; anything but 0 / 1 is refused."""
    with pytest.raises(NotImplementedError, match="rows_gemm"):
        HotPathOpts(**kw).check_supported()


def test_off_changes_no_refusal():
    """With 0 the other refusals read as before (no mention of the option)."""
    with pytest.raises(NotImplementedError) as e:
        HotPathOpts(precision="f16", **NB3).check_supported()
    assert "rows_gemm" not in str(e.value)


def test_from_opt():
    base = dict(shading_feature_mlp_layer3=0, SR=24)
    assert HotPathOpts.from_opt(argparse.Namespace(**base)).rows_gemm == 0           # absent
    assert HotPathOpts.from_opt(argparse.Namespace(**base, rows_gemm=None)).rows_gemm == 0
    assert HotPathOpts.from_opt(argparse.Namespace(**base, rows_gemm=0)).rows_gemm == 0
    o = HotPathOpts.from_opt(argparse.Namespace(**base, rows_gemm=1))
    assert o.rows_gemm == 1 and o.check_supported() is o
    assert HotPathOpts.from_opt(argparse.Namespace(**base), rows_gemm=1).rows_gemm == 1   # an override
    with pytest.raises(NotImplementedError, match="rows_gemm"):
        HotPathOpts.from_opt(argparse.Namespace(**base, rows_gemm=1), is_train=1).check_supported()


def test_command_line_switches():
    from sgnerf_amd.model import HipPointsVolumetricModel
    p = HipPointsVolumetricModel.modify_commandline_options(argparse.ArgumentParser(), is_train=False)
    assert p.parse_args([]).sgn_rows_gemm == 0 and p.parse_args(["--sgn_rows_gemm", "1"]).sgn_rows_gemm == 1


# ---- the window planner ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ci,want", [(0, 4, []), (1, 4, [(0, 1)]), (4, 4, [(0, 4)]), (5, 4, [(0, 4), (4, 1)]),
                                       (9, 1, [(i, 1) for i in range(9)]), (17, 7, [(0, 7), (7, 7), (14, 3)]),
                                       (3, 1 << 20, [(0, 3)])])
def test_plan_windows(n, ci, want):
    """Item count 0, 1, exactly CI, CI + 1; windows in list order, every one at most CI items, all items once."""
    got = rg.plan_windows(n, ci)
    assert got == want
    assert sum(k for _, k in got) == n and all(1 <= k <= ci for _, k in got)
    assert [i for i, _ in got] == list(range(0, n, ci))


def test_plan_windows_refuses_an_empty_window():
    with pytest.raises(ValueError):
        rg.plan_windows(5, 0)


@pytest.mark.parametrize("K", [1, 4, 5, 8])
def test_default_window_stays_below_the_gemm_limit(K):
    """K = 1 and K = 8: a default window's widest operand (x0, 288 floats per row) stays below 2 GiB, and at
    most 1 M rows; the limit itself is what sgn_x3_gemm refuses at (M ld 4 < 2^31 - 1)."""
    ci = rg.default_ci(K)
    rows = ci * K
    assert ci >= 1 and rows <= rg.ROWS_DEFAULT and rows * rg.X0_LD * 4 < 0x7fffffff
    assert rows + K > rg.ROWS_DEFAULT            # and no smaller than it has to be
    lim = rg.max_window_rows()
    assert lim * rg.X0_LD * 4 < 0x7fffffff <= (lim + 1) * rg.X0_LD * 4 and 1_800_000 < lim < 1_900_000
    assert rg.check_ci(lim // K, K) == lim // K
    with pytest.raises(ValueError, match="rows_gemm"):
        rg.check_ci(lim // K + 1, K)
    with pytest.raises(ValueError, match="rows_gemm"):
        rg.check_ci(0, K)


def test_row_layers_are_the_network_without_block3():
    names = [n for n, *_ in rg.row_layers((1, 96))]
    assert names == ["block1.0", "block1.2", "alpha_branch.0", "color_branch.0", "color_branch.2", "color_branch.4",
                     "color_branch.6", "block2_bpnet.0"]
    assert [n for n, *_ in rg.row_layers((0, 0))] == names[:-1]


# ---- the C entries ---------------------------------------------------------------------------------------
def test_entries_exported_and_abi():
    """Additions only: the new symbols exist, no existing struct or signature moved, so the ABI number stays."""
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("sgn_rows_windows", "sgn_rows_inputs_nb3", "sgn_rows_gather_nb3", "sgn_rows_blend_nb3",
              "sgn_x3_gemm_accumulate"):
        assert n in _lib.SIGNATURES and hasattr(raw, n), n
    assert _lib.SIGNATURES["sgn_x3_gemm_accumulate"] == _lib.SIGNATURES["sgn_x3_gemm"]
    assert _lib.lib().sgn_abi_version() == _lib.ABI_VERSION
    assert [f for f, _ in _lib.X3GemmArgs._fields_][-1] == "bpack"


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

    win = L.sgn_rows_windows
    refused(win(Q, 9, p, p, 4, 1, p, None), "K = 9", "K = 1 .. 8")
    refused(win(Q, 8, p, p, 0, 1, p, None), "ci = 0", "ci >= 1")
    refused(win(Q, 8, p, p, 4, 0, p, None), "no window", "n_win >= 1")
    refused(win(Q, 8, p, p, 1 << 28, 1, p, None), "ci K too large", "ci K < 2^30")
    refused(win(Q, 8, p, p, 4, 1, None, None), "no words", "null")
    refused(win(Q, 8, None, p, 4, 1, p, None), "no row offsets", "null")

    inp = L.sgn_rows_inputs_nb3
    refused(inp(P, Q, 0, p, p, 0, 4, p, p, p, None), "K = 0", "K = 1 .. 8")
    refused(inp(P, Q, 9, p, p, 0, 4, p, p, p, None), "K = 9", "K = 1 .. 8")
    refused(inp(P, Q, 8, p, p, -1, 4, p, p, p, None), "item0 < 0", "item window")
    refused(inp(P, Q, 8, p, p, 0, 0, p, p, p, None), "n_items = 0", "item window")
    refused(inp(P, Q, 8, p, None, 0, 4, p, p, p, None), "no window words", "null")
    refused(inp(P, Q, 8, p, p, 0, 4, None, p, p, None), "no x0", "null")
    refused(inp(P, Q, 8, p, p, 0, 4, ctypes.c_void_p(A + 4), p, p, None), "x0 alignment", "aligned")
    pt.rot = A
    refused(inp(P, Q, 8, p, p, 0, 4, p, p, p, None), "rotated points", "rot")
    pt.rot = None
    pt.pers = A
    refused(inp(P, Q, 8, p, p, 0, 4, p, p, p, None), "pers", "pers")
    pt.pers = None
    pt.conf = None
    refused(inp(P, Q, 8, p, p, 0, 4, p, p, p, None), "no conf", "point table")
    pt.conf = A

    gat = L.sgn_rows_gather_nb3
    refused(gat(Q, 8, p, p, 0, 4, p, 95, p, None), "dim % 4", "dim % 4 == 0")
    refused(gat(Q, 8, p, p, 0, 4, None, 96, p, None), "no table", "null")
    refused(gat(Q, 0, p, p, 0, 4, p, 96, p, None), "K = 0", "K = 1 .. 8")

    bl = L.sgn_rows_blend_nb3
    refused(bl(Q, 8, p, p, 0, 4, p, p, p, p, p, p, None, None, None, None), "no flag word", "null")
    refused(bl(Q, 8, p, p, 0, 4, None, p, p, p, p, p, None, None, p, None), "no z", "null")
    refused(bl(Q, 9, p, p, 0, 4, p, p, p, p, p, p, None, None, p, None), "K = 9", "K = 1 .. 8")
    refused(bl(Q, 8, p, p, 0, 4, ctypes.c_void_p(A + 4), p, p, p, p, p, None, None, p, None), "z alignment", "aligned")
    refused(bl(Q, 8, p, p, 1 << 30, 4, p, p, p, p, p, p, None, None, p, None), "item0 too large", "item window")

    # the accumulate entry: rows mode only, one plain operand a, no mask / out2, K <= 128, 128-wide column blocks
    def gemm(**kw):
        g = _lib.X3GemmArgs()
        g.a.p, g.a.ld, g.a.csplit, g.a.ncols, g.a.ones_col = A, 96, 96, 96, -1
        g.b.p, g.b.ld, g.b.csplit, g.b.ncols, g.b.ones_col = A, 352, 96, 96, -1
        g.mode, g.M, g.N, g.K, g.out, g.ldo, g.out_cols = 0, 64, 256, 96, A, 256, 256
        for k, v in kw.items():
            obj, _, f = k.rpartition("__")
            setattr(getattr(g, obj) if obj else g, f, v)
        return ctypes.byref(g)
    acc = L.sgn_x3_gemm_accumulate
    refused(acc(gemm(mode=1), None), "split-K", "accumulate")
    refused(acc(gemm(mask=A, ldm=256), None), "mask", "accumulate")
    refused(acc(gemm(out2=A, ldo2=64, out_cols=192), None), "out2", "accumulate")
    refused(acc(gemm(a__act=1), None), "activation", "accumulate")
    refused(acc(gemm(K=256, a__ncols=256, a__csplit=256, a__ld=256), None), "K = 256", "accumulate")
    refused(acc(gemm(N=96), None), "96-wide blocks", "accumulate")
    refused(acc(None, None), "null", "null")
