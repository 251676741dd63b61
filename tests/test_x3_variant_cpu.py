"""tools/x3_variant.py builds its experiment variants by exact-text patches into mlp_x3.hip and
train_x3.hip: every patch it lists must still find its anchors in the tree's sources (nothing is
compiled here)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sg-nerf_amd", "csrc")

_spec = importlib.util.spec_from_file_location("x3_variant", os.path.join(ROOT, "tools", "x3_variant.py"))
x3_variant = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(x3_variant)

CASES = [("mlp_x3.hip", "patch", p) for p in x3_variant.MLP_PATCHES] + \
        [("train_x3.hip", "patch_tx", p) for p in x3_variant.TX_PATCHES]


@pytest.fixture(scope="module")
def sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in ("mlp_x3.hip", "train_x3.hip")}


def test_patch_lists():
    names = x3_variant.MLP_PATCHES + x3_variant.TX_PATCHES
    assert len(names) == len(set(names)) > 0
    for p in names:
        assert p in x3_variant.__doc__, f"{p} is missing from the tool's docstring"
    for fn in (x3_variant.patch, x3_variant.patch_tx):
        with pytest.raises(SystemExit):
            fn("", "no_such_patch")
    with pytest.raises(SystemExit):   # each list belongs to its own file
        x3_variant.patch("", x3_variant.TX_PATCHES[0])
    with pytest.raises(SystemExit):
        x3_variant.patch_tx("", x3_variant.MLP_PATCHES[0])


@pytest.mark.parametrize("src,fn,name", CASES, ids=[c[2] for c in CASES])
def test_patch_applies(sources, src, fn, name):
    out = getattr(x3_variant, fn)(sources[src], name)   # a missing anchor raises SystemExit
    assert isinstance(out, str) and out != sources[src]
