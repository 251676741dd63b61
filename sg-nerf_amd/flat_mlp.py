"""The aggregator MLP as one flat fp32 parameter (LAYERS order) and the device-side packers that
rebuild the MFMA weight blobs from it every step by index gathers (sgn_gather_segments /
sgn_pack_scaled_f32)."""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .weights import LAYERS, strip_prefix

N_F32 = 2056


class FlatMLP(nn.Module):
    """The 9 viewmlp layers (+ SG's block2_bpnet.0 after them) in one flat fp32 parameter: per
    layer weight (row-major) then bias."""

    def __init__(self, state, device, layers=LAYERS):
        super().__init__()
        self.layers = list(layers)
        # a layer list without block3.* is the viewmlp without block3 (weights.layers_for(block3_layers=0))
        state = strip_prefix(state, block3_layers=2 if any(n.startswith("block3.") for n, *_ in self.layers) else 0)
        parts, self.slices, off = [], {}, 0
        for name, o, i, _ in self.layers:
            parts += [torch.as_tensor(state[name + ".weight"]).float().reshape(-1),
                      torch.as_tensor(state[name + ".bias"]).float().reshape(-1)]
            self.slices[name] = (off, o, i)
            off += o * i + o
        self.flat = nn.Parameter(torch.cat(parts).to(device))

    def w(self, name, t=None):
        off, o, i = self.slices[name]
        return (self.flat if t is None else t)[off:off + o * i].view(o, i)

    def b(self, name, t=None):
        off, o, i = self.slices[name]
        return (self.flat if t is None else t)[off + o * i:off + o * i + o]

    def f(self, name, x):
        return F.linear(x, self.w(name), self.b(name))

    def state(self):
        out = {}
        for name, *_ in self.layers:
            out[name + ".weight"] = self.w(name).detach().clone()
            out[name + ".bias"] = self.b(name).detach().clone()
        return out


class _PackerF32:
    """Device-side packing of the fp32-faithful blob (mlp_x3.hip: (hi, lo) fp16 fragment pairs of
    2^s-scaled weights + the fp32 section) from the flat parameter, through the layout's index maps
    (sgn_mlp_pack_index_f32): per layer the shift s = 14 - e with max |W| = f 2^e (frexp), as
    layer_shift does on the host, then hi = fp16(2^s w), lo = fp16(2^s w - hi).  Equals
    weights.pack_mlp(state, precision="f32") bit for bit (tests/test_train_gpu.py)."""

    YK_ZERO, YK_W, YK_B, YK_BS, YK_INV, YK_ONE, YK_WINV = range(7)

    def __init__(self, device, mlp: "FlatMLP", variant=(0, 0), shifts_only=False):
        """shifts_only: a layer list k_rows16 has no blob for (the viewmlp without block3): `pack` writes the
        per-layer shifts the split-fp16 GEMMs read and nothing else (sgn_pack_scaled_f32 without sections, the call
        rows_gemm.RowsGemmNb3 makes once per weight set), and returns None."""
        L = _lib.lib()
        self.shifts_only = bool(shifts_only)
        if self.shifts_only:
            nl = self.n_layers = len(mlp.layers)
            assert nl <= 16
            self.woff = (ctypes.c_int64 * nl)(*[mlp.slices[n][0] for n, *_ in mlp.layers])
            self.wlen = (ctypes.c_int64 * nl)(*[mlp.slices[n][1] * mlp.slices[n][2] for n, *_ in mlp.layers])
            self.shift = torch.zeros(16, dtype=torch.int32, device=device)
            self.blob = None
            return
        self.n16b = int(L.sgn_mlp_layout_f32(0))
        n32 = int(L.sgn_mlp_layout_f32(1))
        self.total = int(L.sgn_mlp_packed_bytes_f32(*variant))

        def imap(which, n):
            a = (ctypes.c_int32 * n)()
            _lib.check(L.sgn_mlp_pack_index_f32(*variant, which, a, n), "sgn_mlp_pack_index_f32")
            return torch.frombuffer(bytearray(a), dtype=torch.int32).long()
        # the maps are decoded and bounds-checked on the host; the device only gathers
        nl, nflat = len(mlp.layers), mlp.flat.numel()
        woff = torch.tensor([mlp.slices[n][0] for n, *_ in mlp.layers], dtype=torch.long)
        wlen = torch.tensor([mlp.slices[n][1] * mlp.slices[n][2] for n, *_ in mlp.layers], dtype=torch.long)
        blen = torch.tensor([mlp.slices[n][1] for n, *_ in mlp.layers], dtype=torch.long)
        self.wspan = [(int(a), int(a + b)) for a, b in zip(woff, wlen)]
        c16 = imap(0, self.n16b // 2)
        v16 = c16 >= 0
        c16 = torch.clamp(c16, min=0)
        l16 = (c16 >> 20) & 0x3FF
        assert int(l16[v16].max()) < nl, "fragment map names a layer the flat parameter lacks"
        l16 = torch.where(v16, l16, 0)
        e16 = torch.where(v16, c16 & 0xFFFFF, 0)
        assert bool((e16 < wlen[l16]).all()), "fragment map element out of range"
        c32 = imap(1, n32)
        k32 = c32 >> 26
        l32 = (c32 >> 20) & 63
        e32 = c32 & 0xFFFFF
        uses_w = (k32 == self.YK_W) | (k32 == self.YK_WINV)
        uses_b = (k32 == self.YK_B) | (k32 == self.YK_BS)
        uses_l = uses_w | uses_b | (k32 == self.YK_INV)
        assert int(l32[uses_l].max()) < nl, "fp32 map names a layer the flat parameter lacks"
        l32 = torch.where(uses_l, l32, 0)
        fw32 = torch.where(uses_w, woff[l32] + e32, 0)
        fb32 = torch.where(uses_b, woff[l32] + wlen[l32] + e32, 0)
        assert bool((e32[uses_w] < wlen[l32[uses_w]]).all() and (e32[uses_b] < blen[l32[uses_b]]).all())
        f16 = woff[l16] + e16
        assert int(f16.max()) < nflat and int(fw32.max()) < nflat and int(fb32.max()) < nflat
        assert nflat < (1 << 22) and nl <= 16 and int(k32.max()) <= self.YK_WINV
        # one int32 code per blob element for sgn_pack_scaled_f32: flat index | layer << 22 | lo / kind << 26
        code16 = torch.where(v16, f16 | (l16 << 22) | (((c16 >> 30) & 1) << 26), -1)
        code32 = torch.where(uses_w, fw32, fb32) | (l32 << 22) | (k32 << 26)
        self.code16 = code16.to(torch.int32).to(device)
        self.code32 = code32.to(torch.int32).to(device)
        self.n_layers = nl
        self.woff = (ctypes.c_int64 * nl)(*[int(a) for a, _ in self.wspan])
        self.wlen = (ctypes.c_int64 * nl)(*[int(b - a) for a, b in self.wspan])
        self.shift = torch.zeros(16, dtype=torch.int32, device=device)
        self.blob = torch.zeros(self.total, dtype=torch.uint8, device=device)
        assert self.n16b == 2 * self.code16.numel() and self.n16b + 4 * self.code32.numel() <= self.total

    def pack(self, flat):
        """Per-layer shifts and both blob sections from the flat parameter: two launches."""
        flat = flat.detach()
        assert flat.is_contiguous() and flat.dtype == torch.float32
        if self.shifts_only:   # one launch, no host read: the weights change every step
            _lib.check(_lib.lib().sgn_pack_scaled_f32(_lib.ptr(flat), flat.numel(), self.n_layers, self.woff, self.wlen,
                                                      None, 0, None, 0, _lib.ptr(self.shift), None, None,
                                                      _lib.stream_handle()), "sgn_pack_scaled_f32 (shifts)")
            return None
        _lib.check(_lib.lib().sgn_pack_scaled_f32(
            _lib.ptr(flat), flat.numel(), self.n_layers, self.woff, self.wlen, _lib.ptr(self.code16), self.code16.numel(),
            _lib.ptr(self.code32), self.code32.numel(), _lib.ptr(self.shift), _lib.ptr(self.blob[:self.n16b]),
            _lib.ptr(self.blob[self.n16b:]), _lib.stream_handle()), "sgn_pack_scaled_f32")
        return self.blob


class _Packer:
    """Device-side re-packing of the forward and transposed MFMA blobs from the flat weights
    (variant (1, bpnet_dim): the SG blob, block2_bpnet.0's fragments and bias after the base)."""

    def __init__(self, device, variant=(0, 0)):
        L = _lib.lib()
        self.variant = variant
        self.base = int(L.sgn_mlp_section(2))
        self.total = int(L.sgn_mlp_packed_bytes(*variant))
        self.off_f32 = int(L.sgn_mlp_section(0))
        self.off_split = int(L.sgn_mlp_section(1))
        self.tbytes = int(L.sgn_train_tblob_bytes())

        def imap(fn, name, *args, n):
            """The layout's index map (flat index + 1, 0 = zero) as flat indices (-1 = zero)."""
            a = (ctypes.c_int32 * n)()
            _lib.check(fn(*variant, *args, a, n), name)
            return (torch.frombuffer(bytearray(a), dtype=torch.int32) - 1).to(device)
        self.i16 = imap(L.sgn_mlp_pack_index, "sgn_mlp_pack_index", 0, n=self.off_f32 // 2)
        self.i32 = imap(L.sgn_mlp_pack_index, "sgn_mlp_pack_index", 1, n=N_F32)
        self.isp = imap(L.sgn_mlp_pack_index, "sgn_mlp_pack_index", 2, n=(self.base - self.off_split) // 2)
        if variant != (0, 0):
            self.off_bb = self.total - 4 * 256                   # block2_bpnet bias (fp32, acc order)
            self.iwb = imap(L.sgn_mlp_pack_index, "sgn_mlp_pack_index", 3, n=(self.off_bb - self.base) // 2)
            self.ibb = imap(L.sgn_mlp_pack_index, "sgn_mlp_pack_index", 4, n=256)
        self.it = imap(L.sgn_train_pack_index, "sgn_train_pack_index", n=self.tbytes // 2)
        self.blob = torch.zeros(self.total, dtype=torch.uint8, device=device)
        self.tblob = torch.zeros(self.tbytes, dtype=torch.uint8, device=device)
        # (index map, destination bytes, fp16?) -- every section of both blobs in one gather launch
        segs = [(self.i16, self.blob[:self.off_f32], 1), (self.i32, self.blob[self.off_f32:self.off_f32 + 4 * N_F32], 0),
                (self.isp, self.blob[self.off_split:self.base], 1)]
        if variant != (0, 0):
            segs += [(self.iwb, self.blob[self.base:self.off_bb], 1), (self.ibb, self.blob[self.off_bb:], 0)]
        segs.append((self.it, self.tblob, 1))
        for idx, dst, h in segs:
            assert dst.numel() == idx.numel() * (2 if h else 4)
        self._segs = (_lib.GatherSegment * len(segs))(*[_lib.GatherSegment(idx.data_ptr(), dst.data_ptr(), idx.numel(), h, 0)
                                                       for idx, dst, h in segs])

    def pack(self, flat):
        flat = flat.detach()
        assert flat.is_contiguous() and flat.dtype == torch.float32
        _lib.check(_lib.lib().sgn_gather_segments(len(self._segs), self._segs, _lib.ptr(flat), flat.numel(),
                                                  _lib.stream_handle()), "sgn_gather_segments")
        return self.blob, self.tblob


def _colmap(which, n, device):
    a = (ctypes.c_int32 * n)()
    _lib.check(_lib.lib().sgn_train_colmap(which, a, n), "sgn_train_colmap")
    return torch.frombuffer(bytearray(a), dtype=torch.int32).long().to(device)
