"""The f16 training step's small segment kernels (csrc/optim.hip) through the C ABI: sgn_grad_accumulate,
sgn_gather_segments, sgn_zero_segments and sgn_pow2_scale against plain torch on the CPU (float64 sums,
torch's own fp16 rounding), sentinels around every destination."""
import ctypes

import pytest
import torch

import sgnerf_amd  # noqa: F401
from sgnerf_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


# (nb, n, stride, scalar path by a source view at element offset 1, tail given)
@pytest.mark.parametrize("scale", [None, 1024.0])
@pytest.mark.parametrize("layout", [((1, 1024, 1028, False, True), (16, 1023, 1024, False, False), (17, 512, 512, True, True)),
                                    ((600, 1024, 1024, False, False), (16, 1022, 1023, False, True), (1, 512, 516, True, False))])
def test_grad_accumulate(layout, scale):
    """grad[dst[j]] += (sum of nb partials (+ tail)) / scale over three segments in one launch: the float4 path
    (n, stride % 4 == 0, aligned) and the scalar one (n % 4 != 0, or a source at element offset 1), dst entries
    of -1 skipped, a starting gradient that is not zero.  Against a float64 sum within (nb + 2) u (sum |terms| /
    scale + |start|); a single partial group (nb <= 16) also bit for bit against the in-order fp32 sum."""
    g = torch.Generator().manual_seed(17)
    G = 4096
    grad0 = torch.randn(G + 8, generator=g)
    perm = torch.randperm(G, generator=g).to(torch.int32)
    segs = (_lib.GradSegment * len(layout))()
    keep, host, pos = [], [], 0
    for i, (nb, n, stride, off1, has_tail) in enumerate(layout):
        store = torch.randn(nb * stride + 8, generator=g)
        off = 1 if off1 else 0
        src = store[off:off + nb * stride].view(nb, stride)
        tail = torch.randn(n, generator=g) if has_tail else None
        dst = perm[pos:pos + n].clone()
        pos += n
        dst[torch.rand(n, generator=g) < 0.1] = -1
        sd, td, dd = store.to(DEV), (tail.to(DEV) if has_tail else None), dst.to(DEV)
        keep += [sd, td, dd]
        s = segs[i]
        s.src, s.tail, s.dst = sd.data_ptr() + 4 * off, (td.data_ptr() if has_tail else None), dd.data_ptr()
        s.n, s.stride, s.nb = n, stride, nb
        host.append((src[:, :n], tail, dst, nb))
    assert pos <= G
    grad = grad0.to(DEV)
    sc = torch.tensor([scale], device=DEV) if scale else None
    _lib.check(_lib.lib().sgn_grad_accumulate(len(layout), segs, _lib.ptr(sc), _lib.ptr(grad), _lib.stream_handle()),
               "sgn_grad_accumulate")
    torch.cuda.synchronize()
    got = grad.cpu()
    inv = 1.0 / scale if scale else 1.0
    ref = grad0.double().clone()
    bound = torch.zeros_like(ref)
    exact = grad0.clone()
    exact_mask = torch.zeros(G + 8, dtype=torch.bool)
    for src, tail, dst, nb in host:
        ok = dst >= 0
        d = dst[ok].long()
        tot = src.double().sum(0) + (tail.double() if tail is not None else 0)
        ab = src.double().abs().sum(0) + (tail.double().abs() if tail is not None else 0)
        ref[d] += tot[ok] * inv
        bound[d] = (nb + 2) * U * (ab[ok] * inv + grad0[d].double().abs())
        if nb <= 16:   # one partial group: the partials in order, then the tail, in fp32
            s32 = torch.zeros(src.shape[1])
            for b in range(nb):
                s32 = s32 + src[b]
            if tail is not None:
                s32 = s32 + tail
            exact[d] = grad0[d] + s32[ok] * torch.tensor(inv, dtype=torch.float32)
            exact_mask[d] = True
    touched = bound > 0
    assert torch.equal(_bits(got[~touched]), _bits(grad0[~touched]))   # skipped entries, other elements, the slack
    assert torch.equal(_bits(got[exact_mask]), _bits(exact[exact_mask]))
    worst = float(((got.double() - ref).abs()[touched] / bound[touched]).max())
    print(f"grad_accumulate nb={[x[0] for x in layout]} scale={scale}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_gather_segments():
    """dst[j] = src[idx[j]] as fp32 (bit-exact) or fp16 (torch's round to nearest even: ties, a value above
    65504, a subnormal), 0 for indices of -1 and >= n_src; two segments of different lengths in one launch,
    the elements after each destination untouched."""
    g = torch.Generator().manual_seed(18)
    n_src = 5000
    src = torch.randn(n_src, generator=g)
    plant = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2049.0, 2051.0, 65519.0, 65520.0, 70000.0, -1e5,
             1e-7, -3e-8, 2.0 ** -25, 6.1e-5, 0.0]
    src[:len(plant)] = torch.tensor(plant)
    n1, n2 = 3001, 777
    idx1 = torch.randint(0, n_src, (n1,), generator=g, dtype=torch.int32)
    idx2 = torch.randint(0, n_src, (n2,), generator=g, dtype=torch.int32)
    idx1[:len(plant)] = torch.arange(len(plant), dtype=torch.int32)
    idx2[:len(plant)] = torch.arange(len(plant), dtype=torch.int32)
    for idx in (idx1, idx2):
        idx[20], idx[21], idx[22], idx[23] = -1, n_src, n_src + 12345, -7
        idx[24] = n_src - 1
    d16 = torch.full((n1 + 5,), 7.0, dtype=torch.float16, device=DEV)
    d32 = torch.full((n2 + 5,), NAN, device=DEV)
    i1, i2, sd = idx1.to(DEV), idx2.to(DEV), src.to(DEV)
    segs = (_lib.GatherSegment * 2)()
    segs[0].idx, segs[0].dst, segs[0].n, segs[0].fp16 = i1.data_ptr(), d16.data_ptr(), n1, 1
    segs[1].idx, segs[1].dst, segs[1].n, segs[1].fp16 = i2.data_ptr(), d32.data_ptr(), n2, 0
    _lib.check(_lib.lib().sgn_gather_segments(2, segs, _lib.ptr(sd), n_src, _lib.stream_handle()), "sgn_gather_segments")
    torch.cuda.synchronize()

    def expect(idx):
        ok = (idx >= 0) & (idx < n_src)
        return torch.where(ok, src[idx.clamp(0, n_src - 1).long()], torch.zeros(()))
    e16 = expect(idx1).half()
    ep = e16[:len(plant)].float()
    assert bool(torch.isinf(ep).any()) and bool(((ep.abs() < 6.0e-5) & (ep != 0)).any())   # overflow and subnormals are in
    assert torch.equal(d16[:n1].cpu().view(torch.int16), e16.view(torch.int16))
    assert bool((d16[n1:] == 7.0).all())
    assert torch.equal(_bits(d32[:n2].cpu()), _bits(expect(idx2)))
    assert bool(torch.isnan(d32[n2:]).all())


def test_zero_segments():
    """Three regions at 16-B offsets inside one NaN-filled buffer cleared in one launch: a short one, an empty
    one, one longer than the launch's 1024 x 256 threads x 16 B (the stride loop); nothing else touched."""
    big = 1024 * 256 * 16 + 4000 * 16           # bytes
    n = (64 + 48 + 64 + big + 64) // 4 + 4
    buf = torch.full((n,), NAN, device=DEV)
    regions = [(16, 48), (160, 0), (176, big)]   # (byte offset, bytes)
    ptrs = (ctypes.c_void_p * 3)(*[buf.data_ptr() + o for o, _ in regions])
    nbytes = (ctypes.c_int64 * 3)(*[b for _, b in regions])
    _lib.check(_lib.lib().sgn_zero_segments(3, ptrs, nbytes, _lib.stream_handle()), "sgn_zero_segments")
    torch.cuda.synchronize()
    inside = torch.zeros(n, dtype=torch.bool)
    for o, b in regions:
        inside[o // 4:(o + b) // 4] = True
    got = buf.cpu()
    assert bool((got[inside] == 0).all()) and int(inside.sum()) == (48 + big) // 4
    assert bool(torch.isnan(got[~inside]).all()) and int((~inside).sum()) > 20


def _pow2(a, b):
    L = _lib.lib()
    ws = torch.empty(int(L.sgn_pow2_scale_workspace_bytes()), dtype=torch.uint8, device=DEV)
    out = torch.full((3,), -5.0, device=DEV)
    ad = a.to(DEV) if a is not None else None
    bd = b.to(DEV) if b is not None else None
    _lib.check(L.sgn_pow2_scale(_lib.ptr(ad), 0 if a is None else a.numel(), _lib.ptr(bd), 0 if b is None else b.numel(),
                                _lib.ptr(ws), _lib.ptr(out), _lib.stream_handle()), "sgn_pow2_scale")
    torch.cuda.synchronize()
    o = out.cpu()
    assert float(o[1]) == -5.0 and float(o[2]) == -5.0
    return float(o[0])


def test_pow2_scale():
    """2^-floor(log2(max(max|a|, max|b|, 1e-30))): exact powers of two give the exact reciprocal, any other max a
    power of two with 1 <= max x scale < 2, zeros the 1e-30 floor's 2^100, inf 0, a NaN in either array NaN;
    either array may be empty; the max may sit at the last element of a long array."""
    g = torch.Generator().manual_seed(19)
    for e in (-100, -30, -14, -1, 0, 1, 10, 60, 127):
        a = torch.randn(300, generator=g).clamp(-0.9, 0.9) * 2.0 ** e
        a[123] = -(2.0 ** e)
        assert _pow2(a, a[:7] * 0.5) == 2.0 ** -e, e
    for _ in range(6):
        a = torch.randn(1000, generator=g) * float(torch.rand((), generator=g) * 50 + 1e-3)
        b = torch.randn(333, generator=g) * float(torch.rand((), generator=g) * 50 + 1e-3)
        m = max(float(a.abs().max()), float(b.abs().max()))
        s = _pow2(a, b)
        assert s == 2.0 ** round(torch.log2(torch.tensor(s)).item()) and 1.0 <= m * s < 2.0, (m, s)
    # one ulp below a power of two: floor(log2) is k - 1 (scale 2^-(k-1), max x scale just below 2) unless the
    # device's log2f rounds the argument's logarithm up to k (scale 2^-k, just below 1): either is accepted
    for k in (-3, 0, 5):
        m = float(torch.nextafter(torch.tensor(2.0 ** k), torch.tensor(0.0)))
        s = _pow2(torch.tensor([0.1 * m, -m, 0.0]), None)
        assert s in (2.0 ** -(k - 1), 2.0 ** -k), (k, s)
        print(f"pow2_scale one ulp below 2^{k}: scale 2^{round(torch.log2(torch.tensor(s)).item())} "
              f"({'floor is k - 1' if s == 2.0 ** -(k - 1) else 'log2f rounded up to k'})")
    assert _pow2(torch.zeros(100), torch.zeros(3)) == 2.0 ** 100
    assert _pow2(torch.tensor([1.0, float("inf"), 2.0]), torch.ones(4)) == 0.0
    assert _pow2(torch.tensor([1.0, -float("inf")]), None) == 0.0
    s = _pow2(torch.tensor([1.0, NAN, 3.0]), torch.ones(4))
    assert s != s
    s = _pow2(torch.ones(4), torch.tensor([float("inf"), NAN]))
    assert s != s
    assert _pow2(None, torch.tensor([3.0])) == 0.5 and _pow2(torch.tensor([-5.0]), None) == 0.25
    a = torch.rand(1_000_003, generator=g)
    a[-1] = -77.0
    assert _pow2(a, None) == 2.0 ** -6
    assert _pow2(torch.rand(5, generator=g), a) == 2.0 ** -6
