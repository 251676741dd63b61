"""Hand-built scenes for the grid build, the ray march and the layered kNN, with an exact reference.

Two families of scenes:

* Dyadic scenes.  The voxel size is a power of two and the origin, every point, the camera, every
  direction and every depth are dyadic rationals chosen so that each `campos + dir * t`, each
  `(p - shift) / vs` and each squared distance is exactly representable in fp32.  fp32 arithmetic on
  them has no rounding, so the whole query can be restated in Python integers (`exact_grid`,
  `exact_query`), and a kernel, the C restatement (oracle/query_ref.c) and this file must agree bit
  for bit.  The builder asserts the exactness of every quantity (mantissa span <= 24 bits) while the
  reference runs: a scene that leaves the exact domain fails, it is not rounded.

* Rounding scenes (`rounding_scene`).  The same lattice with the voxel size `grid_hyperparameters`
  gives (0.016, not a power of two), the box at the far end of `opt.ranges`, candidate depths one and
  two `nextafter` steps on either side of every face crossing and of the widened box's entry and exit,
  and directions with a 1e-30 and a subnormal component.  Exact arithmetic cannot state these: HERE
  THE ORACLE'S FULL-TABLE SCAN (oracle/query_ref.c, which has no span culling) IS THE REFERENCE.

The exact reference is written from the reference model's kernels
(models/neural_points/query_point_indices_worldcoords.py), not from query_ref.c or the HIP code:

  claim_occ :265-326          claims in point order; beyond max_o the reservoir :312-321
  map_coor2occ :328-363       coor_2_occ of the kept slots, coor_occ on [c - q/2, c + (q+1)/2)
  fill_occ2pnts :365-410      lists in point order, `voxel_idx > 0` (:395) unless fix_occ0,
                              reservoir beyond P :400-407 (the counter keeps counting)
  mask_raypos :413-437, cumsum slot rule :843-844, get_shadingloc :439-461
  query_neigh_along_ray_layered :594-681, semantic filter :548-553 (label_prob reads as 0)

The reservoir draw is `sgnref_uniform`, the one primitive shared by all three implementations
(u = (b + 1) / 2^24); `ceilf(u * (tmp + 1)) - 1` is restated on integers with the product rounded to
24 significant bits, nearest-even, as the fp32 multiply rounds it.

`plantings(scene)` reports, from the exact reference's own run, which edge cases a scene holds and for
which ray, sample or voxel: the CPU test asserts every planting by name.
"""
import bisect
import types
from fractions import Fraction

import numpy as np

import oracle_query as oq
from sgnerf_amd.opts import HotPathOpts

E = 48                      # every dyadic input is an integer multiple of 2^-E
Q = 1 << E
VS = 0.125                  # dyadic voxel size 2^-3
LQ = VS / 4                 # lattice quantum 2^-5: points sit on multiples of it
SHIFT = (-0.5, 0.25, 1.0)   # dyadic grid origin
H10 = 2.0 ** -10


# ---- exact arithmetic helpers -------------------------------------------------------------------
def _I(x):
    """A dyadic float as an integer multiple of 2^-E (asserted exact)."""
    f = Fraction(float(x)) * Q
    assert f.denominator == 1, f"{x!r} is not a multiple of 2^-{E}"
    return int(f)


def _span(n):
    """Mantissa span of an integer: bits from its highest to its lowest set bit."""
    if n == 0:
        return 0
    n = abs(n)
    return n.bit_length() - ((n & -n).bit_length() - 1)


def _fits(n, what):
    assert _span(n) <= 24, f"{what}: mantissa span {_span(n)} bits does not fit fp32"
    return n


def _rne24(n):
    """A positive integer rounded to 24 significant bits, ties to even (one fp32 rounding)."""
    b = n.bit_length()
    if b <= 24:
        return n
    s = b - 24
    q, r = n >> s, n & ((1 << s) - 1)
    half = 1 << (s - 1)
    if r > half or (r == half and (q & 1)):
        q += 1
    return q << s


def _reservoir_slot(seed, stream, i, tmp):
    """insrtidx = ceilf(curand_uniform * (tmp + 1)) - 1 (:315, :403), the draw from sgnref_uniform."""
    u = float(oq.lib().sgnref_uniform(int(seed), int(stream), int(i)))
    num = int(Fraction(u) * (1 << 24))          # u = num / 2^24, num in [1, 2^24]
    prod = _rne24(num * (tmp + 1))               # fp32 product, numerator over 2^24
    return -((-prod) >> 24) - 1                  # ceil - 1


# ---- scenes ----------------------------------------------------------------------------------------
def make_hyper(dims, r2=0.0, shift=SHIFT, vs=VS):
    d = np.array(dims, np.int32)
    return types.SimpleNamespace(shift=np.array(shift, np.float32), scaled_vsize=np.full(3, vs, np.float32),
                                 scaled_vdim=d, r2=np.float32(r2), volume=int(np.prod(d.astype(np.int64))))


def make_opts(**kw):
    base = dict(max_o=4096, P=4, K=4, SR=3, reservoir_seed=11, fix_occ0=0, kernel_size=(3, 3, 3),
                query_size=(3, 3, 3))
    base.update(kw)
    return HotPathOpts(**base)


def lattice_xyz(idx, shift=SHIFT):
    """Lattice indices [N, 3] (integers, multiples of LQ from the origin) as float32 positions."""
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    return (np.array(shift, np.float64)[None] + idx * LQ).astype(np.float32)


class Scene(types.SimpleNamespace):
    """name, xyz [N,3] f32, hyper, opts, campos [3], raydir [R,3], t ([D] or [R,D]), per_ray_t,
    point_labels / ray_labels (or None), seconds, expect (planting names this scene must hold),
    exact (True: dyadic, the exact reference applies)."""

    @property
    def R(self):
        return self.raydir.shape[0]

    @property
    def D(self):
        return self.t.shape[-1]


def _scene(name, idx, dims, opts, campos, raydir, t, expect=(), labels=None, seconds=0, r2=0.0):
    t = np.ascontiguousarray(t, np.float32)
    pl = rl = None
    if labels is not None:
        pl, rl = (np.ascontiguousarray(x, np.int32) for x in labels)
    return Scene(name=name, xyz=lattice_xyz(idx), hyper=make_hyper(dims, r2), opts=opts,
                 campos=np.array(campos, np.float32), raydir=np.ascontiguousarray(raydir, np.float32).reshape(-1, 3),
                 t=t, per_ray_t=int(t.ndim == 2), point_labels=pl, ray_labels=rl, seconds=int(seconds),
                 expect=tuple(expect), exact=True)


def _box_centre(dims):
    return [SHIFT[a] + (dims[a] * 4 // 2) * LQ + LQ / 2 for a in range(3)]


def fan_rays(R, D, seed, dims):
    """A camera inside the box, R dyadic directions (components multiples of 1/4, both zeros, one
    all-zero direction, one ray pointing out through each face), shared t_d = (d + 1) 2^-4."""
    rng = np.random.default_rng(seed)
    dirs = rng.integers(-4, 5, (R, 3)).astype(np.float32) / 4
    neg = rng.random((R, 3)) < 0.5
    dirs = np.where((dirs == 0) & neg, np.float32(-0.0), dirs)
    if R >= 4:
        dirs[1] = (0.0, -0.0, 0.0)
        dirs[2] = (1.0, -0.0, 0.0)
        dirs[3] = (-0.0, 0.0, -0.25)
    t = (np.arange(D) + 1) * 2.0 ** -4
    return _box_centre(dims), dirs, t


def _grid_cloud(dims, P, seed, big=True, filler=60):
    """The grid group's cloud: point 0 alone in its voxel (slot 0), voxels holding P - 1, P, P + 1 (and
    3 P) points, points on lower faces, on the outer upper faces, at shift exactly, just outside,
    duplicates, random filler; every point but the first in a seeded random order."""
    rng = np.random.default_rng(seed)
    dims = np.array(dims)
    pts = []

    def in_voxel(v, n):
        offs = rng.permutation(64)[:n] if n <= 64 else rng.integers(0, 64, n)
        for o in offs:
            pts.append([v[0] * 4 + o // 16, v[1] * 4 + (o // 4) % 4, v[2] * 4 + o % 4])

    groups = {}
    if np.all(dims >= (8, 6, 4)):
        groups = {"P-1": ((1, 1, 1), P - 1), "P": ((2, 5, 3), P), "P+1": ((6, 2, 1), P + 1)}
        if big:
            groups["3P"] = ((7, 5, 3), 3 * P)
        for v, n in groups.values():
            in_voxel(v, n)
    pts.append([0, 0, 0])                                           # at shift exactly -> voxel (0, 0, 0)
    pts.append([min(3, dims[0] - 1) * 4, min(3, dims[1] - 1) * 4, 0])   # on three lower faces (inside)
    for a in range(3):
        up = [1, 1, 1]
        up[a] = dims[a] * 4                                         # on the outer upper face (outside)
        pts.append(up)
        lo = [1, 1, 1]
        lo[a] = -1                                                  # just outside
        pts.append(lo)
    n_group = len(pts)
    for _ in range(filler):
        pts.append([int(rng.integers(0, dims[a] * 4)) for a in range(3)])
    for _ in range(6):
        pts.append([int(rng.integers(-8, dims[a] * 4 + 8)) for a in range(3)])
    gv = {v for v, _ in groups.values()}                            # the counted voxels hold their groups only
    pts = pts[:n_group] + [p for p in pts[n_group:] if tuple(np.floor_divide(p, 4)) not in gv]
    for j in rng.integers(n_group, len(pts), 20):                    # duplicates
        pts.append(list(pts[j]))
    pts = [pts[j] for j in rng.permutation(len(pts))]
    alone = tuple(int(d) // 2 for d in dims)                        # kept free for point 0
    pts = [p for p in pts if tuple(np.floor_divide(p, 4)) != alone]
    pts.insert(0,[alone[0] * 4 + 1, alone[1] * 4 + 2, alone[2] * 4 + 3])
    return np.array(pts, np.int64), {k: v[0] for k, v in groups.items()}


def n_claimed_of(idx, dims):
    v = np.floor_divide(np.asarray(idx).reshape(-1, 3), 4)
    ok = np.all((v >= 0) & (v < np.array(dims)), axis=1)
    return len({tuple(x) for x in v[ok]})


def grid_scene(name, dims=(9, 7, 5), P=4, K=4, SR=3, R=5, D=9, max_o=None, big=True, seed=1, expect=(), **okw):
    idx, groups = _grid_cloud(dims, P, seed, big)
    nc = n_claimed_of(idx, dims)
    mo = {None: 4096, "n-1": nc - 1, "n": nc, "n+1": nc + 1}.get(max_o, max_o)
    campos, dirs, t = fan_rays(R, D, seed + 100, dims)
    sc = _scene(name, idx, dims, make_opts(P=P, K=K, SR=SR, max_o=mo, **okw), campos, dirs, t, expect)
    sc.groups = groups
    return sc


def slots_scene(n, dims=(9, 7, 5), seed=3):
    """Exactly n claimed voxels (n_slots = n): one point in each of n voxels, some duplicated."""
    rng = np.random.default_rng(seed)
    vol = int(np.prod(dims))
    vox = rng.permutation(vol)[:n]
    v3 = np.stack([vox // (dims[1] * dims[2]), (vox // dims[2]) % dims[1], vox % dims[2]], -1)
    idx = v3 * 4 + rng.integers(0, 4, (n, 3))
    idx = np.concatenate([idx, idx[rng.integers(0, n, 12)]])
    campos, dirs, t = fan_rays(5, 9, seed, dims)
    return _scene(f"slots_{n}", idx, dims, make_opts(), campos, dirs, t, expect=(f"n_slots_{n}",))


def empty_scene(kind):
    dims = (9, 7, 5)
    if kind == "n0":
        idx, ex = np.zeros((0, 3), np.int64), ("n_points_0",)
    elif kind == "n1":
        idx, ex = np.array([[17, 9, 6]]), ("n_points_1", "point0_alone_in_slot0")
    else:
        idx = np.array([[-1, 3, 3], [36, 3, 3], [3, 28, 3], [3, 3, 20], [-5, -5, -5], [40, 30, 25]])
        ex = ("all_points_outside",)
    campos, dirs, t = fan_rays(5, 9, 5, dims)
    return _scene(f"empty_{kind}", idx, dims, make_opts(), campos, dirs, t, expect=ex)


# ---- march scenes: one flagged row of voxels, rays along it ------------------------------------
ROW = (3, 2)   # the row y = 3, z = 2 of a (9, 7, 5) grid


def _row_cloud(query1=False):
    """query_size 3: three occupied voxels flag the whole row x = 0..8 (and its neighbours);
    query_size 1 (`query1`): every voxel of the row occupied and nothing else flagged.  Point 0 sits at
    `shift` exactly, alone in slot 0."""
    pts = [[0, 0, 0]]
    xs = range(9) if query1 else (1, 4, 7)
    for x in xs:
        for o in ((1, 1, 1), (2, 3, 0), (0, 2, 3)):
            pts.append([x * 4 + o[0], ROW[0] * 4 + o[1], ROW[1] * 4 + o[2]])
    return np.array(pts, np.int64)


def _row_campos():
    return [SHIFT[0] - 4 * VS, SHIFT[1] + (ROW[0] + 0.5) * VS, SHIFT[2] + (ROW[1] + 0.5) * VS]


def _row_table(a, g, m, D):
    """A strictly increasing dyadic depth table for a +x ray from _row_campos(): `a` candidates before
    the widened box (t < 2 vs), `g` in the entry margin (the first at t_in exactly), `m` inside the box
    (the first on its entry face), the rest from the exit face on (one at t_out exactly)."""
    assert a <= 511 and g <= 256 and m <= 1152 and a + g + m <= D
    t = [(i + 1) * H10 / 2 for i in range(a)]
    t += [0.25 + i * H10 for i in range(g)]
    t += [0.5 + i * H10 for i in range(m)]
    rest = D - len(t)
    t += [1.625 + i * H10 * 64 for i in range(rest)]   # 1.625 exit face, 1.875 = t_out at i = 4
    return t


def march_sr_scene(SR, D=None):
    """Per-ray depth tables: rays with exactly SR - 1, SR, SR + 1 and >> SR flagged candidates, the
    SR-th flagged one at offset 63 / 0 of a 64-group and 7 / 0 of an 8-chunk from the ray's d_lo, a
    table wholly before and wholly after the box, a ray pointing away, spans with d_lo > 0 and
    d_hi < D - 1, both zeros in the idle components."""
    D = D or (400 if SR >= 128 else 129)
    rows, dirs = [], []
    z = (0.0, -0.0)

    def ray(a, g, m, sx=1.0, k=0):
        rows.append(_row_table(a, g, m, D))
        dirs.append((sx, z[k & 1], z[(k >> 1) & 1]))

    for k, m in enumerate((max(SR - 1, 0), SR, SR + 1)):
        ray(3, 5, m, k=k)
    ray(3, 5, D - 8, k=3)                                  # >> SR (as many as the table holds)
    ray(2, (63 - (SR - 1)) % 64, SR + 2, k=1)              # SR-th at offset 63 (and 7)
    ray(2, (64 - (SR - 1)) % 64, SR + 2, k=2)              # SR-th at offset 0 of a 64-group (and 0 of 8)
    ray(0, (7 - (SR - 1)) % 8, SR + 2, k=3)                # SR-th at offset 7 of an 8-chunk
    ray(1, (8 - (SR - 1)) % 8, SR + 2, k=0)                # SR-th at offset 0 of an 8-chunk
    ray(0, 0, SR + 1, k=1)                                 # d_lo = 0
    ray(0, 7, 0, k=2)                                      # only margin candidates
    rows.append([(i + 1) * H10 / 4 for i in range(D)])     # whole table before the box
    dirs.append((1.0, 0.0, -0.0))
    rows.append([2.0 + i * H10 for i in range(D)])         # whole table after the box
    dirs.append((1.0, -0.0, 0.0))
    ray(3, 5, SR + 1, sx=-1.0)                             # pointing away
    ex = ["flagged_SR-1", "flagged_SR", "flagged_SR+1", "flagged_>>SR", "srth_at_64group_offset_63",
          "srth_at_64group_offset_0", "srth_at_8chunk_offset_7", "srth_at_8chunk_offset_0", "span_d_lo_gt_0",
          "span_d_hi_lt_D-1", "table_before_box", "table_after_box", "ray_pointing_away", "dir_plus_zero",
          "dir_minus_zero", "per_ray_t"]
    return _scene(f"march_sr{SR}", _row_cloud(), (9, 7, 5), make_opts(SR=SR, K=4), _row_campos(), dirs,
                  np.array(rows), expect=ex)


def march_shared_scene():
    """Shared depth table; the direction's length places the table before, across and after the box."""
    dirs = [(s, z0, z1) for s, z0, z1 in ((2.0 ** -6, 0.0, -0.0), (0.125, -0.0, 0.0), (0.25, 0.0, 0.0),
                                          (0.5, -0.0, -0.0), (1.0, 0.0, 0.0), (2.0, 0.0, -0.0),
                                          (64.0, -0.0, 0.0), (128.0, 0.0, 0.0), (-1.0, 0.0, 0.0))]
    t = (np.arange(129) + 1) * 2.0 ** -6
    return _scene("march_shared", _row_cloud(), (9, 7, 5), make_opts(SR=8), _row_campos(), dirs, t,
                  expect=("shared_t", "table_before_box", "table_after_box", "ray_pointing_away",
                          "span_d_lo_gt_0", "span_d_hi_lt_D-1"))


def march_d_scene(D, R):
    sc = grid_scene(f"march_D{D}_R{R}", R=R, D=D, seed=7, expect=(f"D_{D}", f"R_{R}", "shared_t"))
    return sc


def march_deep_scene():
    """D = 32767, t_d = d 2^-12: the top of the int16 slot table.  Ray 0 reaches the box at its last
    candidate d = 32766; ray 1 never does; ray 2 enters at d = 16383 and carries >> SR flagged ones."""
    D = 32767
    campos = _row_campos()
    campos[0] = SHIFT[0] - 32766 * 2.0 ** -12
    dirs = [(1.0, 0.0, -0.0), (0.5, -0.0, 0.0), (2.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (4.0, -0.0, -0.0)]
    t = np.arange(D) * 2.0 ** -12
    return _scene("march_deep", _row_cloud(), (9, 7, 5), make_opts(SR=8), campos, dirs, t,
                  expect=("D_32767", "flagged_at_d_32766", "flagged_>>SR", "span_d_lo_gt_0"))


def camera_scene(case):
    """A zero direction component (both signs) on the y axis, the camera's y inside the box, in the
    two-voxel margin, exactly on either edge of the widened box, and outside it."""
    y = {"inside": SHIFT[1] + (ROW[0] + 0.5) * VS, "margin": SHIFT[1] - VS, "lo_edge": SHIFT[1] - 2 * VS,
         "hi_edge": SHIFT[1] + (7 + 2) * VS, "outside_lo": SHIFT[1] - 3 * VS,
         "outside_hi": SHIFT[1] + (7 + 3) * VS}[case]
    campos = _row_campos()
    campos[1] = y
    up = 1.0 if y < SHIFT[1] + 3 * VS else -1.0
    dirs = [(1.0, 0.0, 0.0), (1.0, -0.0, 0.0), (1.0, 0.0, -0.0), (1.0, up * 0.5, 0.0), (1.0, up * 1.0, -0.0),
            (0.5, up * 0.75, 0.0), (0.0, up * 1.0, 0.0), (-0.0, up * 1.0, 0.0)]
    t = (np.arange(65) + 1) * 2.0 ** -5
    return _scene(f"camera_{case}", _row_cloud(), (9, 7, 5), make_opts(SR=8), campos, dirs, t,
                  expect=(f"zero_dir_camera_{case}", "dir_plus_zero", "dir_minus_zero"))


def face_scene():
    """query_size 1: the row's voxels are the only flagged ones.  The camera's y lies exactly on the
    face between the unflagged row y = 2 and the flagged row y = 3; the rays run along that face."""
    campos = _row_campos()
    campos[1] = SHIFT[1] + ROW[0] * VS
    dirs = [(1.0, 0.0, 0.0), (1.0, -0.0, -0.0), (0.5, 0.0, 0.0), (1.0, -2.0 ** -8, 0.0), (1.0, 2.0 ** -8, 0.0)]
    t = (np.arange(64) + 1) * 2.0 ** -5
    return _scene("face", _row_cloud(query1=True), (9, 7, 5), make_opts(SR=64, query_size=(1, 1, 1)), campos, dirs,
                  t, expect=("ray_along_face_flagged_unflagged",))


def corner_scene():
    """A ray that clips the corner voxel (0, 0, 0) only (flagged by the point at `shift` exactly)."""
    campos = [SHIFT[0] - VS / 4, SHIFT[1] + 3 * VS / 4, SHIFT[2] + VS / 2]
    dirs = [(1.0, -1.0, 0.0), (1.0, -1.0, -0.0), (0.5, -0.5, 0.0)]
    t = (np.arange(16) + 1) * 2.0 ** -6
    idx = np.array([[0, 0, 0], [1, 2, 3], [30, 20, 10]])
    return _scene("corner", idx, (9, 7, 5), make_opts(SR=8, query_size=(1, 1, 1), fix_occ0=1), campos, dirs, t,
                  expect=("ray_through_one_corner_voxel",))


# ---- kNN scenes: one planting per isolated region of a (16, 10, 7) grid ----------------------------
KDIMS = (16, 10, 7)
R2_L = 25   # radius^2 in lattice units: 25 = 5^2 = 4^2 + 3^2 is attained, 26 = 5^2 + 1 is the next step


def _own(pool_lo, pool_hi, n, rng):
    """n distinct in-voxel lattice offsets (0..3)^3 whose squared distance from the voxel centre
    offset (2, 2, 2) lies in [pool_lo, pool_hi]."""
    c = [(a, b, d) for a in range(4) for b in range(4) for d in range(4)
         if pool_lo <= (a - 2) ** 2 + (b - 2) ** 2 + (d - 2) ** 2 <= pool_hi]
    assert len(c) >= n
    return [c[j] for j in rng.permutation(len(c))[:n]]


def knn_scene(K, r2=True, semantic=None, seed=5, P=None, name=None):
    """Samples at voxel centres (ray r: dir = centre - campos, shared t = [1, 64]); see the region
    comments.  `semantic`: seconds, with seeded labels in {0, 1, 2}."""
    rng = np.random.default_rng(seed)
    P = P or K + 4
    pts, centres, regions = [], [], {}

    def put(V, off, o):
        pts.append([(V[a] + off[a]) * 4 + o[a] for a in range(3)])

    def region(nm, V):
        regions[nm] = len(centres)
        centres.append(V)
        return V

    # slot 0: point 0 alone in its voxel; its list is empty under the `> 0` rule
    V = region("slot0", (12, 6, 3))
    put(V, (0, 0, 0), (2, 2, 2))
    # incoming point ties the farthest (d2 = 4): not replaced
    V = region("tie_far", (6, 3, 3))
    for o in _own(0, 3, K - 1, rng) + [(0, 2, 2), (2, 0, 2)]:
        put(V, (0, 0, 0), o)
    # two farthest at d2 = 4, then three points at d2 = 3: two replace them, the third ties
    V = region("tie_among", (9, 3, 3))
    body = _own(0, 2, max(K - 2, 0), rng)
    for o in ([(0, 2, 2)] if K == 1 else [(0, 2, 2)] + body[: (K - 2) // 2] + [(2, 2, 0)] + body[(K - 2) // 2:]):
        put(V, (0, 0, 0), o)
    for o in ((1, 1, 1), (3, 3, 3), (1, 3, 1)):
        put(V, (0, 0, 0), o)
    # d2 = 0 on the first push
    V = region("d2zero_first", (12, 3, 3))
    for o in [(2, 2, 2)] + _own(1, 12, K, rng):
        put(V, (0, 0, 0), o)
    # K points at d2 = 0, then candidates at 0 and 1
    V = region("full_at_zero", (3, 6, 3))
    for o in [(2, 2, 2)] * (K + 1) + [(3, 2, 2)]:
        put(V, (0, 0, 0), o)
    # d2 == r2 kept (5, 0, 0) and (4, 3, 0); the next step (5, 1, 0) dropped
    V = region("r2_edge", (6, 6, 3))
    for o in ((3, 2, 2), (3, 3, 2)):
        put(V, (1, 0, 0), o)
    put(V, (1, 1, 0), (2, 1, 2))
    # flagged, nothing in range: nnb = 0, absent from the work list
    V = region("nnb_zero", (9, 6, 3))
    put(V, (1, 1, 0), (3, 3, 3))
    # exactly K in layer 0 (all at d2 >= 5) while a nearer point (d2 = 4) sits in layer 1
    V = region("k_in_layer0", (3, 3, 0))
    for o in _own(5, 12, K, rng):
        put(V, (0, 0, 0), o)
    put(V, (1, 0, 0), (0, 2, 2))
    # K - 1 in layer 0, layer 1 overfills with nearer points
    V = region("km1_overfill", (6, 3, 0))
    for o in _own(6, 12, K - 1, rng):
        put(V, (0, 0, 0), o)
    for off, o in (((0, 0, 1), (2, 2, 0)), ((0, 1, 0), (2, 0, 2)), ((1, 0, 0), (0, 2, 2)), ((1, 0, 0), (0, 1, 2))):
        put(V, off, o)
    # layer-1 total of exactly 1
    V = region("total1", (9, 3, 0))
    put(V, (0, 1, 0), (2, 0, 2))
    # runs 1, 1 (an empty voxel between), then 1, 0, 2, 3 at the end of the visit order; layer 0 short of K
    V = region("runs", (3, 3, 3))
    for o in _own(0, 12, max(K - 2, 0), rng):
        put(V, (0, 0, 0), o)
    put(V, (0, 0, 1), (2, 2, 0))
    put(V, (0, 1, 0), (2, 0, 2))
    put(V, (1, 0, 1), (0, 2, 0))
    for o in ((0, 0, 2), (1, 0, 2)):
        put(V, (1, 1, 0), o)
    for o in ((0, 0, 0), (1, 0, 0), (0, 1, 0)):
        put(V, (1, 1, 1), o)
    # corner voxels: clamped neighbourhoods, fewer than K found when K > 3
    V = region("corner000", (0, 0, 0))
    for off, o in (((0, 0, 0), (1, 2, 3)), ((1, 0, 0), (0, 2, 2)), ((0, 1, 1), (2, 0, 0))):
        put(V, off, o)
    V = region("cornermax", tuple(d - 1 for d in KDIMS))
    for off, o in (((0, 0, 0), (3, 3, 3)), ((-1, 0, 0), (3, 2, 2)), ((0, -1, -1), (2, 3, 3))):
        put(V, off, o)

    campos = np.array([SHIFT[0] - 1.0, SHIFT[1] - 0.5, SHIFT[2] - 0.25])
    ctr = np.array([[SHIFT[a] + (V[a] * 4 + 2) * LQ for a in range(3)] for V in centres])
    dirs = ctr - campos[None]
    ex = ["point0_alone_in_slot0", "sample_in_voxel_000", "sample_in_voxel_dims-1", "tie_incoming_equals_farthest",
          "d2_zero_first_push", "full_at_d2_zero_then_candidate", "nnb_partial_minus1_tail", "nnb_zero_not_in_worklist",
          "exactly_K_in_layer0_nearer_in_layer1", "layer1_total_1", "runs_0_1_2_3_adjacent", "runs_of_length_1_adjacent",
          f"K_{K}"]
    if K > 1:
        ex += ["tie_among_farthest_after_replacement", "K-1_in_layer0_layer1_overfills"]
    ex += ["d2_equals_r2_kept", "r2_next_step_dropped"] if r2 else ["r2_zero"]
    labels = None
    if semantic is not None:
        labels = (rng.integers(0, 3, len(pts)), rng.integers(0, 3, len(centres)))
        ex = [f"K_{K}", "label_zero", "label_equal", "label_different", f"seconds_mod10_{semantic % 10}"] + \
            (["label_rejected"] if semantic % 10 > 1 else [])
    nm = name or f"knn_K{K}" + ("" if r2 else "_r0") + ("" if semantic is None else f"_sem{semantic % 10}")
    sc = _scene(nm, np.array(pts), KDIMS, make_opts(K=K, P=P, SR=2), campos, dirs, np.array([1.0, 64.0]), expect=ex,
                labels=labels, seconds=semantic or 0, r2=R2_L * LQ * LQ if r2 else 0.0)
    sc.regions = regions
    return sc


def knn5_scene(K=4):
    """kernel_size 5 (three layers), query_size 5, r2 = 0: a break after layer 0, after layer 1, all
    three layers, and a sample two voxels from the nearest point."""
    rng = np.random.default_rng(9)
    pts, centres = [[50, 30, 2]], []

    def put(V, off, o):
        pts.append([(V[a] + off[a]) * 4 + o[a] for a in range(3)])

    V = (2, 2, 3); centres.append(V)          # K in layer 0
    for o in _own(0, 12, K, rng):
        put(V, (0, 0, 0), o)
    put(V, (1, 0, 0), (0, 2, 2))
    V = (7, 2, 3); centres.append(V)          # nothing in layer 0, K + 1 in layer 1, nearer ones in layer 2 unseen
    for j in range(K + 1):
        put(V, (1, 0, 0) if j % 2 else (0, -1, 1), (j % 4, 2, 1))
    put(V, (2, 0, 0), (0, 2, 2))
    V = (12, 2, 3); centres.append(V)         # 1 in layer 0, 1 in layer 1, layer 2 overfills
    put(V, (0, 0, 0), (1, 1, 1))
    put(V, (-1, 1, 0), (3, 0, 2))
    for j in range(K + 2):
        put(V, (2, -2, 1) if j % 2 else (-2, 0, 2), (j % 4, (j // 2) % 4, 2))
    V = (2, 7, 3); centres.append(V)          # two voxels from the only point around
    put(V, (2, 2, -2), (0, 0, 3))
    campos = np.array([SHIFT[0] - 1.0, SHIFT[1] - 0.5, SHIFT[2] - 0.25])
    ctr = np.array([[SHIFT[a] + (V[a] * 4 + 2) * LQ for a in range(3)] for V in centres])
    return _scene("knn_kernel5", np.array(pts), KDIMS,
                  make_opts(K=K, P=K + 4, SR=2, kernel_size=(5, 5, 5), query_size=(5, 5, 5)), campos,
                  ctr - campos[None], np.array([1.0, 64.0]),
                  expect=("kernel5_break_after_layer0", "kernel5_break_after_layer1", "kernel5_all_three_layers", "r2_zero"))


def dyadic_scenes():
    """name -> builder of every dyadic scene (built on demand; each build is deterministic)."""
    s = {}

    def add(fn, *a, **k):
        sc = fn(*a, **k)
        assert sc.name not in s, sc.name
        s[sc.name] = sc

    G = ("dims_9_7_5", "point_on_lower_faces_inside", "point_on_outer_upper_face_outside", "point_at_shift",
         "point_just_outside", "duplicate_points", "point0_alone_in_slot0")
    V4 = ("voxel_with_P-1", "voxel_with_P", "voxel_with_P+1")
    add(grid_scene, "grid_main", expect=G + V4 + ("voxel_with_3P",))
    add(grid_scene, "grid_fix0", fix_occ0=1, expect=G + V4)
    add(grid_scene, "grid_q212", query_size=(2, 4, 1), expect=("query_size_even_anisotropic",))
    add(grid_scene, "grid_q5", query_size=(5, 5, 5), kernel_size=(5, 5, 5), expect=())
    add(grid_scene, "grid_q1", query_size=(1, 1, 1), expect=())
    add(grid_scene, "grid_P63", P=63, big=False, K=8, expect=V4 + ("P_63_full_voxel",))
    add(grid_scene, "grid_P64", P=64, big=False, K=8, expect=V4 + ("P_64",))
    add(grid_scene, "grid_maxo_n-1", max_o="n-1", expect=("n_claimed_max_o+1",))
    add(grid_scene, "grid_maxo_n", max_o="n", expect=("n_claimed_max_o",))
    add(grid_scene, "grid_maxo_n+1", max_o="n+1", expect=("n_claimed_max_o-1",))
    add(grid_scene, "grid_maxo_1", max_o=1, fix_occ0=1, expect=("max_o_1",))
    add(grid_scene, "grid_maxo_40", max_o=40, fix_occ0=1, seed=2, expect=())
    add(grid_scene, "grid_degenerate", dims=(1, 6, 2), expect=("dims_1_6_2", "sample_in_degenerate_grid"))
    for n in (255, 256, 257):
        add(slots_scene, n)
    for kind in ("n0", "n1", "outside"):
        add(empty_scene, kind)
    for SR in (1, 3, 8, 9, 64, 128):
        add(march_sr_scene, SR)
    add(march_shared_scene)
    for D, R in ((1, 1), (7, 3), (8, 4), (9, 5), (63, 255), (64, 256), (65, 257), (129, 5)):
        add(march_d_scene, D, R)
    add(march_deep_scene)
    for case in ("inside", "margin", "lo_edge", "hi_edge", "outside_lo", "outside_hi"):
        add(camera_scene, case)
    add(face_scene)
    add(corner_scene)
    for K in (1, 4, 8, 16):
        add(knn_scene, K)
    add(knn_scene, 8, r2=False)
    add(knn_scene, 8, P=63, name="knn_K8_P63")
    add(knn_scene, 8, P=64, name="knn_K8_P64")
    for sec in (10, 11, 12):
        add(knn_scene, 4, semantic=sec)
    add(knn_scene, 4, semantic=12, P=64, name="knn_K4_sem2_P64")    # k_knn<K, SEMANTIC> without the counters
    add(knn5_scene)
    return s


_SCENES, _EXACT = None, {}


def scene_exact(name):
    """(scene, exact grid, exact query, plantings) of the dyadic scene `name`, computed once per process and
    shared by every test that needs it; nothing in it is written afterwards."""
    global _SCENES
    if _SCENES is None:
        _SCENES = dyadic_scenes()
    if name not in _EXACT:
        sc = _SCENES[name]
        g = exact_grid(sc)
        q = exact_query(sc, g)
        _EXACT[name] = (sc, g, q, plantings(sc, g, q))
    return _EXACT[name]


def scene_names():
    global _SCENES
    if _SCENES is None:
        _SCENES = dyadic_scenes()
    return list(_SCENES)


def scene(name):
    scene_names()
    return _SCENES[name]


ALL_PLANTINGS = (
    # grid
    "dims_9_7_5", "dims_1_6_2", "point_on_lower_faces_inside", "point_on_outer_upper_face_outside", "point_at_shift",
    "point_just_outside", "duplicate_points", "voxel_with_P-1", "voxel_with_P", "voxel_with_P+1", "voxel_with_3P",
    "P_63_full_voxel", "P_64", "n_claimed_max_o-1", "n_claimed_max_o", "n_claimed_max_o+1", "max_o_1", "n_slots_255",
    "n_slots_256", "n_slots_257", "point0_alone_in_slot0", "n_points_0", "n_points_1", "all_points_outside",
    "query_size_even_anisotropic",
    # march
    "D_1", "D_7", "D_8", "D_9", "D_63", "D_64", "D_65", "D_129", "D_32767", "flagged_at_d_32766", "flagged_SR-1",
    "flagged_SR", "flagged_SR+1", "flagged_>>SR", "srth_at_8chunk_offset_7", "srth_at_8chunk_offset_0",
    "srth_at_64group_offset_63", "srth_at_64group_offset_0", "dir_plus_zero", "dir_minus_zero",
    "zero_dir_camera_inside", "zero_dir_camera_margin", "zero_dir_camera_lo_edge", "zero_dir_camera_hi_edge",
    "zero_dir_camera_outside_lo", "zero_dir_camera_outside_hi", "ray_pointing_away", "ray_along_face_flagged_unflagged",
    "ray_through_one_corner_voxel", "span_d_lo_gt_0", "span_d_hi_lt_D-1", "table_before_box", "table_after_box",
    "shared_t", "per_ray_t", "R_1", "R_3", "R_4", "R_5", "R_255", "R_256", "R_257",
    # kNN
    "sample_in_voxel_000", "sample_in_voxel_dims-1", "sample_in_degenerate_grid", "tie_incoming_equals_farthest",
    "tie_among_farthest_after_replacement", "d2_zero_first_push", "full_at_d2_zero_then_candidate", "d2_equals_r2_kept",
    "r2_next_step_dropped", "r2_zero", "nnb_partial_minus1_tail", "nnb_zero_not_in_worklist",
    "exactly_K_in_layer0_nearer_in_layer1", "K-1_in_layer0_layer1_overfills", "kernel5_break_after_layer0",
    "kernel5_break_after_layer1", "kernel5_all_three_layers", "K_1", "K_4", "K_8", "K_16", "runs_0_1_2_3_adjacent",
    "runs_of_length_1_adjacent", "layer1_total_1", "label_zero", "label_equal", "label_different", "label_rejected", "seconds_mod10_0",
    "seconds_mod10_1", "seconds_mod10_2")
MARCH_SR = (1, 3, 8, 9, 64, 128)


# ---- exact reference --------------------------------------------------------------------------------
def _geom(sc):
    hy = sc.hyper
    sh = [_I(x) for x in hy.shift]
    vs = [_I(x) for x in hy.scaled_vsize]
    for v in vs:
        assert v > 0 and v & (v - 1) == 0, "the voxel size must be a power of two"
    return sh, vs, [int(x) for x in hy.scaled_vdim]


def _voxel(p, sh, vs, what):
    """floor((p - shift) / vs) per axis on exact integers; p - shift must fit fp32 (the quotient by a
    power of two then does)."""
    return tuple(_fits(p[a] - sh[a], what) // vs[a] for a in range(3))


def exact_grid(sc):
    """build_occ_vox (:706-778) in point order on integers.  Returns the reference-format tensors
    (coor_occ, coor_2_occ [dims], occ_numpnts [max_o], occ_2_pnts [max_o, P]), occ_idx (claims),
    n_slots, n_listed, and `pvox` (voxel of every point, None when outside)."""
    sh, vs, dims = _geom(sc)
    o = sc.opts
    max_o, P = int(o.max_o), int(o.P)
    pts = [[_fits(_I(x), "point") for x in p] for p in sc.xyz]
    inside = lambda c: all(0 <= c[a] < dims[a] for a in range(3))
    pvox = []
    for p in pts:
        c = _voxel(p, sh, vs, "point - shift")
        pvox.append(c if inside(c) else None)
    # claim_occ :296-321
    claimed, occ_2_coor, occ_idx = set(), [None] * max_o, 0
    for i, c in enumerate(pvox):
        if c is None or c in claimed:
            continue
        claimed.add(c)
        tmp, occ_idx = occ_idx, occ_idx + 1
        if tmp < max_o:
            occ_2_coor[tmp] = c
        else:
            j = _reservoir_slot(o.reservoir_seed, 1, i, tmp)
            if j < max_o:
                occ_2_coor[j] = c
    # map_coor2occ :343-361 (coor_2_occ starts again from -1, :735)
    coor_occ = np.zeros(dims, np.int32)
    coor_2_occ = np.full(dims, -1, np.int32)
    n_slots = min(occ_idx, max_o)
    q = [int(x) for x in o.query_size]
    for j in range(n_slots):
        c = occ_2_coor[j]
        coor_2_occ[c] = j
        rng = [range(max(0, c[a] - q[a] // 2), min(dims[a], c[a] + (q[a] + 1) // 2)) for a in range(3)]
        for x in rng[0]:
            for y in rng[1]:
                for z in rng[2]:
                    coor_occ[x, y, z] = 1
    # fill_occ2pnts :385-407
    numpnts = np.zeros(max_o, np.int32)
    lists = np.full((max_o, P), -1, np.int32)
    for i, c in enumerate(pvox):
        if c is None:
            continue
        v = int(coor_2_occ[c])
        if (v >= 0) if o.fix_occ0 else (v > 0):
            tmp = int(numpnts[v])
            numpnts[v] += 1
            if tmp < P:
                lists[v, tmp] = i
            else:
                j = _reservoir_slot(o.reservoir_seed, 2, i, tmp)
                if j < P:
                    lists[v, j] = i
    return types.SimpleNamespace(coor_occ=coor_occ, coor_2_occ=coor_2_occ, occ_numpnts=numpnts, occ_2_pnts=lists,
                                 occ_idx=occ_idx, n_slots=n_slots, n_listed=int(np.minimum(numpnts, P).sum()),
                                 pvox=pvox, pts=pts, slot_coor=occ_2_coor[:n_slots])


def exact_span(sc, r, tt):
    """[d_lo, d_hi] of ray r: the candidates whose t lies in the ray's span through the grid box widened
    by two voxels on every side, in exact rationals (empty: d_hi < d_lo).  `tt`: the ray's depths as
    integers; the third value says whether the ray's line meets the widened box at all.  Every flagged
    candidate lies inside (asserted by exact_query)."""
    sh, vs, dims = _geom(sc)
    c = [_I(x) for x in sc.campos]
    dv = [_I(x) for x in sc.raydir[r]]
    t_in, t_out = None, None   # None: -inf / +inf
    for a in range(3):
        lo, hi = sh[a] - 2 * vs[a], sh[a] + (dims[a] + 2) * vs[a]
        if dv[a] != 0:
            t1, t2 = Fraction(lo - c[a], dv[a]), Fraction(hi - c[a], dv[a])
            t_in = min(t1, t2) if t_in is None else max(t_in, min(t1, t2))
            t_out = max(t1, t2) if t_out is None else min(t_out, max(t1, t2))
        elif c[a] < lo or c[a] > hi:
            return 0, -1, False
    D = len(tt)
    if t_in is not None and t_out is not None and t_in > t_out:
        return 0, -1, False
    d_lo = 0 if t_in is None else bisect.bisect_left(tt, t_in * Q)
    d_hi = D - 1 if t_out is None else bisect.bisect_right(tt, t_out * Q) - 1
    return d_lo, d_hi, True


def exact_query(sc, grid=None):
    """The whole query on integers.  Returns ray_ns [R], ray_d [R, SR], pidx [R, SR, K], loc_w [R, SR, 3]
    (the oracle's dense layout), n_flagged [R] (over the whole table), flagged (per ray: candidate
    indices), d_lo / d_hi [R], traffic = (in-grid voxel words read on the layers visited, kept list
    lengths of the occupied ones; both before any filter), and `trace`: per sample (r, slot) a dict
    of what the kNN went through (used by plantings())."""
    g = grid or exact_grid(sc)
    sh, vs, dims = _geom(sc)
    o = sc.opts
    SR, K, P = int(o.SR), int(o.K), int(o.P)
    R, D = sc.R, sc.D
    campos = [_fits(_I(x), "campos") for x in sc.campos]
    r2 = _I(sc.hyper.r2) * Q
    nlayer = (int(o.kernel_size[0]) + 1) // 2
    semantic = sc.point_labels is not None
    ray_ns = np.zeros(R, np.int32)
    ray_d = np.full((R, SR), -1, np.int32)
    pidx = np.full((R, SR, K), -1, np.int32)
    loc_w = np.zeros((R, SR, 3), np.float32)
    n_flagged = np.zeros(R, np.int64)
    flagged_all, spans, trace = [], [], {}
    n_vox = n_cand = 0
    coor_occ, coor_2_occ = g.coor_occ, g.coor_2_occ
    shared_tt = None if sc.per_ray_t else [_fits(_I(x), "t") for x in sc.t]
    for r in range(R):
        tt = shared_tt if shared_tt is not None else [_fits(_I(x), "t") for x in sc.t[r]]
        assert all(tt[i] < tt[i + 1] for i in range(D - 1)), "depth tables are strictly increasing"
        dv = [_fits(_I(x), "raydir") for x in sc.raydir[r]]
        flagged, pos_of = [], {}
        for d in range(D):
            t = tt[d]
            pos = []
            for a in range(3):
                m = _fits(dv[a] * t, "dir * t")                 # scale Q^2
                assert m % Q == 0
                pos.append(_fits(campos[a] + m // Q, "campos + dir * t"))
            c = _voxel(pos, sh, vs, "position - shift")
            if all(0 <= c[a] < dims[a] for a in range(3)) and coor_occ[c] > 0:   # mask_raypos :433-435
                flagged.append(d)
                if len(flagged) <= SR:
                    pos_of[d] = (pos, c)
        d_lo, d_hi, meets = exact_span(sc, r, tt)
        assert all(d_lo <= d <= d_hi for d in flagged), f"ray {r}: a flagged candidate lies outside its span"
        spans.append((d_lo, d_hi, meets))
        flagged_all.append(flagged)
        n_flagged[r] = len(flagged)
        ray_ns[r] = min(len(flagged), SR)          # cumsum <= SR keeps the first SR (:843-844)
        for s, d in enumerate(flagged[:SR]):
            ray_d[r, s] = d
            pos, f = pos_of[d]
            loc_w[r, s] = [np.float32(p / Q) for p in pos]
            # query_neigh_along_ray_layered :620-680
            ids, buf, kid, far_ind, far2 = [-1] * K, [0] * K, 0, 0, 0
            tr = dict(voxel=f, events=set(), layers=0, kid_after_layer0=None, runs=[])
            cl = int(sc.ray_labels[r]) if semantic else 0
            for layer in range(nlayer):
                tr["layers"] = layer + 1
                for x in range(max(-f[0], -layer), min(dims[0] - f[0], layer + 1)):
                    for y in range(max(-f[1], -layer), min(dims[1] - f[1], layer + 1)):
                        for z in range(max(-f[2], -layer), min(dims[2] - f[2], layer + 1)):
                            if max(abs(x), abs(y), abs(z)) != layer:
                                continue
                            n_vox += 1
                            occ = int(coor_2_occ[f[0] + x, f[1] + y, f[2] + z])
                            if occ < 0:
                                continue
                            kept = min(P, int(g.occ_numpnts[occ]))
                            n_cand += kept
                            if layer == 1:
                                tr["runs"].append(((x, y, z), kept))
                            for gi in range(kept):
                                p = int(g.occ_2_pnts[occ, gi])
                                if semantic:
                                    lv = int(sc.point_labels[p])
                                    if lv == 0:
                                        tr["events"].add("label_zero")
                                    elif lv == cl:
                                        tr["events"].add("label_equal")
                                    elif cl != 0:
                                        tr["events"].add("label_different")
                                    if not (cl == lv or lv == 0 or cl == 0 or (cl != lv and sc.seconds % 10 <= 1)):
                                        tr["events"].add("label_rejected")
                                        continue
                                xv, yv, zv = (_fits(g.pts[p][a] - pos[a], "p - centre") for a in range(3))
                                xx = _fits(xv * xv, "x^2")
                                xy = _fits(yv * yv + xx, "y^2 + x^2")
                                d2 = _fits(zv * zv + xy, "squared distance")
                                if r2 != 0 and d2 > r2:
                                    tr["events"].add(("dropped_d2", d2))
                                    continue
                                if r2 != 0 and d2 == r2:
                                    tr["events"].add("d2_equals_r2_kept")
                                kid += 1
                                if kid - 1 < K:
                                    ids[kid - 1], buf[kid - 1] = p, d2
                                    if kid == 1 and d2 == 0:
                                        tr["events"].add("d2_zero_first_push")
                                    if d2 > far2:
                                        far2, far_ind = d2, kid - 1
                                else:
                                    if d2 == far2:
                                        tr["events"].add("tie_incoming_equals_farthest")
                                    if far2 == 0:
                                        tr["events"].add("full_at_d2_zero_then_candidate")
                                    if d2 < far2:
                                        tr["events"].add("replaced_in_layer%d" % layer)
                                        ids[far_ind], buf[far_ind] = p, d2
                                        far2 = d2
                                        for i in range(K):
                                            if buf[i] > far2:
                                                far2, far_ind = buf[i], i
                                        if K > 1 and sum(b == far2 for b in buf) > 1:
                                            tr["events"].add("tie_among_farthest_after_replacement")
                if layer == 0:
                    tr["kid_after_layer0"] = kid
                if kid >= K:
                    break
            tr["kid"], tr["far2"] = kid, far2
            pidx[r, s] = ids
            trace[(r, s)] = tr
    return dict(ray_ns=ray_ns, ray_d=ray_d, pidx=pidx, loc_w=loc_w, n_flagged=n_flagged, flagged=flagged_all,
                d_lo=np.array([s[0] for s in spans]), d_hi=np.array([s[1] for s in spans]),
                meets=np.array([s[2] for s in spans]), traffic=(n_vox, n_cand), trace=trace)


# ---- plantings ----------------------------------------------------------------------------------------
def plantings(sc, g=None, q=None):
    """name -> where it holds (a list of rays, (ray, slot) samples, voxels or points; or True for a
    property of the whole scene), read off the exact reference's run of this scene."""
    g = g or exact_grid(sc)
    q = q or exact_query(sc, g)
    o = sc.opts
    sh, vs, dims = _geom(sc)
    P, K, SR, max_o = int(o.P), int(o.K), int(o.SR), int(o.max_o)
    R, D = sc.R, sc.D
    out = {}

    def hold(name, where):
        if isinstance(where, (bool, np.bool_)):
            where = bool(where)
        if where is True or (where is not False and len(where) > 0):
            out[name] = where

    N = len(g.pts)
    hold("dims_%d_%d_%d" % tuple(dims), True)
    lat = [[Fraction(p[a] - sh[a], vs[a]) for a in range(3)] for p in g.pts]   # voxel units
    hold("point_on_lower_faces_inside", [i for i in range(N) if g.pvox[i] and all(x.denominator == 1 for x in lat[i])])
    hold("point_on_outer_upper_face_outside", [i for i in range(N) if any(lat[i][a] == dims[a] for a in range(3))])
    hold("point_at_shift", [i for i in range(N) if all(x == 0 for x in lat[i])])
    hold("point_just_outside", [i for i in range(N) if any(-1 < lat[i][a] < 0 for a in range(3))])
    seen, dup = {}, []
    for i, p in enumerate(g.pts):
        if tuple(p) in seen:
            dup.append(i)
        seen[tuple(p)] = i
    hold("duplicate_points", dup)
    occupancy = {}
    for c in g.pvox:
        if c is not None:
            occupancy[c] = occupancy.get(c, 0) + 1
    mapped = lambda c: g.coor_2_occ[c] > 0 or (o.fix_occ0 and g.coor_2_occ[c] == 0)
    for nm, n in (("P-1", P - 1), ("P", P), ("P+1", P + 1), ("3P", 3 * P)):
        hold("voxel_with_" + nm, [c for c, k in occupancy.items() if k == n and mapped(c)])
    if P == 63:
        hold("P_63_full_voxel", [c for c, k in occupancy.items() if k >= 63 and mapped(c)])
    hold("P_64", P == 64)
    hold("n_claimed_max_o-1", g.occ_idx == max_o - 1)
    hold("n_claimed_max_o", g.occ_idx == max_o)
    hold("n_claimed_max_o+1", g.occ_idx == max_o + 1)
    hold("max_o_1", max_o == 1 and g.occ_idx > 1)
    hold("n_slots_%d" % g.n_slots, True)
    first = next((i for i in range(N) if g.pvox[i] is not None), None)
    hold("point0_alone_in_slot0", first == 0 and occupancy[g.pvox[0]] == 1 and g.coor_2_occ[g.pvox[0]] == 0)
    hold("n_points_%d" % N, N <= 1)
    hold("all_points_outside", N > 0 and first is None)
    qs = [int(x) for x in o.query_size]
    hold("query_size_even_anisotropic", any(x % 2 == 0 for x in qs) and len(set(qs)) > 1 and g.n_slots > 0)
    # march
    hold("D_%d" % D, True)
    hold("R_%d" % R, True)
    hold("shared_t" if not sc.per_ray_t else "per_ray_t", True)
    nf = q["n_flagged"]
    hold("flagged_at_d_%d" % (D - 1), [r for r in range(R) if q["ray_d"][r].max() == D - 1])
    hold("flagged_SR-1", [r for r in range(R) if nf[r] == SR - 1])
    hold("flagged_SR", [r for r in range(R) if nf[r] == SR])
    hold("flagged_SR+1", [r for r in range(R) if nf[r] == SR + 1])
    hold("flagged_>>SR", [r for r in range(R) if nf[r] >= 2 * SR + 64 or (nf[r] > SR and nf[r] >= D - 8)])
    off = {r: int(q["ray_d"][r, SR - 1] - q["d_lo"][r]) for r in range(R) if nf[r] >= SR}
    hold("srth_at_8chunk_offset_7", [r for r, x in off.items() if x % 8 == 7])
    hold("srth_at_8chunk_offset_0", [r for r, x in off.items() if x % 8 == 0])
    hold("srth_at_64group_offset_63", [r for r, x in off.items() if x % 64 == 63])
    hold("srth_at_64group_offset_0", [r for r, x in off.items() if x % 64 == 0])
    sign = np.signbit(sc.raydir)
    zero = sc.raydir == 0
    hold("dir_plus_zero", [r for r in range(R) if np.any(zero[r] & ~sign[r])])
    hold("dir_minus_zero", [r for r in range(R) if np.any(zero[r] & sign[r])])
    cam = [_I(x) for x in sc.campos]
    for a in range(3):
        rays = [r for r in range(R) if zero[r, a] and not zero[r].all()]
        if len({bool(sign[r, a]) for r in rays}) < 2:
            continue
        lo, hi, b0, b1 = sh[a] - 2 * vs[a], sh[a] + (dims[a] + 2) * vs[a], sh[a], sh[a] + dims[a] * vs[a]
        case = ("inside" if b0 <= cam[a] < b1 else "lo_edge" if cam[a] == lo else "hi_edge" if cam[a] == hi else
                "margin" if lo < cam[a] < hi else "outside_lo" if cam[a] < lo else "outside_hi")
        hold("zero_dir_camera_" + case, rays)
    box_lo = [sh[a] for a in range(3)]
    box_hi = [sh[a] + dims[a] * vs[a] for a in range(3)]
    dvs = [[_I(x) for x in sc.raydir[r]] for r in range(R)]
    away = lambda r: any((cam[a] < box_lo[a] and dvs[r][a] < 0) or (cam[a] >= box_hi[a] and dvs[r][a] > 0) for a in range(3))
    hold("ray_pointing_away", [r for r in range(R) if away(r) and nf[r] == 0])
    hold("span_d_lo_gt_0", [r for r in range(R) if q["d_hi"][r] >= q["d_lo"][r] > 0 and nf[r] > 0])
    hold("span_d_hi_lt_D-1", [r for r in range(R) if q["d_lo"][r] <= q["d_hi"][r] < D - 1 and nf[r] > 0])
    hold("table_before_box", [r for r in range(R) if q["meets"][r] and not away(r) and q["d_lo"][r] >= D])
    hold("table_after_box", [r for r in range(R) if q["meets"][r] and not away(r) and q["d_hi"][r] < 0])
    # a ray along a face: a coordinate stays exactly on a voxel face while the voxel below is unflagged
    face = []
    for r in range(R):
        for a in range(3):
            if zero[r, a] and (cam[a] - sh[a]) % vs[a] == 0 and nf[r] > 0:
                j = (cam[a] - sh[a]) // vs[a]
                vox = [trace["voxel"] for (rr, s), trace in q["trace"].items() if rr == r]
                below = [tuple(v[b] - (b == a) for b in range(3)) for v in vox]
                if 0 < j < dims[a] and vox and all(g.coor_occ[v] == 1 and g.coor_occ[w] == 0 for v, w in zip(vox, below)):
                    face.append(r)
    hold("ray_along_face_flagged_unflagged", face)
    corners = {(x, y, z) for x in (0, dims[0] - 1) for y in (0, dims[1] - 1) for z in (0, dims[2] - 1)}
    hold("ray_through_one_corner_voxel", [r for r in range(R) if nf[r] > 0 and nf[r] == q["ray_ns"][r] and
                                          len({q["trace"][(r, s)]["voxel"] for s in range(nf[r])} ) == 1 and
                                          q["trace"][(r, 0)]["voxel"] in corners and _only_voxel(sc, r, q)])
    # kNN
    tr = q["trace"]
    hold("K_%d" % K, len(tr) > 0)
    hold("sample_in_voxel_000", [k for k, v in tr.items() if v["voxel"] == (0, 0, 0)])
    hold("sample_in_voxel_dims-1", [k for k, v in tr.items() if v["voxel"] == tuple(d - 1 for d in dims)])
    hold("sample_in_degenerate_grid", [k for k in tr] if min(dims) == 1 else [])
    for ev in ("tie_incoming_equals_farthest", "tie_among_farthest_after_replacement", "d2_zero_first_push",
               "full_at_d2_zero_then_candidate", "d2_equals_r2_kept", "label_zero", "label_equal", "label_different", "label_rejected"):
        hold(ev, [k for k, v in tr.items() if ev in v["events"]])
    r2 = _I(sc.hyper.r2) * Q
    step = (_I(LQ) ** 2)
    hold("r2_next_step_dropped", [k for k, v in tr.items() if ("dropped_d2", r2 + step) in v["events"]] if r2 else [])
    hold("r2_zero", r2 == 0 and len(tr) > 0)
    hold("nnb_partial_minus1_tail", [k for k, v in tr.items() if 0 < v["kid"] < K] if K > 1 else
         [k for k, v in tr.items() if v["kid"] == 0])
    hold("nnb_zero_not_in_worklist", [k for k, v in tr.items() if v["kid"] == 0])
    nearer = []
    for k, v in tr.items():
        if v["layers"] == 1 and v["kid_after_layer0"] == K and _nearer_in_layer1(sc, g, q, k, v):
            nearer.append(k)
    hold("exactly_K_in_layer0_nearer_in_layer1", nearer)
    hold("K-1_in_layer0_layer1_overfills", [k for k, v in tr.items() if v["kid_after_layer0"] == K - 1 and v["kid"] > K
                                            and "replaced_in_layer1" in v["events"]])
    nl = (int(o.kernel_size[0]) + 1) // 2
    if nl == 3:
        hold("kernel5_break_after_layer0", [k for k, v in tr.items() if v["layers"] == 1])
        hold("kernel5_break_after_layer1", [k for k, v in tr.items() if v["layers"] == 2])
        hold("kernel5_all_three_layers", [k for k, v in tr.items() if v["layers"] == 3 and v["kid"] > 0])
    r0123, r11, tot1 = [], [], []
    for k, v in tr.items():
        if v["layers"] < 2:
            continue
        cnt = []
        for x in (-1, 0, 1):
            for y in (-1, 0, 1):
                for z in (-1, 0, 1):
                    if (x, y, z) != (0, 0, 0):
                        cnt.append(dict(v["runs"]).get((x, y, z), 0))
        if any(sorted(cnt[i:i + 4]) == [0, 1, 2, 3] for i in range(23)):
            r0123.append(k)
        runs = [c for c in cnt if c > 0]
        if any(runs[i] == 1 and runs[i + 1] == 1 for i in range(len(runs) - 1)):
            r11.append(k)
        if sum(cnt) == 1:
            tot1.append(k)
    hold("runs_0_1_2_3_adjacent", r0123)
    hold("runs_of_length_1_adjacent", r11)
    hold("layer1_total_1", tot1)
    if sc.point_labels is not None:
        hold("seconds_mod10_%d" % (sc.seconds % 10), True)
    return out


def _only_voxel(sc, r, q):
    """The ray's flagged candidates are all of its in-grid candidates (it touches no other voxel)."""
    sh, vs, dims = _geom(sc)
    tt = [_I(x) for x in (sc.t[r] if sc.per_ray_t else sc.t)]
    cam = [_I(x) for x in sc.campos]
    dv = [_I(x) for x in sc.raydir[r]]
    inside = 0
    for t in tt:
        c = [(cam[a] + dv[a] * t // Q - sh[a]) // vs[a] for a in range(3)]
        inside += all(0 <= c[a] < dims[a] for a in range(3))
    return inside == q["n_flagged"][r]


def _nearer_in_layer1(sc, g, q, key, tr):
    """Some listed point of a layer-1 voxel is nearer to the sample than the farthest kept one."""
    dims = _geom(sc)[2]
    r, s = key
    f = tr["voxel"]
    d = int(q["ray_d"][r, s])
    tt = [_I(x) for x in (sc.t[r] if sc.per_ray_t else sc.t)]
    pos = [_I(sc.campos[a]) + _I(sc.raydir[r][a]) * tt[d] // Q for a in range(3)]
    P = int(sc.opts.P)
    for x in (-1, 0, 1):
        for y in (-1, 0, 1):
            for z in (-1, 0, 1):
                c = (f[0] + x, f[1] + y, f[2] + z)
                if (x, y, z) == (0, 0, 0) or not all(0 <= c[a] < dims[a] for a in range(3)):
                    continue
                occ = int(g.coor_2_occ[c])
                if occ < 0:
                    continue
                for gi in range(min(P, int(g.occ_numpnts[occ]))):
                    p = g.pts[int(g.occ_2_pnts[occ, gi])]
                    if sum((p[a] - pos[a]) ** 2 for a in range(3)) < tr["far2"]:
                        return True
    return False


# ---- rounding scenes ------------------------------------------------------------------------------------
def rounding_scene(variant=0):
    """Non-dyadic family (see the module docstring): THE ORACLE'S FULL-TABLE SCAN IS THE REFERENCE HERE.
    vs = 0.016 from grid_hyperparameters, the cloud against the far end of opt.ranges (coordinates just
    below 10, where one fp32 ulp is 9.5e-7 = 6e-5 voxels), a (9, 7, 5)-sized lattice cloud.  Per-ray
    depth tables hold, for every voxel face the ray crosses on its main axis and for the entry and
    exit of the widened box, the crossing depth and its neighbours one and two nextafter steps either
    side.  The idle direction components are 1e-30 and a subnormal (1e-40), of either sign: ray_span
    divides by them to huge values and to +-inf."""
    import torch
    from sgnerf_amd.hyper import grid_hyperparameters
    rng = np.random.default_rng(21 + variant)
    o = make_opts(SR=128, K=8, P=8)
    vs = np.float32(o.vsize[0] * o.vscale[0])
    n = 300
    idx = rng.integers(0, (9 * 4, 7 * 4, 5 * 4), (n, 3))
    hi = np.array(o.ranges[3:], np.float64)
    xyz = (hi[None] - (np.array([36, 28, 20]) - idx) * (float(vs) / 4)).astype(np.float32)
    xyz[0] = hi.astype(np.float32)            # a point on the range limit itself
    hy = grid_hyperparameters(o, torch.from_numpy(xyz.min(0)), torch.from_numpy(xyz.max(0)))
    shift, dims = hy.shift.astype(np.float64), hy.scaled_vdim
    tiny = (np.float32(1e-30), np.float32(1e-40), np.float32(-1e-30), np.float32(-1e-40), np.float32(0.0), np.float32(-0.0))
    # one camera serves all rays: outside the widened box on axis `variant` (3: on none), inside the cloud on the others
    campos = np.array([shift[a] + (dims[a] / 2 + 0.37) * float(vs) for a in range(3)])
    if variant < 3:
        campos[variant] = shift[variant] - 5.3 * float(vs)
    campos = campos.astype(np.float32)
    dirs = []
    for a in range(3):                        # main axis, both ways, four lengths
        for k in range(4):
            for sgn in (1.0, -1.0):
                d = np.zeros(3, np.float32)
                d[a] = np.float32(sgn * (1.0, 0.7, 1.3, 0.9)[k])
                d[(a + 1) % 3], d[(a + 2) % 3] = tiny[(k + a) % 6], tiny[(k + a + 3) % 6]
                dirs.append(d)
    dirs = np.array(dirs, np.float32)
    D = 0
    rows = []
    for r, d in enumerate(dirs):
        a = int(np.argmax(np.abs(d)))
        faces = [shift[a] + j * float(vs) for j in range(-2, dims[a] + 3)]
        ts = set()
        for f in faces:
            t0 = np.float32((f - float(campos[a])) / float(d[a]))
            if not np.isfinite(t0) or t0 <= 0:
                continue
            lo = t0
            hi_ = t0
            ts.add(t0)
            for k in (1, 2):
                lo = np.nextafter(lo, np.float32(-np.inf))      # steps of t: what ray_span compares
                hi_ = np.nextafter(hi_, np.float32(np.inf))
                ts.update((lo, hi_))
                for sg in (-k, k):                                # steps of the position: what vox_coord sees
                    fk = f + sg * float(np.spacing(np.float32(f)))
                    ts.add(np.float32((fk - float(campos[a])) / float(d[a])))
        ts = sorted(x for x in ts if x > 0)
        if not ts:
            ts = [np.float32(0.5)]
        rows.append(ts)
        D = max(D, len(ts))
    t = np.zeros((len(rows), D), np.float32)
    for r, ts in enumerate(rows):               # pad strictly increasing beyond the last crossing
        last = ts[-1]
        pad = [np.float32(last + (i + 1) * 0.25) for i in range(D - len(ts))]
        t[r] = ts + pad
    assert np.all(t[:, 1:] > t[:, :-1])
    return Scene(name=f"rounding_{variant}", xyz=xyz, hyper=hy, opts=o, campos=campos, raydir=dirs, t=t, per_ray_t=1,
                 point_labels=None, ray_labels=None, seconds=0, expect=(), exact=False)


def oracle_run(sc):
    """(OracleGrid, its query of the scene's rays)."""
    og = oq.OracleGrid(sc.xyz, sc.hyper, sc.opts)
    q = og.query(sc.campos, sc.raydir, sc.t, per_ray_t=bool(sc.per_ray_t), point_labels=sc.point_labels,
                 ray_labels=sc.ray_labels, seconds=sc.seconds)
    return og, q
