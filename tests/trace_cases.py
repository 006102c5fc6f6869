"""Seeded scenes and ray families for the ray-level tests of the traversal, shared by tests/test_trace_edges_cpu.py (oracle
against tests/trace_f64.py, no GPU) and tests/test_trace_edges_gpu.py (library against both).  A scene is a (T, 3, 3) float32
array of triangles; the primitive id of a triangle is its index.  Nothing here looks at a hierarchy."""
import numpy as np

from fovpathtracing_optixcodelatest_amd import scenes

# ---- constants of the tests -------------------------------------------------------------------------------------------------
TINY_NTRI = (1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 21, 64, 65)
# ... and the sizes that bring the sweep to the node counts it is about: a four-wide hierarchy with leaves of up to four
# triangles has about one node per five triangles, so the sizes above end at 12 nodes or so
TINY_NTRI_MORE = (24, 28, 32, 36, 40, 48, 128, 160, 256)
PARTIAL_COUNTS = (1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 255, 257)
REFIT_NTRI = (1, 5, 17, 65)
BUILDERS = {"default": {}, "lbvh": {"FOVPT_BVH": "lbvh"}, "split": {"FOVPT_SPLIT": "1.0"}, "noreinsert": {"FOVPT_REINSERT": "0"},
            "noorder": {"FOVPT_BVH_ORDER": "0"}}
MAX_RATIO_F64 = 500.0       # configurations with a larger M / e (tests/trace_f64.py) are compared with the oracle's bits only

FAMILIES = ("random", "aimed", "axis", "in_plane", "near_tmin")
# Tolerances of the library's (t, u, v) against binary64 on decided hits, per family: relative for t, absolute for u and v.
# Each is 4 x the oracle's own largest deviation from tests/trace_f64.py over every f64-checked configuration below
# (test_tolerances_are_the_measured_ones recomputes them); the library must equal the oracle bit for bit anyway, so the factor
# only absorbs another seed.
# measured: t 1.10e-5 random, 4.22e-5 aimed, 1.45e-6 axis, 1.61e-6 in_plane, 7.82e-5 near_tmin (t ~ 0.01 beside unit triangles);
#           u, v 5.59e-5 random, 3.20e-4 aimed (far origins, grazing), 7.07e-7 axis, 4.43e-6 in_plane, 1.77e-6 near_tmin
TOL_T_REL = {"random": 4.4e-5, "aimed": 1.7e-4, "axis": 5.8e-6, "in_plane": 6.5e-6, "near_tmin": 3.2e-4}
TOL_UV_ABS = {"random": 2.3e-4, "aimed": 1.3e-3, "axis": 2.9e-6, "in_plane": 1.8e-5, "near_tmin": 7.1e-6}


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def _place(tri, scale, offset):
    return (np.asarray(tri, np.float64) * scale + np.asarray(offset, np.float64)).astype(np.float32)


def soup(n, seed, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """n random triangles.  With n >= 8: triangle 1 is an exact duplicate of triangle 0, triangle 2 has zero area (three
    distinct collinear vertices, exactly) and triangles 3 and 4 overlap in one plane z = const.  The special triangles are made
    after scale and offset were applied, so they are exact in the placed scene too."""
    rng = np.random.default_rng(1000 + seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    tri = _place(c + rng.normal(0, 0.25, (n, 3, 3)), scale, offset)
    if n >= 8:
        tri[1] = tri[0]
        grid = np.float32(2.0 ** (np.ceil(np.log2(np.abs(tri).max())) - 18))      # multiples of it below 2^18 * grid add exactly
        a = np.round(tri[2, 0] / grid) * grid
        e = np.round((tri[2, 1] - tri[2, 0]) / grid) * grid
        tri[2] = np.stack([a, a + e, a + e + e]).astype(np.float32)
        tri[3, :, 2] = tri[3, 0, 2]
        tri[4] = tri[3] + (0.5 * (tri[3, 1] - tri[3, 0])).astype(np.float32)       # (neither centroid inside the other)
        tri[4, :, 2] = tri[3, 0, 2]
    return tri


def lattice(k, ntri=None, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """Axis-aligned unit quads on integer coordinates: a floor z = 0, a wall x = 0 and a wall y = k, k x k quads each, a quad
    two triangles sharing a diagonal; the quads of the three planes alternate, so the first ntri triangles hold all three."""
    planes = []
    for i in range(k):
        for j in range(k):
            planes.append([
                [(i, j, 0), (i + 1, j, 0), (i + 1, j + 1, 0), (i, j + 1, 0)],
                [(0, i, j), (0, i + 1, j), (0, i + 1, j + 1), (0, i, j + 1)],
                [(i, k, j), (i, k, j + 1), (i + 1, k, j + 1), (i + 1, k, j)]])
    tris = []
    for three in planes:
        for p in three:
            tris += [[p[0], p[1], p[2]], [p[0], p[2], p[3]]]
    tri = _place(np.array(tris, np.float64), scale, offset)
    return tri if ntri is None else tri[:ntri]


def cornell():
    return triangles_of(scenes.cornell_box())


def triangles_of(model):
    return np.concatenate([m.vertex[m.index.astype(np.int64)] for m in model.meshes]).astype(np.float32)


def model_of(tri):
    tri = np.ascontiguousarray(tri, np.float32)
    return scenes.Model([scenes.TriangleMesh(tri.reshape(-1, 3).copy(), np.arange(3 * len(tri), dtype=np.uint32).reshape(-1, 3), scenes.matte((1, 1, 1)))])


def moved(tri, seed):
    """The vertices of an animated frame: every triangle displaced and turned a little, by a smooth function of its position."""
    rng = np.random.default_rng(2000 + seed)
    t = np.asarray(tri, np.float64)
    size = max(float(np.ptp(t.reshape(-1, 3), axis=0).max()), 1e-3)
    phase = rng.uniform(0, 6.28, 3)
    return (t + 0.15 * size * np.sin(t[..., [1, 2, 0]] * (2.0 / size) + phase)).astype(np.float32)


# ---- ray families -----------------------------------------------------------------------------------------------------------
def _bounds(tri):
    v = np.asarray(tri, np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    ext = np.maximum(hi - lo, 0.05 * (hi - lo).max())
    return lo, hi, ext


def _unit(tri):
    """A typical edge length of the scene."""
    t = np.asarray(tri, np.float64)
    return float(np.median(np.linalg.norm(t[:, 1] - t[:, 0], axis=1)))


def _normalized(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _from_afar(rng, tri, target, standoff):
    """Origins for rays through the given points: in and around the scene's bounds, or, with a standoff, at least that far
    from the point."""
    lo, hi, ext = _bounds(tri)
    n = len(target)
    o = lo - 0.3 * ext + rng.random((n, 3)) * 1.6 * ext
    if standoff > 0:
        o = target - _normalized(target - o) * standoff * (1.0 + rng.random((n, 1)))
    return o


def rays_random(tri, n, seed, standoff=0.0):
    """Origins in and around the bounds, directions towards random points of them (as tests/test_gpu_parity.py draws them)."""
    rng = np.random.default_rng(seed)
    lo, hi, ext = _bounds(tri)
    target = lo + rng.random((n, 3)) * ext
    o = _from_afar(rng, tri, target, standoff).astype(np.float32)
    return o, _normalized(target - o).astype(np.float32)


AIMED_KINDS = ("centroid", "vertex", "edge_mid", "edge_quarter", "reversed")


def rays_aimed(tri, n, seed, standoff=0.0, kind=None):
    """From random origins at points of random triangles: the centroid, a vertex, the middle of an edge, a quarter point of an
    edge -- and, so that the family misses too, away from a centroid.  Equal shares, or one kind only."""
    rng = np.random.default_rng(seed)
    t = np.asarray(tri, np.float32)
    k = rng.choice(_plain_triangles(t), n)                 # (u, v, t on a triangle of zero area are 0 / 0: nothing to aim at)
    a, b = rng.integers(0, 3, n), rng.integers(1, 3, n)
    va, vb = t[k, a], t[k, (a + b) % 3]
    which = np.arange(n) % len(AIMED_KINDS) if kind is None else np.full(n, AIMED_KINDS.index(kind))
    centroid = ((t[k, 0] + t[k, 1] + t[k, 2]) / np.float32(3)).astype(np.float32)
    points = [centroid, va, (va + vb) * np.float32(0.5), va + (vb - va) * np.float32(0.25), centroid]
    target = np.choose(which[:, None], points).astype(np.float64)
    o = _from_afar(rng, tri, target, standoff).astype(np.float32)
    d = _normalized(target - o)
    d[which == AIMED_KINDS.index("reversed")] *= -1.0
    return o, d.astype(np.float32)


def rays_axis(tri, n, seed, standoff=0.0):
    """d = +-e_k with the other two components exactly +0.0 and, in a second copy of the same rays, -0.0.  The two free
    coordinates of an origin are those of a vertex or of the middle of two vertices, so the ray runs exactly through vertices,
    along edges, diagonals and wall planes; the third lies outside the bounds, or (every fourth origin) is a vertex's as well:
    an origin exactly on a wall's coordinate.  The second half repeats the origins with the free coordinates moved to a generic
    point nearby.  Returns (origins, dirs, interior): interior marks the second half."""
    rng = np.random.default_rng(seed)
    v = np.asarray(tri, np.float32).reshape(-1, 3)
    lo, hi, ext = _bounds(tri)
    unit = _unit(tri)
    b = max(1, n // 4)
    axis, sign = np.arange(b) % 3, np.where((np.arange(b) // 3) % 2 == 0, 1.0, -1.0)
    p, q = v[rng.integers(0, len(v), b)], v[rng.integers(0, len(v), b)]
    o = np.where((rng.random((b, 1)) < 0.5), p, (p + q) * np.float32(0.5)).astype(np.float32)
    away = np.maximum(np.maximum(0.5 * ext[axis], unit), standoff) * (1.0 + rng.random(b))
    outside = np.where(sign > 0, lo[axis] - away, hi[axis] + away).astype(np.float32)
    on_wall = np.arange(b) % 4 == 3
    o[np.arange(b), axis] = np.where(on_wall, o[np.arange(b), axis], outside)
    oi = (o.astype(np.float64) + rng.uniform(0.1, 0.4, (b, 3)) * unit).astype(np.float32)
    oi[np.arange(b), axis] = o[np.arange(b), axis]
    d = np.zeros((b, 3), np.float32)
    d[np.arange(b), axis] = sign
    dneg = np.where(d == 0, np.float32(-0.0), d).astype(np.float32)
    assert np.signbit(dneg).sum() >= 2 * b and not np.signbit(d[d == 0]).any()
    interior = np.repeat([False, False, True, True], b)
    return np.concatenate([o, o, oi, oi]), np.concatenate([d, dneg, d, dneg]), interior


def _plain_triangles(tri):
    t = np.asarray(tri, np.float32)
    return np.flatnonzero(np.cross((t[:, 1] - t[:, 0]).astype(np.float64), (t[:, 2] - t[:, 0]).astype(np.float64)).any(axis=1))


def _axis_aligned_triangles(tri):
    t = np.asarray(tri, np.float32)
    flat = ((t[:, 1] == t[:, 0]) & (t[:, 2] == t[:, 0])).sum(1) == 1          # exactly one coordinate shared by the three vertices
    return np.intersect1d(np.flatnonzero(flat), _plain_triangles(t))


def rays_in_plane(tri, n, seed, standoff=0.0):
    """Origin and direction inside the plane of an axis-aligned triangle, from beside the triangle through it.  Both are sums of
    the triangle's edges, so the coordinate normal to the wall is the wall's and the direction's is exactly 0: det is exactly 0
    for every triangle of that wall.  (In the plane of any other triangle det is rounding noise, and so are u, v and t: there
    the contract decides nothing, and a brute force and a hierarchy may differ.)  No rays for a scene without such a triangle."""
    rng = np.random.default_rng(seed)
    t = np.asarray(tri, np.float32)
    walls = _axis_aligned_triangles(t)
    if len(walls) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    k = rng.choice(walls, n)
    v0, e1, e2 = t[k, 0], t[k, 1] - t[k, 0], t[k, 2] - t[k, 0]
    f32 = np.float32
    ab = rng.uniform(0.1, 0.45, (n, 2)).astype(f32)
    target = v0 + ab[:, :1] * e1 + ab[:, 1:] * e2
    phi = rng.uniform(0, 2 * np.pi, n)
    out = np.cos(phi)[:, None].astype(f32) * e1 + np.sin(phi)[:, None].astype(f32) * e2
    out = (out / np.linalg.norm(out, axis=1, keepdims=True).astype(f32)).astype(f32)
    dist = (np.maximum(standoff, 0.0) + (1.5 + rng.random(n)) * np.linalg.norm(e1 + e2, axis=1)).astype(f32)
    o = (target + out * dist[:, None]).astype(f32)
    d = -out
    return o, d.astype(f32)


NEAR_TMIN_EPS = (0.0, 0.005, 0.0099, 0.0101, 0.02)


def rays_near_tmin(tri, n, seed):
    """Rays that start on a surface (t = 0 is below tmin and must be skipped) or just in front of one, the surface at
    t = 0.005, 0.0099, 0.0101 and 0.02 (directions of unit length) -- and, where the scene has axis-aligned triangles, a fifth as
    many rays straight at such a wall from float32(0.01) in front of it: where the wall's coordinate is 0 and its edges are
    powers of two, t is tmin to the bit, and tmin is exclusive."""
    rng = np.random.default_rng(seed)
    t = np.asarray(tri, np.float32).astype(np.float64)
    k = rng.choice(_plain_triangles(tri), n)
    v0, e1, e2 = t[k, 0], t[k, 1] - t[k, 0], t[k, 2] - t[k, 0]
    ab = rng.uniform(0.15, 0.4, (n, 2))
    p = v0 + ab[:, :1] * e1 + ab[:, 1:] * e2
    nrm = _normalized(np.cross(e1, e2))
    d = _normalized(rng.normal(0, 1, (n, 3)))
    flat = np.abs((d * nrm).sum(1)) < 0.3
    d[flat] = _normalized(d[flat] + nrm[flat] * np.where((d[flat] * nrm[flat]).sum(1, keepdims=True) < 0, -1.0, 1.0))
    eps = np.array(NEAR_TMIN_EPS)[np.arange(n) % len(NEAR_TMIN_EPS)][:, None]
    o, d = (p - d * eps).astype(np.float32), d.astype(np.float32)
    walls = _axis_aligned_triangles(tri)
    if len(walls):
        m = max(1, n // 5)
        k = rng.choice(walls, m)
        t32 = np.asarray(tri, np.float32)
        ab = rng.uniform(0.15, 0.4, (m, 2)).astype(np.float32)
        ow = t32[k, 0] + ab[:, :1] * (t32[k, 1] - t32[k, 0]) + ab[:, 1:] * (t32[k, 2] - t32[k, 0])
        axis = np.argmax((t32[k, 1] == t32[k, 0]) & (t32[k, 2] == t32[k, 0]), axis=1)
        side = np.where(np.arange(m) % 2 == 0, np.float32(1), np.float32(-1))
        ow[np.arange(m), axis] = t32[k, 0][np.arange(m), axis] + side * np.float32(0.01)
        dw = np.zeros((m, 3), np.float32)
        dw[np.arange(m), axis] = -side
        o, d = np.concatenate([o, ow]), np.concatenate([d, dw])
    return o, d


def rays(tri, family, n, seed, standoff=0.0):
    """(origins, dirs) of one family, about n rays."""
    if family == "random":
        return rays_random(tri, n, seed, standoff)
    if family == "aimed":
        return rays_aimed(tri, n, seed, standoff)
    if family == "axis":
        return rays_axis(tri, n, seed, standoff)[:2]
    if family == "in_plane":
        return rays_in_plane(tri, n, seed, standoff)
    if family == "near_tmin":
        return rays_near_tmin(tri, n, seed)
    raise ValueError(family)


MIX = {"random": 400, "aimed": 400, "axis": 360, "in_plane": 140, "near_tmin": 200}


def mixed(tri, seed, standoff=0.0, families=FAMILIES, thin=1):
    """About 1500 / thin rays of the given families -> (origins, dirs, family index per ray into FAMILIES)."""
    os_, ds, fs = [], [], []
    for f in families:
        o, d = rays(tri, f, max(4, MIX[f] // thin), seed * 16 + FAMILIES.index(f), standoff)
        os_.append(o), ds.append(d), fs.append(np.full(len(o), FAMILIES.index(f)))
    return np.concatenate(os_), np.concatenate(ds), np.concatenate(fs)


# ---- the configurations the GPU tests run, each with whether it is also held against binary64 ----------------------------------
class Case:
    def __init__(self, name, tri, f64, standoff=0.0, families=FAMILIES, seed=1):
        self.name, self.tri, self.f64, self.standoff, self.families, self.seed = name, tri, f64, standoff, families, seed

    def rays(self, thin=1):
        return mixed(self.tri, self.seed, self.standoff, self.families, thin)


EXACT_FAMILIES = ("aimed", "axis", "in_plane", "near_tmin")


def tiny_cases(kind):
    if kind == "soup":
        return [Case("soup%d" % n, soup(n, n), True, seed=n) for n in TINY_NTRI + TINY_NTRI_MORE]
    return [Case("lattice[:%d]" % n, lattice(2 if n <= 24 else 4 if n <= 96 else 6 if n <= 216 else 7, n), True, seed=n) for n in TINY_NTRI + TINY_NTRI_MORE if n >= 2]


def exact_cases():
    return [Case("lattice3", lattice(3), True, families=EXACT_FAMILIES, seed=31), Case("cornell", cornell(), True, families=EXACT_FAMILIES, seed=32)]


SHIFT = (1000.0, -2000.0, 500.0)
FAR = (1e5, 1e5, 1e5)


def magnitude_cases():
    """(the f64 flag says M / e <= MAX_RATIO_F64 for this configuration; tests/test_trace_edges_cpu.py asserts that it is so)"""
    out = []
    for name, make, f64 in (("lattice3", lambda **kw: lattice(3, **kw), (True, True, False, True, False, False, True)),
                            ("soup40", lambda **kw: soup(40, 40, **kw), (True, True, False, False, False, False, False))):
        out += [Case(name + "*1e3", make(scale=1e3), f64[0], seed=41),
                Case(name + "*1e5", make(scale=1e5), f64[1], seed=42),
                Case(name + "+shift", make(offset=SHIFT), f64[2], seed=43),
                Case(name + "*10+shift", make(scale=10.0, offset=SHIFT), f64[3], seed=44),
                Case(name + "*100+1e5", make(scale=100.0, offset=FAR), f64[4], seed=45),
                Case(name + "+1e5", make(offset=FAR), f64[5], seed=46),
                Case(name + "*0.01", make(scale=0.01), f64[6], standoff=1.0, seed=47),
                # (centimetre triangles from 1500 units away: the slab test's own rounding is larger than the boxes)
                Case(name + "*0.01 far", make(scale=0.01), False, standoff=1500.0, seed=48)]
    return out


def rounds_case():
    return Case("soup300", soup(300, 300), True, families=("random", "aimed"), seed=50)


def rounds_rays(case, n):
    """n rays for the rounds-and-refills test: random and aimed in equal parts."""
    o1, d1 = rays_random(case.tri, n - n // 2, 51)
    o2, d2 = rays_aimed(case.tri, n // 2, 52)
    fam = np.concatenate([np.full(len(o1), FAMILIES.index("random")), np.full(len(o2), FAMILIES.index("aimed"))])
    return np.concatenate([o1, o2]), np.concatenate([d1, d2]), fam


def refit_cases():
    return [Case("moved%d" % n, moved(soup(n, n), n), True, seed=60 + n) for n in REFIT_NTRI]


def all_cases():
    out = tiny_cases("soup") + tiny_cases("lattice") + exact_cases() + magnitude_cases() + refit_cases()
    assert len({c.name for c in out}) == len(out)          # (the tests cache their references by name)
    return out
