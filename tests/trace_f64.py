"""The hit contract of the traversal in binary64: a second, independent statement (numpy, brute force).

Written from DESIGN.md ("ray/triangle: Moeller-Trumbore ... hit iff tmin < t < tmax (0.01, 1e16); closest = min t, ties ->
lowest global primitive id; occlusion = any candidate on a front-facing triangle, det = e1.(d x e2) > 0") and from the
reference's text (deviceProgram.cu:224-248: the occlusion ray culls back faces and does not terminate on the first hit;
:284-300: any hit sets the payload, a miss clears it).  It shares no code with oracle/: binary64 arithmetic on the binary32
inputs, vectorised over the rays, a loop over the triangles.

binary32 and binary64 may differ on a ray that grazes an edge, starts next to tmin, runs inside a triangle's plane or sees
two surfaces at one distance.  Such a ray is UNDECIDED and only rays that are DECIDED may be compared with binary32 results:

    for every triangle (those whose normal e1 x e2 is exactly zero left out: det is exactly 0 for every ray)
      * |det| is exactly 0 or above 1e-6 |e1| |e2| |d|
      * min(u, v, 1 - u - v) is farther than m / cos from 0
      * if the ray passes inside the triangle, t is farther than m (t + L) / cos from 0.01
    and the two smallest accepted t differ by more than 1e-4 relative (an exact copy of an earlier triangle left out: same
    vertices in the same order give the same t, u, v in any arithmetic, and the contract gives the hit to the lower id),

with m = 64 * 2^-24 * M / e, M the largest |coordinate| among the vertices and the batch's origins, e the triangle's shortest
edge, L its longest and cos = |det| / (|e1 x e2| |d|).  2^-24 M / e is the relative error of an edge computed in binary32 from
vertices of magnitude M; 64 is the slack for the operations that follow.  The margin of t is relative to t + L and not to t
alone: t comes out of (o - v0) . n, whose rounding error grows with |o - v0| <= t |d| + L, so next to tmin = 0.01 a margin
relative to t would understate it on triangles that are large beside 0.01.  1 / cos is the amplification at grazing
incidence: u, v and t are quotients by det, which is |e1 x e2| |d| cos, while the rounding errors of their numerators do not
shrink with cos (without it, rays aimed at edges disagreed with the binary32 brute force on 3 of 32 000, all of them with
cos < 1e-3).  A ray that passes a triangle of zero area within rounding of its segment is undecided as well: binary32 sees a
det of rounding noise there and u, v, t that are noise over noise.  None of the constants was fitted to what the library
computes.
"""
import numpy as np

TMIN = 0.01      # deviceProgram.cu:41
TMAX = 1e16      # deviceProgram.cu:42
MISS = 0xFFFFFFFF

MARGIN = 64.0 * 2.0 ** -24
DET_REL = 1e-6
TIE_REL = 1e-4


def magnitude(tri, origins):
    return float(max(np.abs(np.asarray(tri, np.float64)).max(), np.abs(np.asarray(origins, np.float64)).max()))


def shortest_edge(tri):
    """Per triangle; inf for a triangle whose normal is exactly zero (it takes no part in the margins)."""
    t = np.asarray(tri, np.float32).astype(np.float64)
    e = np.stack([np.linalg.norm(t[:, 1] - t[:, 0], axis=1), np.linalg.norm(t[:, 2] - t[:, 0], axis=1), np.linalg.norm(t[:, 2] - t[:, 1], axis=1)])
    flat = ~np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).any(axis=1)
    return np.where(flat, np.inf, e.min(0))


def magnitude_ratio(tri, origins):
    """M / e of a configuration: the largest of the per-triangle ratios the margins are built from."""
    return magnitude(tri, origins) / float(shortest_edge(tri).min())


def trace_f64(tri, origins, dirs):
    """tri (T, 3, 3), origins / dirs (n, 3): binary32 values.  Returns prim (uint32, MISS for none), tuv (n, 3) float64,
    occluded (uint8) and decided (bool), per ray."""
    tri = np.asarray(tri, np.float32).astype(np.float64)
    o = np.asarray(origins, np.float32).astype(np.float64)
    d = np.asarray(dirs, np.float32).astype(np.float64)
    n = o.shape[0]
    M = magnitude(tri, o) if n else 0.0
    dlen = np.linalg.norm(d, axis=1)
    best = np.full(n, np.inf)
    second = np.full(n, np.inf)
    prim = np.full(n, MISS, np.uint32)
    bu, bv = np.zeros(n), np.zeros(n)
    occluded = np.zeros(n, bool)
    decided = np.ones(n, bool)
    for k in range(tri.shape[0]):
        if k and (tri[:k] == tri[k]).all(axis=(1, 2)).any():
            continue                                       # an exact copy: never the closest by the tie-break, occludes what the first does
        v0, v1, v2 = tri[k]
        e1, e2 = v1 - v0, v2 - v0
        nrm = np.cross(e1, e2)
        l1, l2, l3 = np.linalg.norm(e1), np.linalg.norm(e2), np.linalg.norm(v2 - v1)
        if not nrm.any():
            e = e1 if l1 >= l2 else e2                     # zero area: never a hit, but no verdict on a ray through the segment
            decided &= np.abs(((o - v0) * np.cross(d, e)).sum(1)) > MARGIN * 4.0 * M * dlen * max(l1, l2)
            continue
        m = MARGIN * M / min(l1, l2, l3)
        det = -(d @ nrm)                                   # e1 . (d x e2) = -d . (e1 x e2): exactly 0 for a ray in the plane
        flat = det == 0.0
        decided &= flat | (np.abs(det) > DET_REL * l1 * l2 * dlen)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = 1.0 / det
            s = o - v0
            u = (s * np.cross(d, e2)).sum(1) * inv
            q = np.cross(s, e1)
            v = (d * q).sum(1) * inv
            t = (q @ e2) * inv
            inside = np.minimum(np.minimum(u, v), 1.0 - u - v)
            cos = np.abs(det) / (np.linalg.norm(nrm) * dlen)
            decided &= flat | (np.abs(inside) * cos > m)
            decided &= flat | ~(inside > 0.0) | (np.abs(t - TMIN) > m * (t + max(l1, l2, l3) / dlen) / cos)
            ok = ~flat & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t > TMIN) & (t < TMAX)
        occluded |= ok & (det > 0.0)
        closer = ok & (t < best)                           # strict: on equal t the lower primitive id stays
        second = np.where(closer, best, np.where(ok, np.minimum(second, t), second))
        best = np.where(closer, t, best)
        bu, bv = np.where(closer, u, bu), np.where(closer, v, bv)
        prim[closer] = k
    with np.errstate(invalid="ignore"):
        decided &= ~np.isfinite(second) | (second - best > TIE_REL * best)
    tuv = np.stack([np.where(prim != MISS, best, 0.0), bu, bv], axis=1)
    return prim, tuv, occluded.astype(np.uint8), decided
