"""The two scenes of the build-stage tests that tests/trace_cases.py does not have.  A scene is a (T, 3, 3) float32 array."""
import numpy as np

import trace_cases as tc


def cards(k=14, slivers=8, seed=3):
    """A wall of 2 k^2 small triangles (jittered quads in the plane z = 0) and `slivers` long thin triangles that cross it
    diagonally a little in front of it: what spatial splits cut and what reinsertion moves -- on the Morton curve a sliver lies
    among the small triangles around its centroid, and its box covers a good part of the wall."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing="ij"), axis=-1).astype(np.float64)
    g = np.concatenate([g + rng.uniform(-0.2, 0.2, g.shape), rng.uniform(-0.02, 0.02, g.shape[:2] + (1,))], axis=-1)
    tris = []
    for i in range(k):
        for j in range(k):
            a, b, c, d = g[i, j], g[i + 1, j], g[i + 1, j + 1], g[i, j + 1]
            tris += [[a, b, c], [a, c, d]]
    for s in range(slivers):
        x0, y0 = rng.uniform(0, 0.3 * k, 2)
        x1, y1 = rng.uniform(0.7 * k, k, 2)
        if s % 2:
            y0, y1 = y1, y0
        z = 0.05 + 0.01 * s
        tris.append([(x0, y0, z), (x1, y1, z), (x1 - 0.05, y1 + 0.08, z + 0.01)])
    return np.array(tris, np.float64).astype(np.float32)


def duplicates(same=200, others=50, seed=4):
    """`same` copies of one triangle beside `others` ordinary ones: equal keys (the index tie-break of the Karras tree) and equal
    boxes (PLOC's forced pairing)."""
    rng = np.random.default_rng(seed)
    one = np.array([[0.1, 0.2, 0.3], [0.6, 0.25, 0.35], [0.3, 0.7, 0.2]])
    rest = tc.soup(others, 9)
    return np.concatenate([np.tile(one[None], (same, 1, 1)), rest.astype(np.float64) * 0.5 + 1.5]).astype(np.float32)[rng.permutation(same + others)]
