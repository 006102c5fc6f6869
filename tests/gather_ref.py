"""numpy integer restatement of the multi-GPU gather plan (include/fovpt.h, fovpt_gather_plan / _pack / _unpack; k_plan_owner,
k_plan_scan, k_plan_fill, k_gather_pack and k_gather_unpack in csrc/wavefront.hip): the definition the device plan matches index
by index.

    writer   each pixel's last writer among the frame's passes, PAINTED (reconstruct_ref.writers): its pass p and its anchor, from
             which the launch index (lx, ly) = ((anchor - offset) mod 2^32) // factor follows, as in packet_ref.owners
    owner    (lx // tile_w + 3 * (ly // tile_h) + p) % world; tile_w <= 0 means 8, tile_h <= 0 means 4; 255 for a pixel without a
             writer; world 1: rank 0 owns every written pixel
    plan     per rank the flat pixel indices y * width + x it owns, ASCENDING, and their counts
    pack     packed[k] = frame[plan[rank][k]]
    unpack   target[plan[r][k]] = gathered[r * stride + k] for every rank r; pixels nobody owns keep the target's words

Nothing here searches for a writer, so it shares nothing with find_last_writer (csrc/fovpt_pixel.h), which the kernels use."""
import numpy as np

import reconstruct_ref as rr

NOBODY = 255
M32 = 0xffffffff
BLOCK, SCAN_THREADS, WAVE = 256, 1024, 64          # k_plan_owner / k_plan_fill's block, k_plan_scan's block, a wavefront
MOVE_GRID, MOVE_BLOCK = 2048, 256                  # the cap on k_gather_pack / k_gather_unpack's grid and their block


def tile_of(tile):
    tw, th = tile if tile is not None else (0, 0)
    return (tw if tw > 0 else 8), (th if th > 0 else 4)


def launch_map(size, gaze, radii, uniform):
    """-> (pass, lx, ly) per pixel, (h, w) int64 each, of the pixel's last writer; pass -1: nobody writes it."""
    w, h = size
    r_inner, r_outer = radii if radii is not None else (0, 0)
    _, pas, ax, ay = rr.writers(w, h, gaze, r_inner, r_outer, uniform)
    lx, ly = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for p, (gw, gh, fac, fill, ox, oy, _, _) in enumerate(rr.frame_passes(w, h, gaze, r_inner, r_outer, uniform)):
        sel = pas == p
        lx[sel] = ((ax[sel] - ox) & M32) // fac        # (anchor = (l * factor + off) mod 2^32 and l * factor < 2^32)
        ly[sel] = ((ay[sel] - oy) & M32) // fac
        assert (lx[sel] < gw).all() and (ly[sel] < gh).all()
    return pas, lx, ly


def owner_map(size, gaze, radii, uniform, world, tile=None):
    """-> (h, w) uint8: the rank that owns each pixel, NOBODY for a pixel without a writer."""
    assert 1 <= world <= 64
    tw, th = tile_of(tile)
    pas, lx, ly = launch_map(size, gaze, radii, uniform)
    own = (lx // tw + 3 * (ly // th) + pas) % world
    return np.where(pas >= 0, own, NOBODY).astype(np.uint8)


def plan_of(owner, world):
    """owner map -> (per rank the ascending flat pixel indices as int64, the counts)."""
    flat = np.asarray(owner).reshape(-1)
    lists = [np.flatnonzero(flat == r).astype(np.int64) for r in range(world)]
    return lists, [len(a) for a in lists]


def plan(size, gaze, radii, uniform, world, tile=None):
    return plan_of(owner_map(size, gaze, radii, uniform, world, tile), world)


def pack(frame_words, lists, rank):
    return np.asarray(frame_words).reshape(-1)[lists[rank]].copy()


def unpack(gathered, stride, lists, target):
    """gathered: flat, rank r's words at r * stride.  Writes target (flat view of it) in place and returns it."""
    gathered = np.asarray(gathered).reshape(-1)
    flat = target.reshape(-1)
    for r, idx in enumerate(lists):
        assert len(idx) <= stride
        flat[idx] = gathered[r * stride:r * stride + len(idx)]
    return target


# ---- what a case makes the kernels do: measured on the owner map, for tests/test_gather_plan_cpu.py ---------------------------------
def shape_of(owner, world):
    """-> dict(npix, blocks, per, holes, counts, empty_ranks, owners_per_wave (min, max over the waves that hold a written pixel),
    last_block (pixels in the last block), scan_last (the last thread of k_plan_scan with a chunk, the blocks in that chunk))."""
    flat = np.asarray(owner).reshape(-1)
    npix = flat.size
    blocks = (npix + BLOCK - 1) // BLOCK
    per = (blocks + SCAN_THREADS - 1) // SCAN_THREADS
    counts = [int((flat == r).sum()) for r in range(world)]
    per_wave = []
    for b in range(0, npix, WAVE):
        o = np.unique(flat[b:b + WAVE])
        o = o[o != NOBODY]
        if o.size:
            per_wave.append(int(o.size))
    last_thread = (blocks - 1) // per
    return dict(npix=npix, blocks=blocks, per=per, holes=int((flat == NOBODY).sum()), counts=counts,
                empty_ranks=sum(1 for c in counts if c == 0), owners_per_wave=(min(per_wave), max(per_wave)) if per_wave else (0, 0),
                last_block=npix - (blocks - 1) * BLOCK, scan_last=(last_thread, blocks - last_thread * per))
