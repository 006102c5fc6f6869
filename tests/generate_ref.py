"""What the generate stage of a wavefront job must leave behind, as far as it is bookkeeping: stated in integer numpy from the
description of the stage (include/fovpt.h, fovpt_debug_generate), not from the kernels' source.  The
camera rays themselves -- ring test, generator words, jitter, direction, backplate -- are the oracle's (orc_camera_rays).

A job is a list of passes (resolve_ref.Pass) placed in the job's arrays by job(): every pass runs its launch rows [row0, row1)
-- all of them, or a chunk of an oversized launch -- as pass number frame_pass of the caller's frame.

  slot of (pass, launch index (lx, ly), sample s)  = slot_base + ((ly - row0) * gw + lx) * spp + s
  launch record of (pass, (lx, ly))                = launch_base + (ly - row0) * gw + lx           (both relative to the chunk)
  owner of (pass, (lx, ly))                        = (lx // tile_w + 3 * (ly // tile_h) + frame_pass) % world
  a slot is LIVE when it lies in [slot_begin, slot_end), its launch index passes the ring test and belongs to this rank.

A launch walks an index space in block iterations of 256 entries, iteration m on block m % grid; the live entries of a block go
to queue shard sel_first + (block & mask): all eight shards (sel 0: first 0, mask 7) or one half (sel 1: 0, 3; sel 2: 4, 3).
  k_generate        the sample slots themselves: entry slot - slot_begin
  k_generate_owned  (world > 1, all slots, sel 0, and only when the space below is no larger than the slots) per pass the tile
                    rows the job's launch rows touch x per_row = ceil(tiles in a row / world) tiles x tile_w * tile_h launch
                    indices x spp samples, rounded up to whole iterations, the passes one after the other.  Tile k of tile row
                    ty is tile column first + k * world with first = (rank + world - (3 * ty + frame_pass) % world) % world.
So the SHARD of every live slot, and with it the queue counters, are determined, although the position inside a shard is not.

`mut` names ONE deliberate error (MUTATIONS) for tests/test_generate_cpu.py, which shows that the cases can tell."""
import numpy as np

from resolve_ref import Pass, launch_pass, layout, render_passes          # noqa: F401 (the passes and their layout are resolve_ref's)

BLOCK, SHARDS = 256, 8
MUTATIONS = ("record_not_chunk_relative", "owner_without_frame_pass", "owner_ty_not_tripled", "owned_slot_without_row0")


def job(passes, rows=None):
    """Places the passes in the job's arrays -> (sample slots, launch records).  rows = (row0, row1): the job is that chunk of
    launch rows of its one pass."""
    for p, P in enumerate(passes):
        P.frame_pass, P.row0, P.row1 = p, 0, P.gh
    if rows is None:
        return layout(passes)
    assert len(passes) == 1 and 0 <= rows[0] < rows[1] <= passes[0].gh
    P = passes[0]
    full, P.gh = P.gh, rows[1] - rows[0]                                   # layout() sizes a pass by its rows
    out = layout(passes)
    P.gh, P.row0, P.row1 = full, rows[0], rows[1]
    return out


def launch_indices(P):
    """(n, 2) uint32 (lx, ly) of the job's launch indices of pass P, in launch-record order."""
    ly, lx = np.meshgrid(np.arange(P.row0, P.row1, dtype=np.int64), np.arange(P.gw, dtype=np.int64), indexing="ij")
    return np.stack([lx.ravel(), ly.ravel()], axis=1).astype(np.uint32)


def shard_capacity(slots):
    return slots // SHARDS + 512


def chains(slots):
    """The two chains of a job that is split: (sel, slot_begin, slot_end); the first a whole number of block iterations."""
    half = slots // 2 // BLOCK * BLOCK
    return [(1, 0, half), (2, half, slots)]


def owner(P, lx, ly, tile, world, mut=None):
    ty = ly // tile[1]
    rot = (ty if mut == "owner_ty_not_tripled" else 3 * ty) + (0 if mut == "owner_without_frame_pass" else P.frame_pass)
    return (lx // tile[0] + rot) % world


def record_of(P, lx, ly, mut=None):
    return P.launch_base + (ly if mut == "record_not_chunk_relative" else ly - P.row0) * P.gw + lx


def slot_of(P, lx, ly, s, relative=True):
    return P.slot_base + ((ly - P.row0 if relative else ly) * P.gw + lx) * P.spp + s


def owned_space(P, tile, world):
    """-> (tile rows, the rank's tiles per tile row at most, entries) of the padded index space of pass P."""
    tw, th = tile
    tiles_x = (P.gw + tw - 1) // tw
    tile_rows = (P.row1 - 1) // th - P.row0 // th + 1 if P.row1 > P.row0 else 0
    per_row = (tiles_x + world - 1) // world
    return tile_rows, per_row, tile_rows * per_row * tw * th * P.spp


def picks_owned(passes, total_slots, world, tile, sel, slot_begin, slot_end):
    """Must the launcher take k_generate_owned?"""
    space = sum((owned_space(P, tile, world)[2] + BLOCK - 1) // BLOCK * BLOCK for P in passes)
    return world > 1 and sel == 0 and slot_begin == 0 and slot_end == total_slots and space <= total_slots


def walk_owned(passes, rank, world, tile, mut=None):
    """The padded index space of a rank -> per entry that is a launch index of the job: (pass, lx, ly, s, slot, block iteration),
    as int64 arrays, in the order of the space."""
    tw, th = tile
    out = [[] for _ in range(6)]
    it0 = 0
    for p, P in enumerate(passes):
        tile_rows, per_row, count = owned_space(P, tile, world)
        v = np.arange(count, dtype=np.int64)
        t, s = v // P.spp, v % P.spp
        tl, inn = t // (tw * th), t % (tw * th)
        ty = P.row0 // th + tl // per_row
        rot = (ty if mut == "owner_ty_not_tripled" else 3 * ty) + (0 if mut == "owner_without_frame_pass" else P.frame_pass)
        first = (rank + world - rot % world) % world
        lx = (first + (tl % per_row) * world) * tw + inn % tw
        ly = ty * th + inn // tw
        ok = (lx < P.gw) & (ly >= P.row0) & (ly < P.row1)                   # the rest is padding
        slot = slot_of(P, lx, ly, s, relative=mut != "owned_slot_without_row0")
        for k, a in enumerate((np.full(count, p), lx, ly, s, slot, it0 + v // BLOCK)):
            out[k].append(a[ok])
        it0 += (count + BLOCK - 1) // BLOCK
    return [np.concatenate(a) if a else np.zeros(0, np.int64) for a in out]


def expected(passes, total_slots, total_records, alive, rank=0, world=1, tile=(8, 4), sel=0, slot_begin=0, slot_end=None, grid=8, mut=None):
    """alive: per pass the (launch indices,) bool array of the ring test, in launch-record order.
    -> dict(kernel, live (sorted slots), shard (total_slots,) int8, -1 for a slot that is not live, count (8,), cap,
    pass_of / li_of / sample_of (total_slots,): the (pass, launch index in record order, sample) of every slot,
    record_live (total_records,) bool: the records whose backplate is written, record_pass / record_li: whose they are)."""
    slot_end = total_slots if slot_end is None else slot_end
    first, mask = (4 if sel == 2 else 0), (SHARDS - 1 if sel == 0 else 3)
    pass_of, li_of, sample_of = (np.full(total_slots, -1, np.int64) for _ in range(3))
    live_general = np.zeros(total_slots, bool)
    for p, P in enumerate(passes):
        idx = launch_indices(P).astype(np.int64)
        n = idx.shape[0]
        li = np.repeat(np.arange(n), P.spp)
        s = np.tile(np.arange(P.spp), n)
        slot = slot_of(P, idx[li, 0], idx[li, 1], s)
        assert slot.min(initial=0) >= 0 and slot.max(initial=0) < total_slots and (pass_of[slot] < 0).all()
        pass_of[slot], li_of[slot], sample_of[slot] = p, li, s
        mine = owner(P, idx[:, 0], idx[:, 1], tile, world, mut) == rank if world > 1 else np.ones(n, bool)
        live_general[slot] = (np.asarray(alive[p], bool) & mine)[li] & (slot >= slot_begin) & (slot < slot_end)
    kernel = 1 if picks_owned(passes, total_slots, world, tile, sel, slot_begin, slot_end) else 0
    shard = np.full(total_slots, -1, np.int8)
    if kernel == 0:
        slot = np.flatnonzero(live_general)
        shard[slot] = first + (((slot - slot_begin) // BLOCK) % grid & mask)
    else:
        p_, lx, ly, s, slot, it = walk_owned(passes, rank, world, tile, mut)
        keep = np.zeros(slot.shape, bool)
        for p, P in enumerate(passes):                                      # ring test and ownership of the entries
            m = p_ == p
            rec = (ly[m] - P.row0) * P.gw + lx[m]
            keep[m] = np.asarray(alive[p], bool)[rec] & (owner(P, lx[m], ly[m], tile, world, mut) == rank)
        inside = (slot >= 0) & (slot < total_slots)
        assert mut is not None or inside.all()                              # (only a mutation can put one outside)
        keep &= inside
        slot, it = slot[keep], it[keep]
        shard[slot] = first + ((it % grid) & mask)
    live = np.flatnonzero(shard >= 0)
    record_live = np.zeros(total_records, bool)
    record_pass, record_li = np.full(total_records, -1, np.int64), np.full(total_records, -1, np.int64)
    for p, P in enumerate(passes):
        idx = launch_indices(P).astype(np.int64)
        last = slot_of(P, idx[:, 0], idx[:, 1], P.spp - 1)
        rec = record_of(P, idx[:, 0], idx[:, 1], mut)
        w = (shard[last] >= 0) & (rec < total_records)                      # (only a mutation can put one outside)
        record_live[rec[w]] = True
        record_pass[rec[w]], record_li[rec[w]] = p, np.flatnonzero(w)
    return dict(kernel=kernel, live=live, live_general=np.flatnonzero(live_general), shard=shard,
                count=np.bincount(shard[live].astype(np.int64), minlength=SHARDS).astype(np.uint32), cap=shard_capacity(total_slots),
                pass_of=pass_of, li_of=li_of, sample_of=sample_of, record_live=record_live, record_pass=record_pass, record_li=record_li)
