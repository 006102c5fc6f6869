"""The state of an animated application, restated: AppModel drives one SampleRenderer through updates of all four kinds, skin and
morph registration, frames (also several in flight), the post chain (fovpt_post, fovpt_expose, fovpt_packet_*), resizes, scene
reloads, resets and refused calls, keeps on the host everything the context is specified to keep (include/fovpt.h, DESIGN
sections 12 to 20) and checks after every operation what that operation defines.  It never reads state back from the library to
decide what to expect.  tests/app_fuzz.py writes the scripts run() takes; tests/test_app_fuzz_gpu.py runs them.

What it keeps: the rest positions (the renderer's Model, never changed), the current positions, the registered skins and morph
targets, MotionChecker's tracking bookkeeping (through PostChecker), the exposure state (test_expose_gpu.Checker), the frame
size, whether a frame has been rendered at this size, the updates counted since the scene was set, and the packets submitted.

The hierarchy is compared with a twin context built from the same model that is only ever given fovpt_update_vertices of the
model's positions for the meshes just moved, with a rebuild at the same moments.  The build hands out node slots with atomic
counters, so two builds of one model number their nodes differently, and now and then (one rebuild in a few hundred) they group
the primitives differently: same_tree() compares the records always and canonical() forms, the tree with its boxes, leaves and
records but without the numbering, where the two shapes agree.  Whatever the shape, every record and box must be a fixed point
of refit_ref over the model's positions, and the link words a refit must not touch are compared on the context itself.

LateModel, at the end of this file, is the model of the late scripts (app_fuzz.script(seed, late=True)): the rig, the focus state,
the record of the background build, what the last temporal step knew of its interval and the stamp of the last G-buffer trace.
HdrModel, behind it, is the model of the hdr scripts (app_fuzz.script(seed, hdr=True)): the moment history of fovpt_variance, the
size of the context's own variance image and the rendered frame's camera, for the four stages variance, variance filter, bloom and
quality inside the chain.

dry_run() is the part of the model that needs no renderer: the positions.  (oracle.OracleScene exposes trace() and no tree,
so there is no hierarchy for refit_ref to follow without a GPU.)"""
import hashlib

import numpy as np

import packet_ref as pk
import post_ref as po
import refit_ref as rf
import transform_ref as tf
from fovpathtracing_optixcodelatest_amd import abi, lib, renderer

from common import cfg_foveated, cfg_uniform, make_gpu
from post_common import PostChecker
from gpu_common import bits, camera, debug_buffer, device_filled, device_images, host_view
from temporal_motion_common import restate, vertex_arrays

F = np.float32
E_INVALID, E_NO_FRAME = -1, -5
SEQUENCE0 = 7000                                         # packet k carries sequence SEQUENCE0 + k


# ---- without a renderer ----------------------------------------------------------------------------------------------------
def config_of(s):
    """abi.Config of a script."""
    c = s["config"]
    p, m, f, u = c["spp"]
    cfg = cfg_uniform(u, c["max_depth"]) if c["uniform"] else cfg_foveated(c["r_inner"], c["r_outer"], (p, m, f), c["max_depth"])
    cfg.r_inner, cfg.r_outer = c["r_inner"], c["r_outer"]
    cfg.write_guides = 1
    cfg.frames_in_flight, cfg.chains_per_frame = c["frames_in_flight"], c["chains_per_frame"]
    return cfg


def updates_of(op):
    """The updates an operation issues, in order: (update operation, where: "alone", "between" or "pre_chain")."""
    if op["op"] == "update":
        return [(op, "alone")]
    if op["op"] == "frame":
        out = [(b, "between") for b in op["between"] if b is not None and b["op"] == "update"]
        return out + ([(op["pre_chain"], "pre_chain")] if op["pre_chain"] is not None else [])
    return []


def register(have, new):
    for k, v in new.items():
        if v is None:
            have.pop(k, None)
        else:
            have[k] = v


def dry_run(s, model, oracle=None):
    """The positions a script leaves, through the position restatements alone -> (V, 3) float32; every intermediate position
    array is checked to be finite.  oracle: for the scripts with a rig (rig_ref takes its sine and arc cosine from it)."""
    import rig_ref as rg
    _, vtx, _, first = vertex_arrays(model)
    vtx = vtx.copy()
    skins, morphs, rig = dict(s["skins"]), dict(s["morphs"]), s.get("rig")
    for op in s["ops"]:
        if op["op"] == "set_skins":
            register(skins, op["skins"])
            rig = None
        elif op["op"] == "set_morphs":
            register(morphs, op["morphs"])
            rig = None
        elif op["op"] == "set_rig":
            rig = op["rig"]
        elif op["op"] == "set_scene":
            skins, morphs, rig = {}, {}, None
            vtx = vertex_arrays(model)[1].copy()
        for u, _ in updates_of(op):
            if u["kind"] == "animated":
                new = rg.restate(oracle, model, rig, u["poses"]["clip"], u["poses"]["time"], skins, morphs)
            else:
                new = restate(model, u["kind"], u["poses"], skins, morphs)[1]
            for k, v in new.items():
                assert np.isfinite(v).all(), (s["seed"], u["kind"], k)
                vtx[first[k]:first[k + 1]] = v
    return vtx


# ---- the hierarchy without its numbering -----------------------------------------------------------------------------------
def canonical(nodes, tris, shape_only=False):
    """A digest of the wide tree that does not depend on how its nodes, child slots and records are numbered: an entry is its
    box and, for a leaf, the sorted records it holds, for a node, the sorted digests of the child's live entries.  shape_only:
    the grouping of the primitives alone, without boxes and vertices."""
    nodes = np.asarray(nodes, np.uint32).reshape(-1, 4, 8)
    ni, nf = nodes.view(np.int32), nodes.view(F)
    tris = np.asarray(tris, np.uint32).reshape(-1, 12)

    def node(i):
        out = []
        for k in range(4):
            if not nf[i, k, 0] < np.inf:
                continue
            code = int(ni[i, k, 6])
            if code < 0:
                t0, n = rf.leaf_range(code)
                body = b"".join(sorted(tris[t, 9:11].tobytes() if shape_only else tris[t].tobytes() for t in range(t0, t0 + n)))
            else:
                body = node(code)
            out.append(hashlib.sha1((b"" if shape_only else nodes[i, k, :6].tobytes()) + body).digest())
        return b"".join(sorted(out))
    return node(0)


def same_tree(a, b):
    """Two contexts' hierarchies of the same positions.  Always: the same triangle records, whatever their order.  Two builds
    of one scene usually choose the same tree and sometimes do not (the builder's parallel passes break ties by arrival), which
    nothing specifies; where they did, every entry's box is the same too.  -> whether the shapes agree."""
    (na, ta), (nb, tb) = a, b
    ra, rb = (np.asarray(t, np.uint32).reshape(-1, 12)[:, :11] for t in (ta, tb))
    assert ra.shape == rb.shape and np.array_equal(ra[np.lexsort(ra.T[::-1])], rb[np.lexsort(rb.T[::-1])]), "triangle records"
    if canonical(na, ta, shape_only=True) != canonical(nb, tb, shape_only=True):
        return False
    assert canonical(na, ta) == canonical(nb, tb), "hierarchy"
    return True


def links(nodes):
    """The words of the nodes a refit leaves alone: the code and rank of every child record."""
    return np.asarray(nodes, np.uint32).reshape(-1, 4, 8)[:, :, 6:8].copy()


def expected_cost(n):
    levels = rf.levels_of(n)
    return rf.sah_cost(n, levels), tf.cost_tolerance(tf.live_entries(n, levels))


def hierarchy(r):
    from test_refit_gpu import hierarchy as h
    return h(r)


# ---- the model ---------------------------------------------------------------------------------------------------------------
class AppModel(PostChecker):
    def __init__(self, oracle, s, model, cam, probe):
        """s: a script of app_fuzz (its scene already made: model, cam), or any dict with size, config, post, skins, morphs."""
        self.s, self.cam, self.probe, self.cfg_frame = s, dict(cam), probe, config_of(s)
        self.size = tuple(s["size"])
        r = make_gpu(model, probe, cam, self.size, self.cfg_frame)
        super().__init__(oracle, r, cfg=s["post"])
        self.twin = renderer.SampleRenderer(model)
        self.rest = self.vtx.copy()
        self.updates = 0                                  # fovpt_hierarchy_cost's counter
        self.rendered = False                             # a frame exists at this size
        self.packets = 0
        from test_expose_gpu import Checker as ExposeChecker
        self.ex = ExposeChecker(oracle, r)
        self._bufs = []
        self.log = []
        self.fb = self.zero_frame()                       # the context's own frame buffers: zero after a resize
        assert r.hierarchy_cost().updates == 0            # (switches the watching on)
        self.tree_agrees = same_tree(hierarchy(r), hierarchy(self.twin))
        self.log.append(("tree", self.tree_agrees))
        if s["skins"]:
            self.set_skins(s["skins"])
        if s["morphs"]:
            self.set_morphs(s["morphs"])

    def close(self):
        self.r.close()
        self.twin.close()

    def zero_frame(self):
        w, h = self.size
        return dict(frame=np.zeros((h, w), np.uint32), **{k: np.zeros((h, w, 4), F) for k in ("accum", "normal", "color", "albedo")})

    # ---- positions and the tree
    def current(self, meshes=None):
        """{mesh: its current positions} of the meshes named (default: all that differ from rest)."""
        if meshes is None:
            meshes = [k for k in range(len(self.first) - 1) if not np.array_equal(bits(self.vtx[self.first[k]:self.first[k + 1]]), bits(self.rest[self.first[k]:self.first[k + 1]]))]
        return {k: self.vtx[self.first[k]:self.first[k + 1]].copy() for k in meshes}

    def scene_vertices(self):
        p, n = debug_buffer(self.r, "scene_vertices")
        return self.r.download(p, np.empty((n // 12, 3), F))

    def check_scene(self, rebuilt=False, before=None, adopted=None):
        """After an update (and everything enqueued): positions, previous positions of the marked meshes, the tree against the
        twin's, the cost counters and the cost.  adopted: the positions a background build's snapshot held, where the tree is
        an adopted one that no synchronous rebuild has replaced since: `built` is the cost of the tree over those positions."""
        r = self.r
        # (the position buffer exists from a scene's first update on; before that, and so right after fovpt_set_scene, the
        # positions are held through the triangle records below, which must be refit_ref's of the model's positions)
        if self.updates:
            assert np.array_equal(bits(self.scene_vertices()), bits(self.vtx)), "scene_vertices"
        if self.tracking and self.moved.any():
            p, n = debug_buffer(r, "scene_vertices_prev")
            prev = r.download(p, np.empty((n // 12, 3), F))
            for k in np.flatnonzero(self.moved):
                a, b = self.first[k], self.first[k + 1]
                assert np.array_equal(bits(prev[a:b]), bits(self.vtx_step[a:b])), "previous positions of mesh %d" % k
        n, t = hierarchy(r)
        agrees = same_tree((n, t), hierarchy(self.twin))
        if not rebuilt:                                       # a refit changes no shape: what agreed before still does
            assert agrees == self.tree_agrees, "the shapes of the two trees %s after a refit" % ("differ" if self.tree_agrees else "agree")
        self.tree_agrees = agrees
        self.log.append(("tree", agrees))
        levels = rf.levels_of(n)
        wn, wt = rf.refit(n, t, levels, self.tri_vidx, self.vtx)          # every record and box is the restatement's of the
        assert np.array_equal(wt, t), "records against refit_ref"         # model's positions: refitting changes nothing
        assert np.array_equal(wn, n), "boxes against refit_ref"
        if rebuilt:
            rf.check_conservative(n, t, levels)
        elif before is not None:
            assert np.array_equal(links(n), before), "a refit changed the tree's links"
        c = r.hierarchy_cost(wait=True)
        assert (c.updates, c.measured) == (self.updates, self.updates), (c.updates, c.measured, self.updates)
        want, tol = expected_cost(n)
        assert abs(c.current - want) <= tol * want, (c.current, want)
        if adopted is not None:
            sn, _ = rf.refit(n, t, levels, self.tri_vidx, adopted)
            want, tol = expected_cost(sn)
            assert abs(c.built - want) <= tol * want, ("built of an adopted tree", c.built, want)
        elif rebuilt or self.updates == 0:
            assert c.built == c.current

    def update(self, poses, rebuild=False, device=False, kind="vertices", check=True):
        before = links(hierarchy(self.r)[0]) if check and not rebuild else None
        super().update(poses, rebuild=rebuild, device=device, kind=kind)
        self.twin.update_vertices(self.current(sorted(poses)), rebuild=rebuild)
        if poses or rebuild:
            self.updates += 1
        if check:
            self.check_scene(rebuild, before)

    def refused(self, op, check=True):
        r = self.r
        if op["which"] == "no_frame":                         # straight after a resize: nothing of the chain has a frame to work on
            assert not self.rendered
            for call in op["calls"]:
                with_pytest_code(op["code"], dict(post=r.post, expose=r.expose, packet=lambda: r.submitPacket(1))[call])
            return
        with_pytest_code(op["code"], lambda: self.refused_call(op))
        if check:
            self.check_scene()

    def refused_call(self, op):
        r = self.r
        give = restate_refused(r.model, op, self.skins, self.morphs)
        getattr(r, dict(vertices="update_vertices", transforms="update_transforms", skinned="update_skinned", morphed="update_morphed")[op["kind"]])(give)

    # ---- registration
    def set_skins(self, new):
        self.r.set_skins(new)
        register(self.skins, new)
        if self.updates:
            assert np.array_equal(bits(self.scene_vertices()), bits(self.vtx)), "set_skins moved geometry"

    def set_morphs(self, new):
        self.r.set_morphs(new)
        register(self.morphs, new)
        if self.updates:
            assert np.array_equal(bits(self.scene_vertices()), bits(self.vtx)), "set_morphs moved geometry"

    # ---- frames
    def view(self, v):
        r, (w, h) = self.r, self.size
        eye = tuple(float(x) for x in (np.array(self.cam["eye"], np.float64) * (1.0 + np.array(v["eye"]))).astype(F))
        cam = dict(self.cam, eye=eye)
        r.setCamera(renderer.Camera(cam["eye"], cam["lookat"], cam["up"], cam["fovy"], w / float(h)))
        f = r.launchParams.frame
        f.c.x, f.c.y = v["gaze"][0] & 0xffffffff, v["gaze"][1] & 0xffffffff
        f.subframe_index = v["subframe_index"]
        return cam

    def frames(self, op):
        """The frames of one group, each compared with the oracle's frame of the positions at issue time."""
        import torch
        from test_refit_gpu import moved
        r, (w, h) = self.r, self.size
        f = r.launchParams.frame
        n = len(op["views"])
        r.synchronize()
        r.reset_stats()
        issued = []
        for k, v in enumerate(op["views"]):
            cam = self.view(v)
            if n > 1:
                b = (torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), torch.zeros((h, w), dtype=torch.int32, device="cuda"))
                torch.cuda.synchronize()
                f.accum_buffer, f.frame_buffer = b[0].data_ptr(), b[1].data_ptr()
            else:
                b = None
                f.accum_buffer, f.frame_buffer = r._frame_ptrs.accum_buffer, r._frame_ptrs.frame_buffer
            if op["sync"]:
                r.render()
            else:
                r.render_async()
            issued.append((cam, (f.c.x, f.c.y), v["subframe_index"], self.current(), b))
            if k + 1 < n and op["between"][k] is not None:
                u = op["between"][k]
                if u["op"] == "update":
                    self.update(u["poses"], u["rebuild"], u["device"], u["kind"], check=False)
                else:
                    self.refused(u, check=False)
        r.synchronize()
        self._bufs = [x[4] for x in issued]
        paths = rad = shadow = 0
        for k, (cam, gaze, sub, pos, b) in enumerate(issued):
            # the buffers a frame is resolved into keep what no pass of it writes: the context's own from the frames before
            # (zero after a resize), a caller's buffers here zero; the guides are always the context's own
            S = self.oracle.OracleScene(moved(r.model, pos))
            Fr = self.oracle.OracleFrame(w, h, self.oracle.HostProbe(self.probe), cam, gaze=gaze, subframe_index=sub)
            for name in ("normal", "color", "albedo") + (("accum", "frame") if b is None else ()):
                getattr(Fr, name)[...] = self.fb[name]
            cnt = self.oracle.render(S, Fr, self.cfg_frame, nthreads=16)
            for name in ("normal", "color", "albedo") + (("accum", "frame") if b is None else ()):
                self.fb[name] = getattr(Fr, name).copy()
            acc = r.downloadAccum() if b is None else b[0].cpu().numpy()
            px = r.downloadPixels() if b is None else b[1].cpu().numpy().view(np.uint32)
            assert np.array_equal(bits(acc), bits(Fr.accum)), "frame %d of %d: accum, %d pixels" % (k, n, (bits(acc) != bits(Fr.accum)).any(axis=-1).sum())
            assert np.array_equal(px, Fr.frame), "frame %d of %d: rgba8" % (k, n)
            paths, rad, shadow = paths + cnt[2], rad + cnt.lib_radiance, shadow + cnt.lib_shadow
        st = r.stats()
        assert (st.paths, st.radiance_rays, st.shadow_rays) == (paths, rad, shadow), ((st.paths, st.radiance_rays, st.shadow_rays), (paths, rad, shadow))
        for name in ("normal", "albedo", "color"):            # the guides after the last frame issued
            g = r.download(getattr(f, name + "_buffer"), np.empty((h, w, 4), F))
            assert np.array_equal(bits(g), bits(self.fb[name])), name
        self.rendered = True
        self.last_rgba = px
        self.frame_as_rendered = ((w, h), issued[-1][1], (self.cfg_frame.r_inner, self.cfg_frame.r_outer), bool(self.cfg_frame.uniform))
        self.gaze_rendered = issued[-1][1]
        if any(b is not None and b["op"] == "update" for b in op["between"]):
            self.check_scene(rebuilt=any(b is not None and b["op"] == "update" and b["rebuild"] for b in op["between"]))                               # what the updates between the frames left, now that all has run

    def chain(self, c, moved_on=None):
        """The post chain of the frame rendered last.  moved_on: the caller's next gaze and subframe index, written into the
        launch parameters first: every stage works on the frame as it was rendered all the same."""
        r = self.r
        if moved_on is not None:
            f = r.launchParams.frame
            f.c.x, f.c.y = moved_on["gaze"][0] & 0xffffffff, moved_on["gaze"][1] & 0xffffffff
            f.subframe_index = moved_on["subframe_index"]
        color = ptr = None                                    # the colour the next stage is given: numpy, device pointer
        rgba, rgba_ptr = self.last_rgba, None if not self._bufs or self._bufs[-1] is None else self._bufs[-1][1].data_ptr()
        if c["post"] is not None:
            had = self.prev is not None
            out = self.step(stages=c["post"])
            color, ptr = out["color"], r.post_buffers()[0]
            rgba, rgba_ptr = r.downloadPostPixels(), r.post_buffers()[1]
            self.log.append(("post", c["post"], had))
        if c["expose"] is not None:
            before = dict(self.ex.state)
            out = self.expose(c["expose"], r.downloadAccum() if color is None else color, ptr)
            rgba, rgba_ptr = out["rgba"], r.expose_buffers()[1]
            self.log.append(("expose", before["steps"], self.ex.state["steps"]))
        if c["packet"]:
            self.packet(rgba, rgba_ptr)

    def expose(self, d, inp, in_ptr):
        """test_expose_gpu.Checker.step with the frame as rendered where that reads the launch parameters."""
        import expose_ref as ex
        import reconstruct_ref as rr
        from test_expose_gpu import ecfg, histogram, same_state, usable
        r, ck = self.r, self.ex
        c, full = ecfg(d)
        r.expose(c, in_ptr)
        got_c, got_px = r.downloadExposedColor(), r.downloadExposedPixels()
        (w, h), gaze, (ri, ro), uniform = self.frame_as_rendered
        fill, uni = (rr.writers(w, h, gaze, ri, ro, int(uniform))[0], int(uniform)) if full["metering"] == ex.GAZE and full["mode"] == ex.AUTO else (None, 0)
        want_c, want_px, want_h, ck.state = ex.expose(self.oracle, inp, full, ck.state, fill, uni)
        if want_h is not None:
            assert np.array_equal(histogram(r), want_h), "expose: histogram"
        if ck.state["steps"]:
            same_state(r.expose_state(), ck.state, "expose")
        ok = usable(inp)
        assert np.array_equal(bits(got_c[ok]), bits(want_c[ok])), "expose: colour"
        assert np.array_equal(got_px[ok], want_px[ok]), "expose: rgba8"
        return dict(color=got_c, rgba=got_px)

    def packet(self, rgba, rgba_ptr):
        import torch
        from packet_cases import junk_canvas
        from test_packet_gpu import decode_on_device, host_decode
        r, seq = self.r, SEQUENCE0 + self.packets
        want = pk.encode(rgba, *self.frame_as_rendered, sequence=seq)
        if not pk.check(want):                                # (a pass without a launch index: a frame side below 4, say)
            with_pytest_code(E_INVALID, lambda: r.submitPacket(seq, rgba_ptr))
            self.log.append(("packet", None))
            return
        slot = r.submitPacket(seq, rgba_ptr)
        assert slot == self.packets % abi.PACKET_SLOTS       # slots in submit order, over resizes and scene reloads too
        self.packets += 1
        got = r.waitPacket(slot)
        assert got == want, "packet %d" % seq
        self.log.append(("packet", slot))
        h = abi.PacketHeader.from_packet(got)
        dev = torch.frombuffer(bytearray(got), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        for mode in (abi.PACKET_NEAREST, abi.PACKET_SMOOTH):
            ref = pk.decode(got, mode, junk_canvas(self.size))
            assert np.array_equal(decode_on_device(r, dev, h, mode), ref), mode
            assert np.array_equal(host_decode(got, mode, self.size), ref), mode

    # ---- context events
    def resize(self, size):
        r = self.r
        state = bytes(r.expose_state())
        r.resize(size)
        self.size = tuple(size)
        self.rendered, self.prev = False, None               # the frame as rendered and the temporal history go
        self._bufs = []
        self.fb = self.zero_frame()
        f = r.launchParams.frame
        w, h = self.size
        assert not r.download(f.frame_buffer, np.empty((h, w), np.uint32)).any()
        for name in ("accum", "normal", "color", "albedo"):
            assert not r.download(getattr(f, name + "_buffer"), np.empty((h, w, 4), F)).view(np.uint32).any(), name
        if self.updates:                                      # positions stay (skins, morphs and tracking: the next pose and step show)
            assert np.array_equal(bits(self.scene_vertices()), bits(self.vtx))
        assert bytes(r.expose_state()) == state              # the exposure state stays
        if self.ex.state["steps"]:
            from test_expose_gpu import same_state
            same_state(r.expose_state(), self.ex.state, "after a resize")

    def set_scene(self):
        from test_temporal_gpu import _scene_again
        r = self.r
        _scene_again(r)
        _scene_again(self.twin)
        self.vtx, self.vtx_step = self.rest.copy(), self.rest.copy()
        self.moved[:] = False
        self.prev, self.tracking, self.untracked = None, False, False
        self.skins.clear()
        self.morphs.clear()
        self.updates = 0
        self.ex.reset()
        for call in (lambda: r.update_skinned({0: np.stack([tf.IDENTITY])}), lambda: r.update_morphed({0: np.zeros(1, F)})):
            with_pytest_code(E_INVALID, call)                 # refused until a skin or morph is set again
        with_pytest_code(E_INVALID, lambda: debug_buffer(r, "scene_vertices_prev"))     # tracking is off: its buffers are gone
        assert r.expose_state().steps == 0                    # a fresh exposure state
        c = r.hierarchy_cost()
        assert (c.updates, c.measured) == (0, 0) and c.built == c.current
        self.check_scene(rebuilt=True)                        # the tree is the twin's, of the rest positions

    # ---- a script
    def run_op(self, op):
        kind = op["op"]
        if kind == "update":
            self.update(op["poses"], op["rebuild"], op["device"], op["kind"])
        elif kind == "set_skins":
            self.set_skins(op["skins"])
        elif kind == "set_morphs":
            self.set_morphs(op["morphs"])
        elif kind == "frame":
            self.frames(op)
            if op["pre_chain"] is not None:
                u = op["pre_chain"]
                self.update(u["poses"], u["rebuild"], u["device"], u["kind"])
            self.chain(op["chain"], op.get("moved_on"))
        elif kind == "resize":
            self.resize(op["size"])
        elif kind == "set_scene":
            self.set_scene()
        elif kind == "temporal_reset":
            self.r.temporal_reset()
            self.reset()
        elif kind == "expose_reset":
            self.r.expose_reset()
            self.ex.reset()
        else:
            assert kind == "refused", kind
            self.refused(op)

    def run(self):
        for k, op in enumerate(self.s["ops"]):
            try:
                self.run_op(op)
            except Exception as e:
                raise AssertionError("seed %s, operation %d (%s): %s: %s" % (self.s.get("seed"), k, op["op"], type(e).__name__, e)) from e


def restate_refused(model, op, skins, morphs):
    """What a refused update is given: the poses as drawn, those of meshes that do not exist or have no skin included."""
    ok = {k: v for k, v in op["poses"].items() if 0 <= k < len(model.meshes) and (op["kind"] != "skinned" or k in skins)}
    give, _ = restate(model, op["kind"], ok, skins, morphs)
    for k, v in op["poses"].items():
        if k not in ok:
            give[k] = v
    return give


def with_pytest_code(code, call):
    """call() raises lib.FovptError with that code."""
    try:
        call()
    except lib.FovptError as e:
        assert e.code == code, (e.code, code, str(e))
        return
    raise AssertionError("a call that must be refused with %d was accepted" % code)


# ---- the late family's model ---------------------------------------------------------------------------------------------------
T_ = po.TEMPORAL
IDLE, BUILDING, READY = abi.REBUILD_IDLE, abi.REBUILD_BUILDING, abi.REBUILD_READY
DELAY = "FOVPT_ASYNC_BUILD_DELAY_MS"
RAW, BC1, BY_FILL = abi.PACKET_RAW, abi.PACKET_BC1, abi.PACKET_BY_FILL


class _Ptr:
    """A device address where a helper asks for a tensor's data_ptr()."""

    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


class LateModel(AppModel):
    """AppModel for the scripts of app_fuzz.script(seed, late=True).  On top of AppModel it keeps: the rig (present or dropped:
    fovpt_set_skins, fovpt_set_morphs and fovpt_set_scene drop it); the focus state (test_focus_gpu.Checker's, survives a resize,
    reset by fovpt_focus_reset and fovpt_set_scene); the record of the background build (in flight or not, known to be READY after
    a wait, the five counters, snapshot_update, the positions at the snapshot); what the last temporal step knew of its interval
    (warp_motion_common.Intervals' `last`); and whether the context's last G-buffer trace is newer than every render, update,
    resize, scene and adoption (the stamp fovpt_warp_motion checks for a caller's G-buffer).

    Background builds stay deterministic.  No pixel depends on which conservative tree is in use, so frames, G-buffers and stages
    are compared as ever.  An update that enqueues something while a build is in flight adopts the result if the state is READY:
    after rebuild_state(WAIT) that is certain and expected; without it the model reads fovpt_rebuild_state(0).adopted once after
    the call, accepts exactly "not adopted" and "adopted by one", goes on with what happened and logs it ("race")."""

    def __init__(self, oracle, s, model, cam, probe):
        from test_focus_gpu import Checker as FocusChecker
        self.rig = None
        self.rec = dict(flight=False, ready=False, requested=0, started=0, adopted=0, discarded=0, snapshot_update=0, snapshot=None)
        self._pending = None                              # what the updates issued without a check (between frames) did to the tree
        self.last = None
        self.trace_fresh = False
        self._late_keep = []
        super().__init__(oracle, s, model, cam, probe)
        self.fc = FocusChecker(oracle, self.r)
        if s.get("rig") is not None:
            self.set_rig(s["rig"])

    def split(self, vtx):
        return {k: vtx[self.first[k]:self.first[k + 1]].copy() for k in range(len(self.first) - 1)}

    # ---- the background build
    def check_info(self):
        rec, info = self.rec, self.r.rebuild_state()
        got = (info.requested, info.started, info.adopted, info.failed, info.discarded)
        assert got == (rec["requested"], rec["started"], rec["adopted"], 0, rec["discarded"]), (got, rec["requested"], rec["started"], rec["adopted"], rec["discarded"])
        assert info.last_error == 0
        if rec["flight"]:
            assert info.state in ((READY,) if rec["ready"] else (BUILDING, READY)), info.state
            assert info.snapshot_update == rec["snapshot_update"], (info.snapshot_update, rec["snapshot_update"])
        else:
            assert info.state == IDLE, info.state

    def adopt(self):
        """The bookkeeping of an adoption -> the snapshot's positions.  The twin is brought to the same tree: a rebuild over the
        snapshot, a refit over the present positions (the caller does both once the call's own update is in self.vtx)."""
        rec = self.rec
        snap = rec["snapshot"]
        rec.update(flight=False, ready=False, snapshot=None)
        rec["adopted"] += 1
        self.updates += 1
        self.trace_fresh = False                          # a caller's G-buffer no longer goes with the hit records
        return snap

    def twin_adopts(self, snap):
        self.twin.update_vertices(self.split(snap), rebuild=True)
        self.twin.update_vertices(self.split(self.vtx))

    def rebuild_state(self, wait, adopt):
        rec = self.rec
        info = self.r.rebuild_state(wait=wait, adopt=adopt)
        took = False
        if rec["flight"]:
            rec["ready"] = rec["ready"] or wait
            if adopt and rec["ready"]:
                took = True
            elif adopt:
                assert info.adopted in (rec["adopted"], rec["adopted"] + 1), info.adopted
                took = info.adopted == rec["adopted"] + 1
                self.log.append(("race", "rebuild_state", took))
        if took:
            at, now = rec["snapshot_update"], self.updates
            snap = self.adopt()
            self.twin_adopts(snap)
            self.check_scene(True, None, snap)
            self.log.append(("adopt", "rebuild_state", at, now, self.tree_agrees))
        self.check_info()

    def check_scene(self, rebuilt=False, before=None, adopted=None):
        # AppModel.frames() ends with check_scene(rebuilt=any(b["rebuild"] ...)), which is true for "async" as well and knows
        # nothing of adoptions.  What the updates between the frames really did to the tree is in _pending (update(check=False)
        # fills it), and it replaces the arguments on purpose: keep this where frames() or its argument changes.
        if self._pending is not None:
            rebuilt, before, adopted = self._pending["shape"], None, self._pending["adopted"]
            self._pending = None
        super().check_scene(rebuilt, before, adopted)

    # ---- updates
    def update(self, poses, rebuild=False, device=False, kind="vertices", check=True):
        import rig_ref as rg
        from temporal_motion_common import MotionChecker
        r, rec = self.r, self.rec
        sync, asyn, animated = rebuild is True, rebuild == "async", kind == "animated"
        moves = animated or bool(poses)
        before = links(hierarchy(r)[0]) if check and not sync else None
        if sync and rec["flight"]:                            # a synchronous rebuild ends the build
            rec.update(flight=False, ready=False, snapshot=None)
            rec["discarded"] += 1
        idle = not rec["flight"]                              # when the call comes in: what a request looks at
        may_adopt = moves and not sync and rec["flight"]
        certain = may_adopt and rec["ready"]
        if animated:
            new = rg.restate(self.oracle, r.model, self.rig, poses["clip"], poses["time"], self.skins, self.morphs)
            r.update_animated(poses["clip"], poses["time"], rebuild=rebuild)
            for k, v in new.items():
                self.vtx[self.first[k]:self.first[k + 1]] = v
                self.moved[k] = True                          # one update for the tracking
            self.untracked = self.untracked or (bool(new) and not self.tracking)
            meshes = sorted(new)
        else:
            MotionChecker.update(self, poses, rebuild=rebuild, device=device, kind=kind)
            meshes = sorted(poses)
        snap = None
        if may_adopt:
            took = certain
            if not certain:
                n = r.rebuild_state().adopted
                assert n in (rec["adopted"], rec["adopted"] + 1), n
                took = n == rec["adopted"] + 1
                self.log.append(("race", "update", took))
            if took:
                at, now = rec["snapshot_update"], self.updates
                snap = self.adopt()                           # (counts one, before the call's own update)
        if moves or sync:
            self.updates += 1
        if moves:
            self.trace_fresh = False
        if asyn:
            rec["requested"] += 1
            if idle:                                          # (a call that adopts counts its own request and starts nothing)
                rec.update(flight=True, ready=False, snapshot_update=self.updates, snapshot=self.vtx.copy())
                rec["started"] += 1
        if snap is not None:
            self.twin_adopts(snap)
        else:
            self.twin.update_vertices(self.current(meshes), rebuild=sync)
        if check:
            self.check_scene(sync or snap is not None, before if snap is None else None, snap)
        else:
            p = self._pending = self._pending or dict(shape=False, adopted=None)
            if sync or snap is not None:
                p.update(shape=True, adopted=snap)
        if snap is not None:
            self.log.append(("adopt", "update", at, now, self.tree_agrees if check else None))

    def refused(self, op, check=True):
        import ctypes as C
        r, which = self.r, op["which"]
        if which in ("no_rig", "clip_range"):
            assert (self.rig is None) == (which == "no_rig")
            with_pytest_code(op["code"], lambda: r.update_animated(op["clip"], op["time"]))
        elif which == "async_with_rebuild":
            both = abi.UPDATE_REBUILD | abi.UPDATE_REBUILD_ASYNC
            if op["kind"] == "animated":
                with_pytest_code(op["code"], lambda: r._check(r._L.fovpt_update_animated(r._ctx, op["clip"], C.c_float(op["time"]), both)))
            else:
                with_pytest_code(op["code"], lambda: r._check(r._L.fovpt_update_vertices(r._ctx, None, 0, both)))
        elif which == "warp_motion_stale":
            assert self.prev is not None and self.tracking and self.moved.any() and self.rendered      # an update since the step
            to = self.to_camera(op["to"])[0]
            with_pytest_code(op["code"], lambda: r.warp_motion(to))
            return
        else:
            return super().refused(op, check)
        if check:
            self.check_scene()

    # ---- registration
    def set_skins(self, new):
        super().set_skins(new)
        self.rig = None

    def set_morphs(self, new):
        super().set_morphs(new)
        self.rig = None

    def set_rig(self, rig):
        before = self.r.hierarchy_cost().updates
        self.r.set_rig(rig)
        self.rig = rig
        assert self.r.hierarchy_cost().updates == before == self.updates      # a rig is no update
        if self.updates:
            assert np.array_equal(bits(self.scene_vertices()), bits(self.vtx)), "set_rig moved geometry"

    # ---- context events
    def resize(self, size):
        from test_focus_gpu import state_tuple
        super().resize(size)
        self.last, self.trace_fresh, self._late_keep = None, False, []
        if self.fc.state["steps"]:                            # the focus state stays
            assert state_tuple(self.r.focus_state()) == state_tuple(self.fc.state), "focus state after a resize"

    def set_scene(self):
        rec = self.rec
        if rec["flight"]:                                     # the scene ends the build
            rec.update(flight=False, ready=False, snapshot=None)
            rec["discarded"] += 1
        self.rig, self.last, self.trace_fresh = None, None, False
        self.fc.reset()
        super().set_scene()
        with_pytest_code(E_INVALID, lambda: self.r.update_animated(0, 0.5))        # the rig went with the scene
        assert self.r.focus_state().steps == 0

    # ---- the chain
    def to_camera(self, to):
        from test_warp_gpu import to_camera
        return to_camera((to[1], to[2]), self.size, base=self.cam)

    def step(self, inp=None, in_ptr=None, out=None, with_motion=True, stages=None):
        st = self.stages if stages is None else stages
        m, untracked = self.motion(), self.untracked
        m = dict(m, vtx_prev=m["vtx_prev"].copy(), vtx=m["vtx"].copy())
        res = super().step(inp, in_ptr, out, with_motion, stages)
        if st & T_:
            self.last = None if untracked else m              # what the step knew of the interval it ended
        self.trace_fresh = True
        return res

    def focus(self, d, color, ptr):
        """test_focus_gpu.Checker.step with the frame as rendered where that reads the launch parameters."""
        import focus_ref as fr
        from test_focus_gpu import fcfg, state_tuple
        r = self.r
        cfg, full = fcfg({k: v for k, v in d.items() if k != "gbuffer"})
        g = r.temporal_gbuffer() if d["gbuffer"] == "temporal" else None
        inp = r.downloadAccum() if color is None else color
        oc, op, oz = device_images(self.size, 16, 4, 4)
        r.focus(cfg, g, ptr, oc.data_ptr(), op.data_ptr(), oz.data_ptr())
        gb = r.downloadGBuffer()                              # (the same rays as the call's own trace, and as the step's)
        self.trace_fresh = True
        steps = self.fc.state["steps"]
        want = fr.focus(self.oracle, gb, self.frame_as_rendered[1], inp, full, self.fc.state)
        self.fc.state = want["state"]
        if self.fc.state["steps"]:
            got = r.focus_state()
            assert state_tuple(got) == state_tuple(self.fc.state), ("focus: state", state_tuple(got), state_tuple(self.fc.state))
        assert np.array_equal(bits(host_view(oz, "coc")), bits(want["coc"])), "focus: radius"
        assert np.array_equal(bits(host_view(oc, "color")), bits(want["color"])), "focus: colour"
        assert np.array_equal(host_view(op, "rgba"), want["rgba"]), "focus: rgba8"
        self.log.append(("focus", full["mode"], int(want["state"]["count"]) if full["mode"] == abi.FOCUS_AUTO else None, int(want["acted"].sum()), steps))
        self._late_keep += [oc, op, oz]
        return want["color"], oc.data_ptr(), want["rgba"], op.data_ptr()

    def warp(self, la, color, ptr, rgba, rgba_ptr):
        """fovpt_warp through test_warp_gpu.check; fovpt_warp_motion as warp_motion_common.check does it, with the chain's images
        as the inputs and `last` from the model's own steps."""
        import warp_motion_ref as wm
        import warp_ref as wr
        from test_warp_gpu import check as warp_check, counts_of
        from warp_motion_common import frame_data, mcfg
        r = self.r
        to, want_cam = self.to_camera(la["to"])
        inp = r.downloadAccum() if color is None else color
        images, radius = la["images"], la["fill_radius"]
        if la["stage"] == "warp":
            gb = r.downloadGBuffer()
            self.trace_fresh = True
            warp_check(r, to, want_cam, gb, inp, rgba, radius, images, (ptr, rgba_ptr), None, "warp")
            self.log.append(("warp",))
            return
        cfg = mcfg(images=images, fill_radius=radius, advance=la["advance"])
        g = r.temporal_gbuffer() if la["gbuffer"] == "temporal" else None
        if la["adopt"]:                                       # an adoption between the step's trace and the warp
            assert self.rec["flight"] and g is not None
            self.rebuild_state(True, True)
            assert not self.trace_fresh
            with_pytest_code(E_NO_FRAME, lambda: r.warp_motion(to, cfg, g, ptr, rgba_ptr))
            self.log.append(("stale", "refused"))
            frame_data(r)                                     # a fresh trace: the caller's set goes with the hit records again
            self.trace_fresh = True
        assert self.prev is not None and self.tracking and not self.moved.any()     # legal: a step, tracking, no update since
        assert g is None or self.trace_fresh                  # ... and with a caller's G-buffer, a trace newer than everything else
        oc, op, om = device_images(self.size, 16, 4, 4)
        r.warp_motion(to, cfg, g, ptr, rgba_ptr, oc.data_ptr(), op.data_ptr(), om.data_ptr())
        got_counts = counts_of(r)
        gb, uv = frame_data(r)                                # (the same rays as the trace the call used, or made)
        self.trace_fresh = True
        d = dict(images=images, fill_radius=radius, advance=la["advance"])
        want = wm.warp(gb, uv, self.last, camera(r), want_cam, d, inp, rgba)
        plain = wr.warp(gb, camera(r), want_cam, dict(images=images, fill_radius=radius), inp, rgba)
        assert np.array_equal(host_view(om, "map"), want["map"]), "warp_motion: map"
        assert got_counts == want["counts"] and sum(got_counts[1:]) == self.size[0] * self.size[1], (got_counts, want["counts"])
        differs = not np.array_equal(want["map"], plain["map"])
        if images & wr.COLOR:
            assert np.array_equal(bits(host_view(oc, "color")), bits(want["color"])), "warp_motion: colour"
            differs = differs or not np.array_equal(bits(want["color"]), bits(plain["color"]))
        else:
            assert (oc.cpu().numpy() == 0x5a).all()
        if images & wr.RGBA:
            assert np.array_equal(host_view(op, "rgba"), want["rgba"]), "warp_motion: rgba8"
            differs = differs or not np.array_equal(want["rgba"], plain["rgba"])
        else:
            assert (op.cpu().numpy() == 0x5a).all()
        moving = self.last is not None and bool(self.last["moved"].any()) and la["advance"] > 0
        if not moving:                                        # nothing known to move: fovpt_warp's bits
            assert not differs, "warp_motion without motion is not fovpt_warp"
        self.log.append(("warp_motion", moving, differs, self.last is None))
        if la["adopt"]:
            self.log.append(("stale", "accepted"))

    def lens(self, la, color, ptr):
        from test_lens_gpu import lcfg, run
        r = self.r
        inp = r.downloadAccum() if color is None else color
        cfg, full = lcfg(self.size, filter=la["filter"], chroma=la["chroma"])
        want = run(r, self.oracle, inp, _Ptr(ptr), cfg, full, self.to_camera(la["to"]) if la["to"] is not None else None, "lens")
        self.log.append(("lens", not np.array_equal(bits(want["color"]), bits(inp))))

    def packet(self, rgba, rgba_ptr, codec=None):
        import torch
        import packet_bc_ref as bc
        from packet_cases import junk_canvas
        from test_packet_gpu import decode_on_device
        if codec is None:
            return super().packet(rgba, rgba_ptr)
        r, seq = self.r, SEQUENCE0 + self.packets
        pas = pk.passes(*self.frame_as_rendered)
        give = tuple(k if p < len(pas) or k == BY_FILL else RAW for p, k in enumerate(codec))      # nothing beyond the frame's passes
        if not pk.check(pk.encode(rgba, *self.frame_as_rendered, sequence=seq)):    # as the raw packet: a pass without a launch index
            with_pytest_code(E_INVALID, lambda: r.submitPacket(seq, rgba_ptr, codec=give))
            self.log.append(("coded", None, 0))
            return
        resolved = tuple((BC1 if pas[p][3] > 1 else RAW) if codec[p] == BY_FILL else codec[p] for p in range(len(pas)))
        want = bc.encode(rgba, *self.frame_as_rendered, resolved, sequence=seq)
        slot = r.submitPacket(seq, rgba_ptr, codec=give)
        assert slot == self.packets % abi.PACKET_SLOTS
        self.packets += 1
        got = r.waitPacket(slot)
        assert got == want, "coded packet %d" % seq
        hd = bc.parse(got)
        two = 0
        for (gw, gh, *_, off), k in zip(hd["passes"], hd["codecs"]):
            if k == BC1:
                w = np.frombuffer(got, "<u4", 2 * ((gw + 3) // 4) * ((gh + 3) // 4), off).reshape(-1, 2)
                two += int(((w[:, 0] & 0xffff) != (w[:, 0] >> 16)).sum())
        self.log.append(("coded", resolved, two))
        h = abi.PacketHeader.from_packet(got)
        dev = torch.frombuffer(bytearray(got), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        for mode in (abi.PACKET_NEAREST, abi.PACKET_SMOOTH):
            ref = bc.decode(got, mode, junk_canvas(self.size))
            assert np.array_equal(decode_on_device(r, dev, h, mode), ref), mode
            assert np.array_equal(renderer.decode_packet(got, mode, self.size, out=junk_canvas(self.size)), ref), mode

    def chain(self, c, moved_on=None):
        """post -> focus -> expose -> packet (of the unwarped frame) -> warp | warp_motion | lens."""
        if "focus" not in c:
            return super().chain(c, moved_on)
        r = self.r
        if moved_on is not None:
            f = r.launchParams.frame
            f.c.x, f.c.y = moved_on["gaze"][0] & 0xffffffff, moved_on["gaze"][1] & 0xffffffff
            f.subframe_index = moved_on["subframe_index"]
        color = ptr = None
        rgba, rgba_ptr = self.last_rgba, None if not self._bufs or self._bufs[-1] is None else self._bufs[-1][1].data_ptr()
        if c["post"] is not None:
            had = self.prev is not None
            out = self.step(stages=c["post"])
            color, ptr = out["color"], r.post_buffers()[0]
            rgba, rgba_ptr = r.downloadPostPixels(), r.post_buffers()[1]
            self.log.append(("post", c["post"], had))
        if c["focus"] is not None:
            color, ptr, rgba, rgba_ptr = self.focus(c["focus"], color, ptr)
        if c["expose"] is not None:
            out = self.expose(c["expose"], r.downloadAccum() if color is None else color, ptr)
            color, ptr = out["color"], r.expose_buffers()[0]
            rgba, rgba_ptr = out["rgba"], r.expose_buffers()[1]
        if c["packet"]:
            self.packet(rgba, rgba_ptr, c["codec"])
        la = c["last"]
        if la is not None and la["stage"] == "lens":
            self.lens(la, color, ptr)
        elif la is not None:
            self.warp(la, color, ptr, rgba, rgba_ptr)

    # ---- a script
    def run_op(self, op):
        kind = op["op"]
        if kind == "frame":
            self.frames(op)
            self.trace_fresh, self._late_keep = False, []
            if op.get("adopt_first"):
                self.rebuild_state(True, True)
            if op["pre_chain"] is not None:
                u = op["pre_chain"]
                self.update(u["poses"], u["rebuild"], u["device"], u["kind"])
            self.chain(op["chain"], op.get("moved_on"))
        elif kind == "set_rig":
            self.set_rig(op["rig"])
        elif kind == "rebuild_state":
            self.rebuild_state(op["wait"], op["adopt"])
        elif kind == "focus_reset":
            self.r.focus_reset()
            self.fc.reset()
        else:
            super().run_op(op)
        self.check_info()

    def run(self):
        import os
        had = os.environ.get(DELAY)
        if self.s.get("delay_ms"):
            os.environ[DELAY] = str(self.s["delay_ms"])      # (widens the BUILDING window; no assertion depends on it)
        try:
            super().run()
        finally:
            if had is None:
                os.environ.pop(DELAY, None)
            else:
                os.environ[DELAY] = had


# ---- the hdr family's model ----------------------------------------------------------------------------------------------------
M_ = po.MOTION
B_KARIS, B_GAINS, B_STATE = abi.BLOOM_KARIS, abi.BLOOM_GAINS, abi.BLOOM_EXPOSURE_STATE


class _Frame(_Ptr):
    """A per-pixel device buffer at a known address where a helper asks for a tensor: data_ptr(), and cpu().numpy() as the bytes
    of a frame of `channels` 32-bit words per pixel."""

    def __init__(self, r, p, size, channels):
        super().__init__(p)
        self.r, self.shape = r, (size[1], size[0], 4 * channels)

    def cpu(self):
        return self

    def numpy(self):
        return self.r.download(self.p, np.empty(self.shape, np.uint8))


class HdrModel(LateModel):
    """LateModel for the scripts of app_fuzz.script(seed, hdr=True): fovpt_variance, fovpt_variance_filter, fovpt_bloom and
    fovpt_quality inside the chain.  On top of LateModel it keeps on the host: the previous moment history (None: the next step
    has none; fovpt_variance_reset, fovpt_resize -- to the same size too -- and fovpt_set_scene end it, fovpt_temporal_reset,
    fovpt_expose_reset and fovpt_focus_reset do not), the size the context's own variance image was written at, the camera of the
    frame as rendered, and the exposure state (AppModel's, which fovpt_bloom reads with EXPOSURE_STATE).  Every stage's passes,
    gaze and FOV_OFF flag are those of self.frame_as_rendered, never the launch parameters' at call time.

    Log entries, one per stage of a chain: ("variance", had_history, spatial_count, kept_count, reject_depth, reject_class, moved,
    pixels) -- pixels that took the window, pixels with n >= 2, taps rejected by depth and by class, whether the step's interval
    moved a mesh, and the frame's pixel count, which "the window on some pixels but not all" needs across resizes; ("vfilter",
    changed_pixels); ("bloom", flags, steps of the exposure state it read or None without EXPOSURE_STATE, texels of pyramid level 0
    that are not +0); ("quality", flags, differing_pixels)."""

    def __init__(self, oracle, s, model, cam, probe):
        from test_variance_gpu import Moments
        self.var_own_size = None
        self.cam_rendered = None
        super().__init__(oracle, s, model, cam, probe)
        self.mom = Moments(self.r, self.cfg_frame)            # (its `prev` is the model's history; fills and camera are given per step)

    @property
    def var_prev(self):
        return self.mom.prev

    @var_prev.setter
    def var_prev(self, hist):
        self.mom.prev = hist

    def frames(self, op):
        super().frames(op)
        self.cam_rendered = camera(self.r)             # (nothing below changes the camera: the chain's stages use the rendered one)

    def rendered_fills(self):
        """(fill with 1 where no pass writes, pass, fill with 0 there, FOV_OFF) of the frame as rendered."""
        import reconstruct_ref as rr
        import variance_ref as vr
        (w, h), gaze, (ri, ro), uniform = self.frame_as_rendered
        fill, pas = vr.fills(w, h, gaze, ri, ro, int(uniform))
        return fill, pas, rr.writers(w, h, gaze, ri, ro, int(uniform))[0], int(uniform)

    # ---- the four stages
    def variance(self, v, motion, motion_ptr):
        """One fovpt_variance on the accum buffer through test_variance_gpu.Moments.step, with the motion buffer the post step
        wrote and the rendered frame's fills and camera -> (the restatement's variance image, the address the call wrote it to,
        the G-buffer argument it was given)."""
        r = self.r
        g = r.temporal_gbuffer() if v["gbuffer"] == "temporal" else None
        assert (motion is not None) == v["motion"]
        had = self.mom.prev is not None
        hist, var, rec = self.mom.step(v["cfg"], g, None, motion, own=v["own"], label="variance", motion_ptr=motion_ptr,
                                       fill=self.rendered_fills()[0], cam=self.cam_rendered)
        if g is None:
            self.trace_fresh = True                           # (the call's own trace, and the same rays again for the comparison)
        moved = motion is not None and self.last is not None and bool(self.last["moved"].any())
        self.log.append(("variance", had, int(rec["spatial"].sum()), int((hist[..., 2] >= 2).sum()),
                         int(rec["reject_depth"].sum()), int(rec["reject_class"].sum()), moved, int(hist[..., 2].size)))
        if v["own"]:
            self.var_own_size = self.size
        self._late_keep.append(self.mom.out)
        return var, self.mom.out.data_ptr() if self.mom.out is not None else r.variance_buffers()[0], g

    def vfilter(self, f, var, var_ptr, g, color, ptr):
        """One fovpt_variance_filter through test_variance_gpu.run_filter, on the device buffers the stages before it wrote."""
        from test_variance_gpu import run_filter
        r = self.r
        inp, in_ptr = (color, ptr) if f["input"] == "post" else (r.downloadAccum(), None)
        assert f["variance"] == "given" or self.var_own_size == self.size
        fill, pas, _, _ = self.rendered_fills()
        outs = {}
        want, _ = run_filter(self.oracle, r, self.cfg_frame, f["cfg"], inp, var, g, f["out_own"], "vfilter", in_ptr=in_ptr,
                             var_ptr=var_ptr if f["variance"] == "given" else None, fills=(fill, pas), outs=outs)
        if g is None:
            self.trace_fresh = True
        self._late_keep += outs["keep"]
        self.log.append(("vfilter", int((bits(want[..., :3]) != bits(np.asarray(inp, F)[..., :3])).any(axis=-1).sum())))
        return want, outs["color"], outs["got_rgba"], outs["rgba"]

    def bloom(self, b, color, ptr):
        import bloom_ref as br
        from test_bloom_gpu import check
        r = self.r
        d = b["cfg"]
        inp = r.downloadAccum() if color is None else color
        _, _, fill0, uniform = self.rendered_fills()
        E, steps = None, None
        if d["flags"] & B_STATE:                              # the record's exposure once a step has made one, else the config's
            steps = int(self.ex.state["steps"])
            E = self.ex.state["exposure"] if steps else d["exposure"]
        if b["in_place"]:
            assert ptr is not None
            out = (_Frame(r, ptr, self.size, 4), device_images(self.size, 16, 4)[1])
        else:
            out = None if b["own"] else device_images(self.size, 16, 4)
        want = check(self.oracle, r, d, inp, (fill0, uniform), in_ptr=ptr, out=out, E=E, label="bloom")
        off = br.level_offsets(self.size[0], self.size[1], d["levels"])
        lit = int((bits(want["pyramid"][:off[1]]) != 0).any(axis=-1).sum())
        self.log.append(("bloom", d["flags"], steps, lit))
        self._late_keep.append(out)
        if out is None:
            out_c, out_p = r.bloomBuffers()
        else:
            out_c, out_p = out[0].data_ptr(), out[1].data_ptr()
        return want["color"], out_c, want["rgba"], out_p

    def quality(self, q, test, test_ptr, ref, ref_ptr):
        import ctypes as C
        import quality_cases as qc
        import quality_ref as qr
        from test_quality_gpu import qcfg, sums_of
        r = self.r
        (w, h), gaze, (ri, ro), uniform = self.frame_as_rendered
        cfg, full = qcfg(dict(flags=q["flags"], ring_width=q["ring_width"]))
        n = C.sizeof(abi.QualitySums)
        assert n == 1344
        out = None if q["record_own"] else device_filled(n, 0xa5)
        cls = device_filled(w * h, 0xee) if q["classes"] else None
        r.qualityAsync(ref_ptr, test_ptr, cfg, out.data_ptr() if out is not None else None, cls.data_ptr() if cls is not None else None)
        got = r.readQuality(sums=True) if out is None else None
        r.synchronize()
        got = sums_of(out) if out is not None else got
        classes = qr.classes_of_frame(w, h, gaze, ri, ro, int(uniform))
        want = qr.quality(test, ref, classes, gaze, full)
        assert bytes(got) == bytes(qc.sums_of_dict(want)), "quality: record"
        if cls is not None:
            assert np.array_equal(cls.cpu().numpy().reshape(h, w), classes), "quality: class map"
        self.log.append(("quality", q["flags"], int(sum(want["differing"]))))

    def chain(self, c, moved_on=None):
        """post -> variance -> vfilter -> focus -> bloom -> expose -> quality -> packet (of the unwarped frame) -> warp | warp_motion
        | lens: every hand-over a device pointer into the stage before."""
        if "variance" not in c:
            return super().chain(c, moved_on)
        r = self.r
        f = r.launchParams.frame
        if moved_on is not None:
            f.c.x, f.c.y = moved_on["gaze"][0] & 0xffffffff, moved_on["gaze"][1] & 0xffffffff
            f.subframe_index = moved_on["subframe_index"]
        color = ptr = None
        frame_ptr = int(f.frame_buffer)
        rgba, rgba_ptr = self.last_rgba, None if not self._bufs or self._bufs[-1] is None else self._bufs[-1][1].data_ptr()
        post_rgba = post_ptr = motion = motion_ptr = None
        if c["post"] is not None:
            had = self.prev is not None
            out = self.step(stages=c["post"])
            color, ptr = out["color"], r.post_buffers()[0]
            rgba, rgba_ptr = r.downloadPostPixels(), r.post_buffers()[1]
            post_rgba, post_ptr = rgba, rgba_ptr
            if c["post"] & M_:
                motion, motion_ptr = out["motion"], r.motion_buffer()
            self.log.append(("post", c["post"], had))
        if c["variance"] is not None:
            if c["variance"]["adopt"]:                        # an adoption between the step's trace and the call that is handed it
                assert self.rec["flight"]
                self.rebuild_state(True, True)
            var, var_ptr, g = self.variance(c["variance"], motion, motion_ptr)
            if c["vfilter"] is not None:
                color, ptr, rgba, rgba_ptr = self.vfilter(c["vfilter"], var, var_ptr, g, color, ptr)
        if c["focus"] is not None:
            color, ptr, rgba, rgba_ptr = self.focus(c["focus"], color, ptr)
        if c["bloom"] is not None:
            color, ptr, rgba, rgba_ptr = self.bloom(c["bloom"], color, ptr)
        if c["expose"] is not None:
            out = self.expose(c["expose"], r.downloadAccum() if color is None else color, ptr)
            color, ptr = out["color"], r.expose_buffers()[0]
            rgba, rgba_ptr = out["rgba"], r.expose_buffers()[1]
        if c["quality"] is not None:
            ref, ref_ptr = (post_rgba, post_ptr) if c["quality"]["ref"] == "post" else (self.last_rgba, frame_ptr)
            self.quality(c["quality"], rgba, rgba_ptr, ref, ref_ptr)
        if c["packet"]:
            self.packet(rgba, rgba_ptr, c["codec"])
        la = c["last"]
        if la is not None and la["stage"] == "lens":
            self.lens(la, color, ptr)
        elif la is not None:
            self.warp(la, color, ptr, rgba, rgba_ptr)

    # ---- events
    def resize(self, size):
        super().resize(size)
        self.var_prev, self.var_own_size = None, None         # (to the same size as well)

    def set_scene(self):
        super().set_scene()
        self.var_prev = None

    def refused(self, op, check=True):
        from test_bloom_gpu import bcfg
        from test_quality_gpu import qcfg
        from test_variance_gpu import vcfg
        r, which = self.r, op["which"]
        if which == "vfilter_no_image":                       # a frame at this size, and no variance step into the context's image yet
            assert self.rendered and self.var_own_size != self.size
            with_pytest_code(op["code"], lambda: r.variance_filter())
        elif which == "variance_bad_config":                  # refused before anything is enqueued: the history goes on
            with_pytest_code(op["code"], lambda: r.variance(vcfg(**{op["field"]: op["value"]})))
        elif which == "bloom_bad_levels":
            with_pytest_code(op["code"], lambda: r.bloom(bcfg(dict(levels=op["value"]))[0]))
        elif which == "quality_bad_ring":
            with_pytest_code(op["code"], lambda: r.qualityAsync(int(r.launchParams.frame.frame_buffer), None, qcfg(dict(ring_width=op["value"]))[0]))
        else:
            return super().refused(op, check)

    def run_op(self, op):
        if op["op"] == "variance_reset":
            self.r.variance_reset()
            self.var_prev = None
            self.check_info()
        else:
            super().run_op(op)
