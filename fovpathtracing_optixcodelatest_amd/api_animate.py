"""The animated geometry of SampleRenderer, beside csrc/api_animate.hip: vertex, transform, skin, morph and rig updates, the
background rebuild and the cost of the refit hierarchy."""
import ctypes as C

import numpy as np

from . import abi


class Animation:
    """Mixed into SampleRenderer (renderer.py), which brings _L, _ctx, _check, model and _keep_updates."""

    # -- what update_vertices, update_skinned and update_morphed share
    @staticmethod
    def _all_device(who, values):
        """All host or all device: True when there are values and every one is a CUDA tensor; a mix raises ValueError."""
        on_device = [hasattr(v, "is_cuda") and bool(v.is_cuda) for v in values]
        if any(on_device) and not all(on_device):
            raise ValueError("%s: mixes host arrays and device tensors" % who)
        return bool(on_device) and all(on_device)

    @staticmethod
    def _host_palette(who, mesh, m, noun):
        """A (J, 3, 4) array, or a (J, 4, 4) one whose last rows are 0 0 0 1, as contiguous (J, 3, 4) float32."""
        m = np.asarray(m, np.float32)
        if m.ndim == 3 and m.shape[1:] == (4, 4):
            if not (m[:, 3] == np.float32([0, 0, 0, 1])).all():
                raise ValueError("%s: mesh %d: the last row of a (4, 4) matrix must be 0 0 0 1" % (who, mesh))
            m = m[:, :3]
        if m.ndim != 3 or m.shape[1:] != (3, 4):
            raise ValueError("%s: mesh %d needs a (J, 3, 4) or (J, 4, 4) %s" % (who, mesh, noun))
        return np.ascontiguousarray(m)

    @staticmethod
    def _device_palette(who, mesh, m):
        """The device pointer of a contiguous float32 (J, 3, 4) CUDA tensor."""
        import torch
        if m.dtype != torch.float32 or m.dim() != 3 or tuple(m.shape[1:]) != (3, 4) or not m.is_contiguous():
            raise ValueError("%s: mesh %d needs a contiguous (J, 3, 4) float32 tensor" % (who, mesh))
        return m.data_ptr()

    @staticmethod
    def _rebuild_flag(rebuild):
        """rebuild=False / True / "async" as FOVPT_UPDATE_* bits (True: synchronous; "async": beside the frames, rebuild_state())."""
        if isinstance(rebuild, str):
            if rebuild != "async":
                raise ValueError("rebuild is False, True or \"async\", not %r" % (rebuild,))
            return abi.UPDATE_REBUILD_ASYNC
        return abi.UPDATE_REBUILD if rebuild else 0

    def _update(self, fn, entries, num, device, rebuild, keep):
        self._check(fn(self._ctx, entries, num, (abi.UPDATE_DEVICE if device else 0) | self._rebuild_flag(rebuild)))
        if device:
            self._keep_updates = keep          # (the tensors are read on the stream after the call returns)

    # -- animated geometry (include/fovpt.h, fovpt_update_vertices): optixAccelBuild(OPERATION_UPDATE) over the same build inputs
    def update_vertices(self, updates, rebuild=False):
        """New vertex positions for meshes of the scene: updates maps a mesh index to an (n, 3) float32 numpy array, or to a
        CUDA torch tensor (device pointers, read in stream order on the renderer's stream: torch's writes of them must be ordered
        before the call).  All host or all device.  rebuild=False refits the hierarchy asynchronously; True builds it anew
        (synchronous).  The renderer's Model is not changed."""
        items = sorted(updates.items())
        device = self._all_device("update_vertices", updates.values())
        ups = (abi.VertexUpdate * max(1, len(items)))()
        keep = []
        for k, (mesh, v) in enumerate(items):
            if device:
                import torch
                if v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3:
                    raise ValueError("update_vertices: mesh %d needs an (n, 3) float32 tensor" % mesh)
                v = v.contiguous()
                ptr, n = v.data_ptr(), v.shape[0]
            else:
                v = np.ascontiguousarray(v, np.float32)
                if v.ndim != 2 or v.shape[1] != 3:
                    raise ValueError("update_vertices: mesh %d needs an (n, 3) array" % mesh)
                ptr, n = v.ctypes.data, v.shape[0]
            keep.append(v)
            ups[k].mesh, ups[k].num_vertices, ups[k].vertex = int(mesh), int(n), ptr
        self._update(self._L.fovpt_update_vertices, ups, len(items), device, rebuild, keep)

    # -- rigid motion and the cost of the refit tree (include/fovpt.h, fovpt_update_transforms / fovpt_hierarchy_cost)
    def update_transforms(self, transforms, rebuild=False):
        """Per-mesh affine transforms of the positions the scene was set with: transforms maps a mesh index to a (3, 4) array,
        or a (4, 4) one whose last row is 0 0 0 1 (ValueError otherwise).  Absolute, not cumulative; applied on the device, then
        update_vertices()' refit (or, rebuild=True, rebuild) with the same ordering.  The renderer's Model is not changed."""
        items = sorted(transforms.items())
        tfs = (abi.MeshTransform * max(1, len(items)))()
        for k, (mesh, m) in enumerate(items):
            m = np.asarray(m, np.float32)
            if m.shape == (4, 4):
                if not np.array_equal(m[3], np.float32([0, 0, 0, 1])):
                    raise ValueError("update_transforms: mesh %d: the last row of a (4, 4) matrix must be 0 0 0 1" % mesh)
                m = m[:3]
            if m.shape != (3, 4):
                raise ValueError("update_transforms: mesh %d needs a (3, 4) or (4, 4) matrix" % mesh)
            tfs[k].mesh = int(mesh)
            tfs[k].m[:] = [float(x) for x in m.reshape(-1)]
        self._check(self._L.fovpt_update_transforms(self._ctx, tfs, len(items), self._rebuild_flag(rebuild)))

    def rebuild_state(self, wait=False, adopt=False) -> abi.RebuildInfo:
        """The background rebuild an update with rebuild="async" starts (state REBUILD_IDLE / _BUILDING / _READY, the counters,
        last_error, snapshot_update, ms_build).  Never waits for the device.  wait=True waits until the state is not BUILDING;
        adopt=True makes a READY hierarchy the scene's now (otherwise the next update that enqueues something does)."""
        out = abi.RebuildInfo()
        self._check(self._L.fovpt_rebuild_state(self._ctx, (abi.REBUILD_WAIT if wait else 0) | (abi.REBUILD_ADOPT if adopt else 0), C.byref(out)))
        return out

    def hierarchy_cost(self, wait=False) -> abi.HierarchyCost:
        """The SAH cost of the hierarchy as built and as last measured on the device (built, current, updates, measured).  The
        first call switches watching on: every later refit is followed by a measurement.  wait=False never blocks and may lag
        (measured < updates); wait=True measures the present tree if need be and waits for it.  Rebuild when current / built
        passes your threshold."""
        out = abi.HierarchyCost()
        self._check(self._L.fovpt_hierarchy_cost(self._ctx, abi.COST_WAIT if wait else 0, C.byref(out)))
        return out

    # -- skinning (include/fovpt.h, fovpt_set_skins / fovpt_update_skinned)
    def set_skins(self, skins):
        """Sets, replaces or removes the skins of meshes: skins maps a mesh index to (joints (n, 4) uint16, weights (n, 4)
        float32), n the mesh's vertex count, or to None (remove).  The skin's joint count is the largest index used plus one; a
        third element, (joints, weights, num_joints), states it instead.  Weights are used as given, not normalised.  Set-up-time
        state of the scene: copied before the call returns, geometry does not move.  Bad shapes raise ValueError."""
        items = sorted(skins.items())
        sk = (abi.MeshSkin * max(1, len(items)))()
        keep = []
        for k, (mesh, jw) in enumerate(items):
            if not 0 <= int(mesh) < len(self.model.meshes):
                raise ValueError("set_skins: mesh %d of %d" % (mesh, len(self.model.meshes)))
            sk[k].mesh, sk[k].num_vertices = int(mesh), int(self.model.meshes[mesh].vertex.shape[0])
            if jw is None:
                continue
            j, w = jw[0], jw[1]
            j = np.asarray(j)
            if j.ndim != 2 or j.shape[1] != 4 or j.dtype.kind not in "ui" or (j.size and (j.min() < 0 or j.max() > 0xffff)):
                raise ValueError("set_skins: mesh %d needs (n, 4) joint indices that fit uint16" % mesh)
            j, w = np.ascontiguousarray(j, np.uint16), np.ascontiguousarray(w, np.float32)
            if w.shape != j.shape:
                raise ValueError("set_skins: mesh %d needs (n, 4) weights, one per joint index" % mesh)
            keep += [j, w]
            sk[k].num_vertices, sk[k].num_joints = j.shape[0], (int(jw[2]) if len(jw) > 2 else int(j.max()) + 1 if j.size else 1)
            sk[k].joints, sk[k].weights = j.ctypes.data, w.ctypes.data
        self._check(self._L.fovpt_set_skins(self._ctx, sk, len(items)))

    def update_skinned(self, poses, rebuild=False):
        """Poses of skinned meshes: poses maps a mesh index to its palette, a (J, 3, 4) array or a (J, 4, 4) one whose last rows
        are 0 0 0 1, or a contiguous float32 CUDA torch tensor (J, 3, 4) (read in stream order on the renderer's stream, not
        validated), J the joint count of the mesh's skin.  All host or all device.  Every vertex's rest position goes through the
        weighted sum of its four joints' matrices on the device; absolute, not cumulative; then update_vertices()' refit (or,
        rebuild=True, rebuild) with the same ordering.  Bad shapes raise ValueError.  The renderer's Model is not changed."""
        items = sorted(poses.items())
        device = self._all_device("update_skinned", poses.values())
        ps = (abi.SkinPose * max(1, len(items)))()
        keep = []
        for k, (mesh, m) in enumerate(items):
            if device:
                ptr = self._device_palette("update_skinned", mesh, m)
            else:
                m = self._host_palette("update_skinned", mesh, m, "array")
                ptr = m.ctypes.data
            keep.append(m)
            ps[k].mesh, ps[k].num_joints, ps[k].matrices = int(mesh), int(m.shape[0]), ptr
        self._update(self._L.fovpt_update_skinned, ps, len(items), device, rebuild, keep)

    # -- morph targets (include/fovpt.h, fovpt_set_morphs / fovpt_update_morphed)
    def set_morphs(self, morphs):
        """Sets, replaces or removes the morph targets of meshes: morphs maps a mesh index to a list of targets or to None
        (remove).  A target is a dense (n, 3) float32 array of deltas, n the mesh's vertex count, or a pair (index (k,) unsigned
        integers, strictly ascending, delta (k, 3) float32) that moves k of the vertices; k may be 0.  Set-up-time state of the
        scene: copied before the call returns, geometry does not move.  Bad shapes raise ValueError."""
        items = sorted(morphs.items())
        mm = (abi.MeshMorph * max(1, len(items)))()
        keep = []
        for k, (mesh, targets) in enumerate(items):
            if not 0 <= int(mesh) < len(self.model.meshes):
                raise ValueError("set_morphs: mesh %d of %d" % (mesh, len(self.model.meshes)))
            nv = int(self.model.meshes[mesh].vertex.shape[0])
            mm[k].mesh, mm[k].num_vertices = int(mesh), nv
            if targets is None:
                continue
            if len(targets) == 0:
                raise ValueError("set_morphs: mesh %d: an empty list of targets (None removes them)" % mesh)
            ts = (abi.MorphTarget * len(targets))()
            for t, target in enumerate(targets):
                if isinstance(target, tuple):
                    idx, d = np.asarray(target[0]), np.ascontiguousarray(target[1], np.float32).reshape(-1, 3)
                    if idx.ndim != 1 or (idx.size and (idx.dtype.kind not in "ui" or idx.min() < 0 or idx.max() > 0xffffffff)) or idx.shape[0] != d.shape[0]:
                        raise ValueError("set_morphs: mesh %d target %d needs (k,) vertex indices and (k, 3) deltas" % (mesh, t))
                    idx = np.ascontiguousarray(idx, np.uint32)
                    keep.append(idx)
                    ts[t].index = idx.ctypes.data
                else:
                    d = np.ascontiguousarray(target, np.float32)
                    if d.ndim != 2 or d.shape != (nv, 3):
                        raise ValueError("set_morphs: mesh %d target %d: a dense target needs (%d, 3) deltas" % (mesh, t, nv))
                keep.append(d)
                ts[t].count, ts[t].delta = d.shape[0], (d.ctypes.data if d.shape[0] else None)
            keep.append(ts)
            mm[k].num_targets, mm[k].targets = len(targets), ts
        self._check(self._L.fovpt_set_morphs(self._ctx, mm, len(items)))

    def update_morphed(self, poses, rebuild=False):
        """Poses of morphed meshes: poses maps a mesh index to its weights, a (T,) float32 array, T the mesh's target count, or to
        a pair (weights, palette) whose palette is what update_skinned() takes for the mesh's skin; or to contiguous float32 CUDA
        torch tensors, (T,) and (J, 3, 4) (read in stream order on the renderer's stream, not validated).  All host or all
        device.  Every vertex's rest position takes w[t] * delta of each of its targets whose weight is not zero, in ascending
        targets, and then goes through the skin where a palette is given; absolute, not cumulative; then update_vertices()'
        refit (or, rebuild=True, rebuild) with the same ordering.  Bad shapes raise ValueError.  The renderer's Model is not
        changed."""
        items = [(mesh, v if isinstance(v, tuple) else (v, None)) for mesh, v in sorted(poses.items())]
        device = self._all_device("update_morphed", [x for _, v in items for x in v if x is not None])
        ps = (abi.MorphPose * max(1, len(items)))()
        keep = []
        for k, (mesh, (w, m)) in enumerate(items):
            if device:
                import torch
                if w.dtype != torch.float32 or w.dim() != 1 or not w.is_contiguous():
                    raise ValueError("update_morphed: mesh %d needs a contiguous (T,) float32 tensor of weights" % mesh)
                wp, mp = w.data_ptr(), (None if m is None else self._device_palette("update_morphed", mesh, m))
            else:
                w = np.ascontiguousarray(w, np.float32)
                if w.ndim != 1:
                    raise ValueError("update_morphed: mesh %d needs a (T,) array of weights" % mesh)
                if m is not None:
                    m = self._host_palette("update_morphed", mesh, m, "palette")
                wp, mp = w.ctypes.data, (None if m is None else m.ctypes.data)
            keep += [w, m]
            ps[k].mesh, ps[k].num_targets, ps[k].weights = int(mesh), int(w.shape[0]), wp
            ps[k].num_joints, ps[k].matrices = (0 if m is None else int(m.shape[0])), mp
        self._update(self._L.fovpt_update_morphed, ps, len(items), device, rebuild, keep)

    # -- rigs (include/fovpt.h, fovpt_set_rig / fovpt_update_animated)
    @staticmethod
    def pack_rig(rig):
        """(abi.RigDesc, what it points to) of a rig: a dict with parent (N,) integers, translation (N, 3), rotation (N, 4)
        (x y z w) and scale (N, 3) float32, the nodes' parents and rest poses; bindings, a list of dicts with mesh and either
        node (rigid), or joint_nodes (J,) and inverse_bind (J, 3, 4), or neither (morph weights only); clips, a list of lists of
        channels, each a dict with target, path and interpolation (abi.RIG_*), times (K,) and values (K, 3 / 4 / 3 / targets).
        Bad shapes raise ValueError; the values themselves are the library's to check."""
        keep = []

        def arr(a, dtype, shape, what):
            a = np.ascontiguousarray(a, dtype)
            if a.ndim != len(shape) or any(s is not None and s != d for s, d in zip(shape, a.shape)):
                raise ValueError("set_rig: %s needs shape %s, not %s" % (what, shape, a.shape))
            keep.append(a)
            return a

        parent = arr(rig["parent"], np.int32, (None,), "parent")
        n = parent.shape[0]
        t, q, s = arr(rig["translation"], np.float32, (n, 3), "translation"), arr(rig["rotation"], np.float32, (n, 4), "rotation"), \
            arr(rig["scale"], np.float32, (n, 3), "scale")
        nodes = (abi.RigNode * max(1, n))()
        for i in range(n):
            nodes[i].parent = int(parent[i])
            nodes[i].translation[:], nodes[i].rotation[:], nodes[i].scale[:] = t[i].tolist(), q[i].tolist(), s[i].tolist()
        bindings = list(rig.get("bindings", ()))
        bs = (abi.RigBinding * max(1, len(bindings)))()
        for k, b in enumerate(bindings):
            bs[k].mesh, bs[k].node = int(b["mesh"]), int(b.get("node", -1))
            if b.get("joint_nodes") is not None:
                j = np.asarray(b["joint_nodes"])
                if j.ndim != 1 or j.dtype.kind not in "ui" or (j.size and (j.min() < 0 or j.max() > 0xffff)):
                    raise ValueError("set_rig: binding %d needs (J,) joint nodes that fit uint16" % k)
                j = arr(j, np.uint16, (None,), "joint_nodes")
                ib = Animation._host_palette("set_rig", int(b["mesh"]), b["inverse_bind"], "inverse bind palette")
                if ib.shape[0] != j.shape[0]:
                    raise ValueError("set_rig: binding %d needs one inverse bind matrix per joint node" % k)
                keep.append(ib)
                bs[k].num_joints, bs[k].joint_nodes, bs[k].inverse_bind = j.shape[0], j.ctypes.data, ib.ctypes.data
        clips = list(rig.get("clips", ()))
        cs = (abi.RigClip * max(1, len(clips)))()
        for k, clip in enumerate(clips):
            ch = (abi.RigChannel * max(1, len(clip)))()
            for h, c in enumerate(clip):
                times = arr(c["times"], np.float32, (None,), "clip %d channel %d: times" % (k, h))
                values = arr(c["values"], np.float32, (times.shape[0], None), "clip %d channel %d: values" % (k, h))
                width = {abi.RIG_TRANSLATION: 3, abi.RIG_ROTATION: 4, abi.RIG_SCALE: 3}.get(int(c["path"]))
                if width is not None and values.shape[1] != width:
                    raise ValueError("set_rig: clip %d channel %d needs (K, %d) values" % (k, h, width))
                ch[h].target, ch[h].path, ch[h].interpolation, ch[h].num_keys = int(c["target"]), int(c["path"]), int(c["interpolation"]), times.shape[0]
                ch[h].times, ch[h].values = times.ctypes.data, values.ctypes.data
            keep.append(ch)
            cs[k].num_channels, cs[k].channels = len(clip), ch
        desc = abi.RigDesc()
        desc.nodes, desc.num_nodes, desc.bindings, desc.num_bindings, desc.clips, desc.num_clips = nodes, n, bs, len(bindings), cs, len(clips)
        keep += [nodes, bs, cs]
        return desc, keep

    def set_rig(self, rig):
        """Sets, replaces or (None) removes the scene's rig: see pack_rig() for the form.  Called after set_skins() / set_morphs(),
        either of which drops it.  Set-up-time state of the scene: copied before the call returns, geometry does not move."""
        if rig is None:
            self._check(self._L.fovpt_set_rig(self._ctx, None))
            return
        desc, keep = self.pack_rig(rig)
        self._check(self._L.fovpt_set_rig(self._ctx, C.byref(desc)))
        del keep

    def update_animated(self, clip, time, rebuild=False):
        """Poses every mesh the rig binds from clip `clip` at `time`: the keys are sampled, the hierarchy composed and the
        palettes, weights and rigid matrices applied on the device; absolute, not cumulative; then update_vertices()' refit (or,
        rebuild=True, rebuild) with the same ordering.  The caller wraps its own time to loop.  The renderer's Model is not
        changed."""
        self._check(self._L.fovpt_update_animated(self._ctx, int(clip), float(time), self._rebuild_flag(rebuild)))
