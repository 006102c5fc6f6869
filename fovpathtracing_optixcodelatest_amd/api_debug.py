"""The test hooks of SampleRenderer, beside csrc/api_debug.hip: production kernels on inputs a test lays out.  Not part of the
reference's interface."""
import ctypes as C

import numpy as np

from . import abi


class DebugHooks:
    """Mixed into SampleRenderer (renderer.py), which brings _L, _ctx, _check, config and launchParams."""

    def _probe_ref(self, probe):
        """byref of `probe`, or of the launch parameters' probe for None."""
        return C.byref(probe if probe is not None else self.launchParams.probe)

    def debug_trace(self, origins, dirs):
        """The production traversal kernel on a batch of rays -> (global prim id or 0xffffffff, (t, u, v), occluded 0 / 1)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = o.shape[0]
        prim, tuv, occ = np.empty(n, np.uint32), np.empty((n, 3), np.float32), np.empty(n, np.uint8)
        self._check(self._L.fovpt_debug_trace(self._ctx, n, o.ctypes.data, d.ctypes.data, prim.ctypes.data, tuv.ctypes.data, occ.ctypes.data))
        return prim, tuv, occ

    def debug_trace_queued(self, rays, q_count, sq_count, sel=0, it_closest=0, it_shadow=0, grid_closest=0, grid_shadow=0, slots=0,
                           decoy=None, other=None, both=False):
        """The production traversal launches (closest hit, then occlusion) on a queue state laid out here (include/fovpt.h,
        fovpt_debug_trace_queued).  rays = dict(o (n, 3), d (n, 3), slot (n,), target (n,), vis (n, 4), occ (n, 4)); q_count /
        sq_count (8,) = the rays per shard of the radiance / shadow queue; other = the other chain's rays with q_count and
        sq_count among its keys (sel != 0 only); both: run the other chain's launches behind this one's.
        -> dict: cap; hit = dict(shard, pos, rec (k, 4) float32, prim) of the hit-buffer entries found, in ascending physical
        order; hit_found; cells (N + 1, max_depth, 4) and alpha (N + 1, 4) float32 of all N = n + n_other slots and the trap
        slot, the fill pattern abi.DEBUG_SHADE_FILL where nothing was written; stat_radiance, stat_shadow, stat_paths (what the
        launches added); counters_changed; queues_unchanged."""
        L = abi.DebugTraceLaunch()
        keep = []                                                   # (the arrays the struct points into)

        def put(prefix, r):
            o = np.ascontiguousarray(r["o"], np.float32).reshape(-1, 3)
            k = o.shape[0]
            a = dict(origins3=o, dirs3=np.ascontiguousarray(r["d"], np.float32).reshape(k, 3),
                     slot=np.ascontiguousarray(r["slot"], np.uint32).reshape(k), target=np.ascontiguousarray(r["target"], np.uint32).reshape(k),
                     vis4=np.ascontiguousarray(r["vis"], np.float32).reshape(k, 4), occ4=np.ascontiguousarray(r["occ"], np.float32).reshape(k, 4))
            for key, arr in a.items():
                keep.append(arr)
                setattr(L, prefix + key, arr.ctypes.data)
            return k

        n = put("", rays)
        m = put("other_", other) if other is not None else 0
        L.n, L.n_other, L.sel, L.both = n, m, sel, 1 if both else 0
        L.it_closest, L.it_shadow, L.grid_closest, L.grid_shadow, L.slots = it_closest, it_shadow, grid_closest, grid_shadow, slots
        for s in range(8):
            L.q_count[s], L.sq_count[s] = int(q_count[s]), int(sq_count[s])
            L.other_q_count[s] = int(other["q_count"][s]) if other is not None else 0
            L.other_sq_count[s] = int(other["sq_count"][s]) if other is not None else 0
            L.decoy[s] = int(decoy[s]) if decoy is not None else 0
        N, depth = n + m, self.config.max_depth
        a = dict(hit_place2=np.empty((N, 2), np.uint32), hit4=np.empty((N, 4), np.float32), hit_prim=np.empty(N, np.uint32),
                 cells4=np.empty((N + 1, depth, 4), np.float32), alpha4=np.empty((N + 1, 4), np.float32))
        R = abi.DebugTraceResult()
        for k, v in a.items():
            v.view(np.uint8)[...] = abi.DEBUG_SHADE_FILL
            setattr(R, k, v.ctypes.data)
        self._check(self._L.fovpt_debug_trace_queued(self._ctx, C.byref(L), C.byref(R)))
        k = min(int(R.hit_found), N)
        return dict(cap=int(R.cap), hit=dict(shard=a["hit_place2"][:k, 0], pos=a["hit_place2"][:k, 1], rec=a["hit4"][:k], prim=a["hit_prim"][:k]),
                    hit_found=int(R.hit_found), cells=a["cells4"], alpha=a["alpha4"], stat_radiance=int(R.stat_radiance),
                    stat_shadow=int(R.stat_shadow), stat_paths=int(R.stat_paths), counters_changed=int(R.counters_changed),
                    queues_unchanged=int(R.queues_unchanged))

    def debug_probe_sample(self, r12, plain=False, probe=None):
        """The production probe_sample with its two random numbers given (pairs in [0, 0.999999]) on `probe` (default: the launch
        parameters' probe), searched the way a launch would, or plainly -> dict(row, col, dir, color, pdf, path): path = the
        abi.PROBE_PATH_* bits of the layout that ran."""
        r = np.ascontiguousarray(r12, np.float32).reshape(-1, 2)
        n = r.shape[0]
        rowcol, out, path = np.empty((n, 2), np.int32), np.empty((n, 7), np.float32), C.c_int(0)
        self._check(self._L.fovpt_debug_probe_sample(self._ctx, self._probe_ref(probe),
                                                     abi.DEBUG_PROBE_PLAIN if plain else 0, n, r.ctypes.data, rowcol.ctypes.data,
                                                     out.ctypes.data, C.byref(path)))
        return dict(row=rowcol[:, 0].copy(), col=rowcol[:, 1].copy(), dir=out[:, 0:3].copy(), color=out[:, 3:6].copy(),
                    pdf=out[:, 6].copy(), path=path.value)

    def debug_probe_eval(self, dirs, plain=False, probe=None):
        """probe_dir_to_uv + probe_eval, the backplate of a camera ray -> dict(uv, texel, path)."""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = d.shape[0]
        out, path = np.empty((n, 6), np.float32), C.c_int(0)
        self._check(self._L.fovpt_debug_probe_eval(self._ctx, self._probe_ref(probe),
                                                   abi.DEBUG_PROBE_PLAIN if plain else 0, n, d.ctypes.data, out.ctypes.data, C.byref(path)))
        return dict(uv=out[:, 0:2].copy(), texel=out[:, 2:6].copy(), path=path.value)

    def debug_bsdf(self, material, N, view, albedo, etaI, etaO, seeds, L_given):
        """Per row: bsdf_sample with Random(seed), bsdf_eval / bsdf_pdf at the sampled direction when its pdf is above 0, and
        bsdf_pdf / bsdf_eval at L_given -> the columns of oracle.bsdf_table_given (without `type`)."""
        N, view, albedo, L_given = (np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (N, view, albedo, L_given))
        etaI, etaO = np.ascontiguousarray(etaI, np.float32), np.ascontiguousarray(etaO, np.float32)
        seeds = np.ascontiguousarray(seeds, np.int32)
        n = N.shape[0]
        assert view.shape[0] == albedo.shape[0] == L_given.shape[0] == etaI.size == etaO.size == seeds.size == n
        out = np.empty((n, 14), np.float32)
        self._check(self._L.fovpt_debug_bsdf(self._ctx, C.byref(material), n, N.ctypes.data, view.ctypes.data, albedo.ctypes.data,
                                             etaI.ctypes.data, etaO.ctypes.data, seeds.ctypes.data, L_given.ctypes.data, out.ctypes.data))
        return dict(light=out[:, 0:3].copy(), pdf=out[:, 3].copy(), eval=out[:, 4:7].copy(), pdf_again=out[:, 7].copy(),
                    rng_after=out[:, 8:10].copy().view(np.uint32), eval_given=out[:, 10:13].copy(), pdf_given=out[:, 13].copy())

    def debug_tex2d(self, texture, uv):
        """tex2d of texture `texture` of the scene at (u, v) pairs -> (n, 4) float32."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.empty((uv.shape[0], 4), np.float32)
        self._check(self._L.fovpt_debug_tex2d(self._ctx, int(texture), uv.shape[0], uv.ctypes.data, out.ctypes.data))
        return out

    def debug_shade(self, origin, dir4, prim, tuv, rng3, thr4, depth_iter=0, sel=0, grid=1, partition=0, shard_count=None, probe=None):
        """The production k_shade on n chosen hits, one launch under the current config (max_depth, options, write_guides) ->
        dict: per slot rng (n, 4) uint32, thr, rad (n, max_depth, 4), alpha, guide_n, guide_a (float32; the fill pattern where
        nothing was written); next_count / shadow_count (8,); next / shadow = dict(shard, pos, o, d[, vis, occ]) of the queue
        entries found, in ascending physical order; next_found / shadow_found, counters_changed, cap."""
        o = np.ascontiguousarray(origin, np.float32).reshape(-1, 3)
        n = o.shape[0]
        d = np.ascontiguousarray(dir4, np.float32).reshape(n, 4)
        prim = np.ascontiguousarray(prim, np.uint32).reshape(n)
        tuv = np.ascontiguousarray(tuv, np.float32).reshape(n, 3)
        rng3 = np.ascontiguousarray(rng3, np.uint32).reshape(n, 3)
        thr4 = np.ascontiguousarray(thr4, np.float32).reshape(n, 4)
        depth = self.config.max_depth
        L = abi.DebugShadeLaunch()
        L.n, L.depth_iter, L.grid, L.partition, L.sel = n, depth_iter, grid, partition, sel
        if shard_count is None:
            shard_count = [0] * 8
            shard_count[4 if sel == 2 else 0] = n
        for s in range(8):
            L.shard_count[s] = int(shard_count[s])
        f4 = lambda *shape: np.empty(shape + (4,), np.float32)
        a = dict(rng4=np.empty((n, 4), np.uint32), thr4=f4(n), rad4=f4(n, depth), alpha4=f4(n), guide_n4=f4(n), guide_a4=f4(n),
                 next_place2=np.empty((n, 2), np.uint32), next_o4=f4(n), next_d4=f4(n), shadow_place2=np.empty((n, 2), np.uint32),
                 shadow_o4=f4(n), shadow_d4=f4(n), shadow_vis4=f4(n), shadow_occ4=f4(n))
        for v in a.values():
            v.view(np.uint8)[...] = abi.DEBUG_SHADE_FILL
        R = abi.DebugShadeResult()
        for k, v in a.items():
            setattr(R, k, v.ctypes.data)
        self._check(self._L.fovpt_debug_shade(self._ctx, self._probe_ref(probe), C.byref(L),
                                              o.ctypes.data, d.ctypes.data, prim.ctypes.data, tuv.ctypes.data, rng3.ctypes.data, thr4.ctypes.data,
                                              C.byref(R)))
        nn, ns = min(R.next_found, n), min(R.shadow_found, n)
        return dict(rng=a["rng4"], thr=a["thr4"], rad=a["rad4"], alpha=a["alpha4"], guide_n=a["guide_n4"], guide_a=a["guide_a4"],
                    next_count=np.array(R.next_count[:], np.uint32), shadow_count=np.array(R.shadow_count[:], np.uint32),
                    next=dict(shard=a["next_place2"][:nn, 0], pos=a["next_place2"][:nn, 1], o=a["next_o4"][:nn], d=a["next_d4"][:nn]),
                    shadow=dict(shard=a["shadow_place2"][:ns, 0], pos=a["shadow_place2"][:ns, 1], o=a["shadow_o4"][:ns], d=a["shadow_d4"][:ns],
                                vis=a["shadow_vis4"][:ns], occ=a["shadow_occ4"][:ns]),
                    next_found=int(R.next_found), shadow_found=int(R.shadow_found), counters_changed=int(R.counters_changed), cap=int(R.cap))

    def debug_build(self, tri, mesh_of_prim=None, ploc=True, split_budget=0.0, reinsert_rounds=0, order_children=True):
        """The production hierarchy build over `tri` (T, 9) float32 under explicit switches, and what every stage left -> dict of
        the arrays and scalars of struct fovpt_debug_build_trace (include/fovpt.h), the arrays cut to the build's sizes; an array
        its build did not make (no splits, a tiny build) is None.  Touches neither the scene nor the environment."""
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
        n = tri.shape[0]
        mesh = None if mesh_of_prim is None else np.ascontiguousarray(mesh_of_prim, np.uint32).reshape(n)
        sw = abi.DebugBuildSwitches(1 if ploc else 0, float(split_budget), int(reinsert_rounds), 1 if order_children else 0)
        cap, rounds = int(n * (1.0 + float(split_budget))) + 1, 4097
        ci = max(cap - 1, 1)
        u32, i32, f32 = np.uint32, np.int32, np.float32
        a = dict(split_count=np.zeros(n, u32), split_first=np.zeros(n, u32), ref_prim=np.zeros(cap, u32), boxes=np.zeros((cap, 6), f32),
                 keys_s=np.zeros(cap, np.uint64), vals_s=np.zeros(cap, u32), left0=np.zeros(ci, i32), right0=np.zeros(ci, i32),
                 ibox0=np.zeros((ci, 6), f32), round_end=np.zeros(rounds, u32), left1=np.zeros(ci, i32), right1=np.zeros(ci, i32),
                 ibox1=np.zeros((ci, 6), f32), size_int=np.zeros(ci, u32), node_first=np.zeros(ci, u32), leaf_pos=np.zeros(cap, u32),
                 dp=np.zeros((ci, 4), u32), nodes_pre=np.zeros((ci, 32), u32), nodes=np.zeros((ci, 32), u32), tris=np.zeros((cap, 12), u32))
        T = abi.DebugBuildTrace()
        for k, v in a.items():
            setattr(T, k, v.ctypes.data)
        T.cap_refs, T.cap_rounds = cap, rounds
        self._check(self._L.fovpt_debug_build(self._ctx, n, tri.ctypes.data, mesh.ctypes.data if mesh is not None else None, C.byref(sw), C.byref(T)))
        R, N = int(T.num_refs), int(T.num_nodes)
        I = 0 if T.tiny else R - 1
        size = dict(split_count=n if T.have_count else None, split_first=n if T.have_splits else None, ref_prim=R if T.have_splits else None,
                    boxes=R, keys_s=None if T.tiny else R, vals_s=R, leaf_pos=R, round_end=int(T.num_rounds) if (ploc and not T.tiny) else None,
                    nodes_pre=N, nodes=N, tris=R)
        out = {}
        for k, v in a.items():
            m = size.get(k, None if T.tiny else I)
            out[k] = None if m is None else v[:m].copy()
        for k in ("num_refs", "tiny", "have_count", "have_splits", "root", "num_rounds", "num_nodes", "max_depth", "reinserted", "num_levels"):
            out[k] = int(getattr(T, k))
        out["s_cut"] = np.float32(T.s_cut)
        out["cbounds"] = np.array(T.cbounds[:], np.float32)
        out["level_first"] = [int(x) for x in T.level_first[:int(T.num_levels) + 1]]
        return out

    def debug_resolve_passes(self, render=True, width=0, height=0):
        """The pass table of the frame a render() (or a launch(width, height)) of the current launch parameters would resolve:
        a list of abi.DebugPass.  Sample slot of (pass, launch index li, sample s) = slot_base + li * spp + s."""
        passes, n = (abi.DebugPass * 3)(), C.c_int(0)
        self._check(self._L.fovpt_debug_resolve(self._ctx, C.byref(self.launchParams), 1 if render else 0, int(width), int(height), passes,
                                                C.byref(n), None, None, None, None, None, None, None))
        return [passes[i] for i in range(n.value)]

    def debug_resolve(self, state, cells, alpha, backplate, guide_n=None, guide_a=None, render=True, width=0, height=0):
        """The production resolve kernel on a path state in slot order (debug_resolve_passes): state (slots,) uint32 =
        flags | depth << 8, cells (slots, max_depth, 4), alpha (slots, 4), backplate (launch records, 4), guides (slots, 4) under
        write_guides.  The results are in the frame buffers (downloadAccum, downloadPixels, ...).  Returns the number of
        queue-counter words the kernel left non-zero."""
        passes = self.debug_resolve_passes(render, width, height)
        slots = sum(p.gw * p.rows * p.spp for p in passes)
        launches = sum(p.gw * p.rows for p in passes)
        depth = self.config.max_depth
        state = np.ascontiguousarray(state, np.uint32)
        cells, alpha, backplate = (np.ascontiguousarray(x, np.float32) for x in (cells, alpha, backplate))
        assert state.shape == (slots,) and cells.shape == (slots, depth, 4) and alpha.shape == (slots, 4) and backplate.shape == (launches, 4)
        guides = []
        for g in (guide_n, guide_a):
            if g is not None:
                g = np.ascontiguousarray(g, np.float32)
                assert g.shape == (slots, 4)
            guides.append(g)
        out, n, left = (abi.DebugPass * 3)(), C.c_int(0), C.c_uint32(0)
        self._check(self._L.fovpt_debug_resolve(self._ctx, C.byref(self.launchParams), 1 if render else 0, int(width), int(height), out, C.byref(n),
                                                state.ctypes.data, cells.ctypes.data, alpha.ctypes.data,
                                                guides[0].ctypes.data if guides[0] is not None else None,
                                                guides[1].ctypes.data if guides[1] is not None else None, backplate.ctypes.data, C.byref(left)))
        return left.value

    def debug_generate(self, render=True, width=0, height=0, rows=None, sel=0, slot_begin=0, slot_end=0, grid=0):
        """The production generate launch on the frame a render() (or a launch(width, height), or its chunk of launch rows
        rows = (row0, row1)) of the current launch parameters would run, as a job launches it: sel = 0 or a chain's 1 / 2, the
        sample slots [slot_begin, slot_end) (0, 0: a job's own), grid blocks (0: a job's own) -> dict: passes (list of
        abi.DebugPass), rng (slots, 4) uint32, backplate (launch records, 4), guide_n / guide_a (slots, 4) or None without
        write_guides -- the fill pattern abi.DEBUG_SHADE_FILL where nothing was written --, count (8,), found, counters_changed,
        cap, kernel (0 k_generate, 1 k_generate_owned), slot_begin, slot_end, grid as launched, and the queue entries found in
        ascending physical order: shard, pos, o (n, 4), d (n, 4)."""
        L = abi.DebugGenerateLaunch()
        L.render, L.width, L.height = 1 if render else 0, int(width), int(height)
        L.row0, L.row1 = (int(rows[0]), int(rows[1])) if rows is not None else (0, 0)
        L.sel, L.slot_begin, L.slot_end, L.grid = int(sel), int(slot_begin), int(slot_end), int(grid)
        passes, n = (abi.DebugPass * 3)(), C.c_int(0)
        self._check(self._L.fovpt_debug_generate(self._ctx, C.byref(self.launchParams), C.byref(L), passes, C.byref(n), None))
        table = [passes[i] for i in range(n.value)]
        slots = sum(p.gw * p.rows * p.spp for p in table)
        launches = sum(p.gw * p.rows for p in table)
        guides = bool(self.config.write_guides)
        a = dict(rng4=np.empty((slots, 4), np.uint32), backplate4=np.empty((launches, 4), np.float32), place2=np.empty((slots, 2), np.uint32),
                 o4=np.empty((slots, 4), np.float32), d4=np.empty((slots, 4), np.float32))
        if guides:
            a.update(guide_n4=np.empty((slots, 4), np.float32), guide_a4=np.empty((slots, 4), np.float32))
        R = abi.DebugGenerateResult()
        for k, v in a.items():
            v.view(np.uint8)[...] = abi.DEBUG_SHADE_FILL
            setattr(R, k, v.ctypes.data)
        self._check(self._L.fovpt_debug_generate(self._ctx, C.byref(self.launchParams), C.byref(L), passes, C.byref(n), C.byref(R)))
        assert bool(R.guides) == guides
        m = min(R.found, slots)
        return dict(passes=table, rng=a["rng4"], backplate=a["backplate4"], guide_n=a.get("guide_n4"), guide_a=a.get("guide_a4"),
                    count=np.array(R.count[:], np.uint32), found=int(R.found), counters_changed=int(R.counters_changed), cap=int(R.cap),
                    kernel=int(R.kernel), slot_begin=int(R.slot_begin), slot_end=int(R.slot_end), grid=int(R.grid),
                    shard=a["place2"][:m, 0], pos=a["place2"][:m, 1], o=a["o4"][:m], d=a["d4"][:m])

    def debug_math(self, op, a, b=None):
        a = np.ascontiguousarray(a, np.float32)
        bb = np.ascontiguousarray(b, np.float32) if b is not None else None
        out = np.empty_like(a)
        self._check(self._L.fovpt_debug_math(self._ctx, op, a.ctypes.data, bb.ctypes.data if bb is not None else None,
                                             out.ctypes.data, a.size))
        return out
