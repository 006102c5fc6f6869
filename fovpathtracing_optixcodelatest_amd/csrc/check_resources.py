#!/usr/bin/env python3
"""Build guard (Makefile): reads the -Rpass-analysis=kernel-resource-usage remarks of a device compile and fails when a
per-frame kernel (k_generate, k_traverse, k_shade, k_resolve, the denoiser's k_denoise_*, the reconstruction's k_gbuffer_* and
k_reconstruct, the temporal reprojection's k_temporal, the refit's k_gather_vertices / k_refit_level / k_flatten,
the transforms' k_transform_vertices*, the rig's k_rig_pose, the skinning's k_skin_vertices, the morph targets' k_morph_vertices / k_morph_skin_vertices, the cost measurement's k_tree_cost*, the exposure's k_expose_*, the bloom stage's k_bloom_*, the warp's k_warp_* (k_warp_scatter_motion of fovpt_warp_motion among them), the frame packets' k_packet_*, the focus stage's k_focus_*, the lens pre-distortion's k_lens, the variance stage's k_variance_moments and k_vfilter_*, the quality measurement's k_quality_*) uses scratch memory, when k_rig_pose's LDS is not the 48 KiB it is designed for, or when k_traverse drops below the waves per
SIMD it is written for.  (The one-off kernels of the BVH build -- k_collapse4, rocPRIM's radix sort -- do use scratch, and run.)

Why: every hot kernel here is tuned to a register budget; a compiler or flag change that makes one spill would silently
turn LDS / register traffic into scratch traffic.  (Round 2 saw a diagnostic build of k_traverse that used scratch die with
HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION; the product must never get there unnoticed.)"""
import re, sys

HOT = ("k_generate", "k_traverse", "k_shade", "k_resolve", "k_denoise", "k_gbuffer", "k_reconstruct", "k_temporal", "k_gather_vertices",
       "k_refit_level", "k_flatten", "k_transform_vertices", "k_rig_pose", "k_skin_vertices", "k_morph_vertices", "k_morph_skin_vertices", "k_tree_cost", "k_expose", "k_bloom", "k_warp", "k_packet", "k_focus", "k_lens", "k_quality", "k_variance", "k_vfilter")
text = open(sys.argv[1]).read()
bad = []
name = None
for line in text.splitlines():
    m = re.search(r"remark: Function Name: (\S+)", line)
    if m:
        name = m.group(1)
        continue
    m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
    if m and name and any(h in name for h in HOT) and int(m.group(1)) != 0:
        bad.append("%s uses %s bytes of scratch per lane" % (name, m.group(1)))
    m = re.search(r"remark:\s+Occupancy \[waves/SIMD\]: (\d+)", line)
    if m and name and "k_traverse" in name and int(m.group(1)) < 8 and "--allow-low-occupancy" not in sys.argv:
        bad.append("%s reaches only %s waves per SIMD (8 expected)" % (name, m.group(1)))
    m = re.search(r"remark:\s+LDS Size \[bytes/block\]: (\d+)", line)
    if m and name and "k_rig_pose" in name and int(m.group(1)) != 48 * 1024:      # the worlds of FOVPT_RIG_MAX_NODES nodes, nothing else
        bad.append("%s uses %s bytes of LDS (49152 expected)" % (name, m.group(1)))
if bad:
    sys.stderr.write("check_resources: " + "; ".join(bad) + "\n")
    sys.exit(1)
