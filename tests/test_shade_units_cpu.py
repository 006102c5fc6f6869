"""The reference side of the sample-level shading tests (tests/shade_cases.py, tests/test_shade_units_gpu.py), without a GPU.

Two things are shown here.  The oracle's new rows are anchored: orc_probe_sample_at is ProbeSample on the numbers the stream
draws and its searches are np.searchsorted on every sorted CDF, the extended BSDF table is the existing one plus columns that
agree with the binary64 restatement, oracle.tex2d is bilinear wrap addressing.  And the cases cannot pass vacuously: the
numbers handed to the searches are bit-equal to guide abscissae and CDF entries, every texel of the small probes is returned,
columns behind flat CDF runs are returned, no search leaves its row, every lobe and total internal reflection occur, light
directions below the surface occur, and NaN rows are rare."""
import numpy as np
import pytest

import shade_cases as sc


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sorted(hp):
    return bool((np.diff(hp.cdfy) >= 0).all() and (np.diff(hp.cdfx, axis=1) >= 0).all())


@pytest.mark.parametrize("case", sc.probe_cases(), ids=lambda c: c.name)
def test_probe_sample_at_is_probe_sample_on_the_streams_numbers(oracle, case):
    """Random(seed) draws r1 = Randf(0, 1), r2 = Randf(0, 1) per sample (Sample2D): fed those numbers, orc_probe_sample_at gives
    what orc_probe_sample gives for the seed, bit for bit.  Both go through the oracle's ProbeSampleAt, so what this pins is
    the hand-over -- which two numbers of the stream a sample takes, in which order, and that Randf(0, 1) passes them
    unchanged.  That ProbeSampleAt itself is ProbeSample is held by the searchsorted check below and by the vectors the
    reference's own code produced (tests/test_ref_pin_cpu.py)."""
    hp = case.host_probe(oracle)
    for seed in (0, 1, 12345, 0x7fffffff, 0xdeadbeef):
        n = 500
        d, c, p = oracle.probe_sample(hp, seed if seed < 0x80000000 else seed - (1 << 32), n)
        f = oracle.random_stream(seed, 2 * n)[1]
        r12 = ((np.float32(1.0) - f) * np.float32(0.0) + f * np.float32(1.0)).astype(np.float32).reshape(n, 2)     # Randf(min, max), maths.h:213-217
        assert np.array_equal(_bits(r12), _bits(f.reshape(n, 2)))                      # (the identity on Randf's range)
        got = oracle.probe_sample_at(hp, r12)
        assert np.array_equal(_bits(got["dir"]), _bits(d)) and np.array_equal(_bits(got["color"]), _bits(c))
        assert np.array_equal(_bits(got["pdf"]), _bits(p))


@pytest.mark.parametrize("case", sc.probe_cases(), ids=lambda c: c.name)
def test_probe_case_conditions(oracle, case):
    """What the pairs of a probe case reach, from the reference alone.  Two conditions are deliberately narrower than "for
    every probe": 100 numbers bit-equal to a CDF entry are not asked of the 1 x 1 probe, whose only entries are 1.0, above
    Randf's range; and a returned column behind a flat run of five or more equal entries is asked of the two cases built to
    have such runs (flat_run) -- the CDFs of the others have none, so no input could return one."""
    hp, r12, want = sc.probe_reference(oracle, case)
    h, w = case.height, case.width
    row, col = want["row"], want["col"]
    assert r12.min() >= 0.0 and r12.max() <= sc.R_MAX and np.isfinite(r12).all()
    # no search leaves its array (the reference would read past the row: such inputs are outside the contract)
    assert row.min() >= 0 and row.max() < h and col.min() >= 0 and col.max() < w, (row.max(), col.max())
    # on sorted CDFs the two searches are lower bounds
    if _sorted(hp):
        assert np.array_equal(row, np.searchsorted(hp.cdfy, r12[:, 0], "left"))
        for k in np.unique(row):
            m = row == k
            assert np.array_equal(col[m], np.searchsorted(hp.cdfx[k], r12[m, 1], "left")), k
    else:
        assert case.path == sc.PATH_PLAIN
    # numbers bit-equal to a guide abscissa, and to a CDF entry
    on_guide = int(np.isin(r12[:, 0], sc.guide_abscissae(h)).sum() + np.isin(r12[:, 1], sc.guide_abscissae(w)).sum())
    on_entry = int(np.isin(r12[:, 0], hp.cdfy).sum() + np.isin(r12[:, 1], hp.cdfx[np.unique(row)].ravel()).sum())
    print(case.name, "pairs", len(r12), "on a guide abscissa", on_guide, "on a CDF entry", on_entry)
    assert on_guide >= 100
    if (hp.cdfy <= sc.R_MAX).any() or (hp.cdfx <= sc.R_MAX).any():
        assert on_entry >= 100
    else:
        assert (h, w) == (1, 1)            # its only entries are 1.0, above Randf's range: no number can equal one
    # every texel that can be sampled is returned (small probes)
    if h * w <= 300:
        positive = (hp.pdfx > 0) & (hp.pdfy > 0)[:, None]
        if case.tables is not None:        # hand-made tables: what can be sampled is what the CDFs step at
            positive = (np.diff(hp.cdfx, axis=1, prepend=0.0) > 0) & (np.diff(hp.cdfy, prepend=0.0) > 0)[:, None]
        seen = np.zeros((h, w), bool)
        seen[row, col] = True
        assert seen[positive].all(), np.argwhere(positive & ~seen)[:8]
    # a returned column behind a flat run of five or more equal entries
    if case.flat_run:
        behind = 0
        for k in np.unique(row):
            c = hp.cdfx[k]
            for j in np.unique(col[row == k]):
                behind += int(j >= 5 and (c[j - 5:j] == c[j - 1]).all() and c[j] > c[j - 1])
        print(case.name, "columns behind a flat run", behind)
        assert behind >= 1


def test_probe_layouts_are_all_asked_for():
    paths = {c.path for c in sc.probe_cases()}
    assert {sc.PATH_PLAIN, sc.PATH_GUIDED | sc.PATH_RECORDS, sc.PATH_GUIDED | sc.PATH_ONE_ROW} <= paths
    assert any(c.flat_run for c in sc.probe_cases())


@pytest.mark.parametrize("case", sc.probe_cases(), ids=lambda c: c.name)
def test_probe_eval_is_dir_to_uv_then_the_texel(oracle, case):
    hp = case.host_probe(oracle)
    d = sc.probe_directions(case.width, case.height)
    got = oracle.probe_eval(hp, d)
    assert np.array_equal(_bits(got["uv"]), _bits(oracle.probe_dir_to_uv(d)))
    uv = got["uv"]
    assert np.isfinite(uv).all() and uv.min() >= 0.0 and uv.max() <= 1.0
    px = np.clip((uv[:, 0] * np.float32(case.width)).astype(np.int32), 0, case.width - 1)
    py = np.clip((uv[:, 1] * np.float32(case.height)).astype(np.int32), 0, case.height - 1)
    assert np.array_equal(_bits(got["texel"]), _bits(hp.data[py, px]))
    assert (uv[:, 0] == 1.0).any() and (uv[:, 0] == 0.0).any() and (uv[:, 1] == 0.0).any() and (uv[:, 1] == 1.0).any()
    assert len(np.unique(py * case.width + px)) >= min(case.width * case.height, 50)


# ---- Disney BSDF ----------------------------------------------------------------------------------------------------------
def test_bsdf_table_given_extends_the_table(oracle):
    for name, mat, eta_i, eta_o, g, t in sc.bsdf_tables(oracle):
        n = sc.BSDF_ROWS
        old = oracle.bsdf_table(mat, g["N"], g["view"], g["albedo"], np.full(n, eta_i, np.float32), np.full(n, eta_o, np.float32), g["seeds"])
        for k in old:
            assert np.array_equal(old[k].view(np.uint32), t[k].view(np.uint32)), (name, eta_i, k)


def test_bsdf_given_columns_against_the_binary64_restatement(oracle):
    """eval_given / pdf_given against tests/disney_f64.py under the rule of test_bsdf_against_an_independent_binary64_restatement,
    unchanged: rows near a branch condition (disney_f64's `near` masks) or without a finite binary64 value are left out, at
    least half of a table's rows remain, and they agree within 2e-4 * max(1, 0.01 / max(0.001, roughness)^2), relative to the
    largest component (floor 1e-6).  That test takes its directions from BSDFSample; the rows here are chosen, so two more
    masks of the same kind apply, both stated in disney_f64.py: N.V within 1e-3 of 0, and N.H within the clearcoat lobe's
    width of its peak."""
    import disney_f64 as D
    checked = 0
    for name, mat, eta_i, eta_o, g, t in sc.bsdf_tables(oracle):
        Nn, Vv, L, alb = (g[k].astype(np.float64) for k in ("N", "view", "L_given", "albedo"))
        with np.errstate(all="ignore"):
            ev, near_e = D.bsdf_eval(mat, alb, eta_i, eta_o, Nn, Vv, L)
            pdf, near_p = D.bsdf_pdf(mat, eta_i, eta_o, Nn, Vv, L)
            near = near_e | near_p | D.near_grazing_view(Nn, Vv) | D.near_clearcoat_peak(mat, Nn, Vv, L)
        use = ~near & np.isfinite(ev).all(1) & np.isfinite(pdf)
        print("%-20s eta %.1f/%.1f: %d of %d rows compared" % (name, eta_i, eta_o, use.sum(), len(use)))
        assert use.sum() > 0.5 * len(use), (name, use.sum())
        scale = np.maximum(np.abs(ev[use]).max(1), 1e-6)
        tol = 2e-4 * max(1.0, 0.01 / max(0.001, mat.roughness) ** 2)
        e_err = (np.abs(t["eval_given"][use] - ev[use]).max(1) / scale).max()
        p_err = (np.abs(t["pdf_given"][use] - pdf[use]) / np.maximum(pdf[use], 1e-6)).max()
        assert e_err < tol and p_err < tol, (name, eta_i, eta_o, e_err, p_err, tol)
        checked += int(use.sum())
    assert checked > 100000


def test_bsdf_case_conditions(oracle):
    types, tir, below, grazing = set(), 0, 0, 0
    for name, mat, eta_i, eta_o, g, t in sc.bsdf_tables(oracle):
        types |= set(np.unique(t["type"][t["pdf"] > 0]).tolist())
        if mat.transmission > 0 and eta_i > eta_o:
            tir += int((t["pdf"] == 0).sum())
        ndl = (g["N"] * g["L_given"]).sum(1)
        below += int((ndl <= 0).sum())
        grazing += int((ndl == 0).sum())
        bad = ~(np.isfinite(t["light"]).all(1) & np.isfinite(t["pdf"]) & np.isfinite(t["eval"]).all(1) & np.isfinite(t["pdf_again"])
                & np.isfinite(t["eval_given"]).all(1) & np.isfinite(t["pdf_given"]))
        nan = np.isnan(t["light"]).any(1) | np.isnan(t["pdf"]) | np.isnan(t["eval"]).any(1) | np.isnan(t["pdf_again"]) | np.isnan(t["eval_given"]).any(1) | np.isnan(t["pdf_given"])
        print("%-20s eta %.1f/%.1f: NaN rows %.3f %%, non-finite rows %.3f %%" % (name, eta_i, eta_o, 100.0 * nan.mean(), 100.0 * bad.mean()))
        assert nan.mean() <= 0.01, (name, eta_i, eta_o, nan.mean())
    assert types == {0, 1, 2}, types               # eReflected, eTransmitted, eSpecular
    assert tir > 100 and below > 1000 and grazing > 100, (tir, below, grazing)
    g = sc.bsdf_tables(oracle)[0][4]
    ndv = (g["N"].astype(np.float64) * g["view"]).sum(1)
    assert (ndv == 0).any() and (ndv == 1).any() and ((ndv > 0) & (ndv < 2e-7)).any() and (ndv < 0).any()
    assert (np.abs(g["N"][:, 0]) == np.abs(g["N"][:, 1])).sum() > 100
    assert (g["L_given"] == -g["view"]).all(1).sum() > 100


# ---- tex2d -----------------------------------------------------------------------------------------------------------------
def _tex2d_f64(tex, uv):
    """Bilinear filtering with wrap addressing, normalized coordinates, texel centres at +0.5, RGBA8 as value / 255: binary64."""
    h, w = tex.shape
    x, y = uv[:, 0].astype(np.float64) * w - 0.5, uv[:, 1].astype(np.float64) * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    ix0, iy0 = np.mod(x0, w).astype(np.int64), np.mod(y0, h).astype(np.int64)
    ix1, iy1 = (ix0 + 1) % w, (iy0 + 1) % h

    def c(iy, ix):
        p = tex[iy, ix].astype(np.uint64)
        return np.stack([p & 255, (p >> 8) & 255, (p >> 16) & 255, p >> 24], 1).astype(np.float64) / 255.0
    return (1 - fx) * (1 - fy) * c(iy0, ix0) + fx * (1 - fy) * c(iy0, ix1) + (1 - fx) * fy * c(iy1, ix0) + fx * fy * c(iy1, ix1)


@pytest.mark.parametrize("k", range(len(sc.TEXTURE_SIZES)), ids=["%dx%d" % s for s in sc.TEXTURE_SIZES])
def test_tex2d_is_bilinear_wrap_addressing(oracle, k):
    """oracle.tex2d against the binary64 statement on every finite coordinate of the cases.

    The bound, per channel, with e = 2^-24 (the relative error of one binary32 rounding) and all values in [0, 1]:
      * the coordinate: x = fl(fl(u w) - 0.5) differs from u w - 0.5 by at most e (|u| w + |x|) <= e (2 |u| w + 1) texels, and
        the filtered value moves by at most one unit per texel of x and per texel of y (it is piecewise linear between texel
        values in [0, 1]); fx = x - floor(x) is exact;
      * a weight such as fl(fl(1 - fx) fl(1 - fy)) carries three roundings, the texel value c / 255 one, each product
        weight * value one more: at most 5 e of the product, and the four exact products sum to at most 1: 5 e;
      * the three additions of partial sums that stay below 1 + 5 e: 3 e.
    Together 8 e + e (2 |u| w + 2 |v| h + 2), taken as 10 e + 2 e (|u| w + |v| h).  Coordinates beyond 2^20 texels are left
    to the bit comparison with the device: there the bound says nothing (binary32 cannot hold their fraction, and the
    conversion to an integer saturates at 1e9), only that the result is a mixture of texel values."""
    tex = sc.textures()[k]
    h, w = tex.shape
    uv = sc.texture_coordinates(w, h)
    got = oracle.tex2d(tex, uv)
    finite = np.isfinite(uv).all(1)
    assert (~finite).sum() >= 10 and np.isnan(got[np.isinf(uv).any(1) | np.isnan(uv).any(1)]).all()
    assert np.isfinite(got[finite]).all() and got[finite].min() >= 0.0 and got[finite].max() <= 1.0 + 2.0 ** -22
    reach = np.abs(uv[:, 0].astype(np.float64)) * w + np.abs(uv[:, 1].astype(np.float64)) * h
    with np.errstate(invalid="ignore"):
        m = finite & (reach <= 2.0 ** 20)
    assert m.sum() > 3000 and (finite & ~m).sum() >= 10
    want = _tex2d_f64(tex, uv[m])
    e = 2.0 ** -24
    bound = (10 * e + 2 * e * reach[m])[:, None]
    err = np.abs(got[m] - want)
    print("tex2d %dx%d: %d coordinates, largest error %.3g (bound there %.3g)" % (w, h, m.sum(), err.max(), bound[np.unravel_index(err.argmax(), err.shape)[0], 0]))
    assert (err <= bound).all(), (uv[m][np.argwhere(err > bound)[:4, 0]])
    # texel centres give the texel, edges the mean of two
    centre = np.float32([[(i + 0.5) / w, (j + 0.5) / h] for j in range(h) for i in range(w)])
    px = tex.ravel().astype(np.uint64)
    texels = np.stack([px & 255, (px >> 8) & 255, (px >> 16) & 255, px >> 24], 1) / 255.0
    assert np.abs(oracle.tex2d(tex, centre) - texels).max() <= 10 * e + 4 * e
