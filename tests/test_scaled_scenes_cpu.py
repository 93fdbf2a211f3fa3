"""The rescaled scenes and ray tables of scaled_scene_support.py are what they claim (no GPU; the oracle only).  Without this the GPU
tests of test_scaled_scenes_gpu.py could pass on rays that hit nothing.

Findings about the reference's own arithmetic, each asserted below as it is:
  * The plane's |n.d| >= 1e-6 (objects.go:103) is the one absolute test on a direction.  In the similar family n.d scales with
    2^k: from k = -40 down no ray of any table reaches the floor, and from k = 60 up the flat rays of "components" (one component
    2^-60 of the others) gain it.  The anchor takes that rule into account instead of dropping a row (similar_expectation).
  * Rows of "far origins" and "mixed" with a component of 1e100 (the tame limit) times 2^k, similar family, k >= 90: b b and a c of
    objects.go:46 exceed DBL_MAX and the discriminant is NaN.  216 and 104 rows, named by overflows_in_fp64 from the inputs.
  * Subnormal direction and origin components (5e-324, 2^-1060, 2^-1030; the origins 1 and 4 ulps off y = 0) times 2^k < 1 are
    rounded: those rows are not 2^k times the original, named by underflows_in_fp64.
  * "trusted for k <= 49" of the similar family holds from k = -49 up only: 4^-50 < 1e-30, and at k = -140 the FP32 square is 0."""
import numpy as np
import pytest

import ray_inject_support as S
import scaled_scene_support as X


def test_scales_and_bands():
    assert X.K == (-140, -40, -4, -3, 40, 60, 61, 64, 90, 96, 97, 119, 120, 130) and X.TABLES == tuple(t for t in
        ("near geometry", "incoherent", "far origins", "mixed", "components")) and "length" not in X.TABLES
    want = {-140: "floor", -40: "floor", -4: "floor", -3: "ordinary", 40: "ordinary", 60: "ordinary", 61: "fp32 squares overflow",
            64: "fp32 squares overflow", 90: "fp32 squares overflow", 96: "fp32 squares overflow", 97: "keep all", 119: "keep all",
            120: "plain loop", 130: "plain loop"}
    assert {k: X.band(k) for k in X.K} == want and set(want.values()) == set(X.BANDS)
    # the thresholds, restated: either side of each
    f32 = np.float32
    with np.errstate(over="ignore"):
        assert np.isfinite(f32(X.coordinate(60)) * f32(X.coordinate(60))) and np.isinf(f32(X.coordinate(61)) * f32(X.coordinate(61)))
        # rm2 = (r + m)^2 at k = 64: infinite for the spheres of radius 1.5 and 1, finite for 0.25 (m = 8 / 4096)
        rm2 = lambda r: f32((r + 8.0 / 4096.0) * 2.0 ** 64) * f32((r + 8.0 / 4096.0) * 2.0 ** 64)  # noqa: E731
        assert np.isinf(rm2(1.5)) and np.isinf(rm2(1.0)) and np.isfinite(rm2(0.25)) and np.isfinite(rm2(0.75))
        assert all(np.isinf(f32((r + 8.0 / 4096.0) * 2.0 ** 90) ** 2) for r in (0.25, 0.5, 0.75, 1.0, 1.5))
    assert X.coordinate(96) < 1e30 <= X.coordinate(97) and X.coordinate(119) < 1e37 <= X.coordinate(120)
    assert X.coordinate(130) > S.FLT_MAX and X.coordinate(-4) == 0.5 and X.coordinate(-3) == 1.0
    assert 0 < X.coordinate(-140) < S.FLT_MIN and float(f32(X.coordinate(-140))) == X.coordinate(-140)  # an FP32 denormal, exactly
    assert X.bound(-140) == X.bound(-4) == X.bound(-3) == 1.0 and X.bound(96) == 8 * 2.0 ** 96 and np.isinf(X.bound(97))
    assert (1.0 / 4096.0) / X.coordinate(-140) > 4e37  # margin / scene


@pytest.mark.parametrize("scene_name", X.SCENES)
def test_scene_bound_of_every_scaled_scene(scene_name):
    doc = S.scene_doc(scene_name)
    for k in X.K:
        d = X.scaled_doc(doc, k)
        assert S.scene_bound(d) == (8 * 2.0 ** k if X.band(k) != "floor" else 1.0), k
        assert d["materials"] == doc["materials"] and d["sky"] == doc["sky"]
        cam, c0 = d["camera"], doc["camera"]
        assert (cam["fov"], cam["up"]) == (c0["fov"], c0["up"]) and cam["position"]["z"] == 12 * 2.0 ** k and cam["target"]["y"] == 2 * 2.0 ** k
        for o, o0 in zip(d["objects"], doc["objects"]):  # exact: dividing gives the original back
            assert all(o[key][c] * 2.0 ** -k == o0[key][c] for key in ("position", "size") for c in "xyz"), (k, o0)
            assert (o["type"], o["material_id"]) == (o0["type"], o0["material_id"])
    assert doc == S.scene_doc(scene_name)  # the base document is not touched
    thin = X.scaled_doc(dict(doc, camera=dict(S.CAMERA, aperture=0.25, focus_dist=9.0)), 3)["camera"]
    assert (thin["aperture"], thin["focus_dist"]) == (2.0, 72.0)


def test_scaled_rays_scale_what_the_family_says():
    t = S.classes()["incoherent"]
    for k in (-140, 61, 130):
        sim, unit = X.scaled_rays(t, k, "similar"), X.scaled_rays(t, k, "unit")
        assert np.array_equal(sim * 2.0 ** -k, t) and np.array_equal(unit[:, 0:3], sim[:, 0:3]) and np.array_equal(unit[:, 3:6], t[:, 3:6])
    assert X.families(-4) == ("similar", "unit") and X.families(-40) == ("similar",)
    with pytest.raises(AssertionError):
        X.scaled_rays(t, 1, "other")


@pytest.mark.parametrize("scene_name", X.SCENES)
def test_similar_rays_hit_what_they_hit_unscaled(oracle, scene_name):
    """The similarity anchor: at all 14 scales and on all five tables the oracle's first hits of the similar family are those of
    k = 0, id for id (similar_expectation says how the plane's absolute test enters, and which rows are excused)."""
    plane = [i for i, o in enumerate(S.scene_doc(scene_name)["objects"]) if o["type"] == "plane"]
    assert len(plane) == 1
    for table_name in X.TABLES:
        tab = S.classes()[table_name]
        for k in X.K:
            ids = S.first_hits(oracle, X.doc_of(scene_name, k), X.rays_of(table_name, k, "similar"))
            want, exact, gained = X.similar_expectation(oracle, scene_name, table_name, k)
            bad = np.flatnonzero(exact & ~gained & (ids != want))
            assert len(bad) == 0, (table_name, k, bad[:8].tolist(), ids[bad[:8]].tolist(), want[bad[:8]].tolist())
            with np.errstate(all="ignore"):
                t_plane = -tab[:, 1] / tab[:, 4]  # (p_y - o_y) / d_y with p_y = 0, the same at every scale
            ok = (ids == want) | ((ids == plane[0]) & (t_plane >= S.TMIN))
            bad = np.flatnonzero(exact & gained & ~ok)
            assert len(bad) == 0, (table_name, k, "plane gained", bad[:8].tolist())
            # what is excused is what the header names, and nothing at the scales in between
            excused = int(np.count_nonzero(S.is_finite(tab) & ~exact))
            over = int(np.count_nonzero(X.overflows_in_fp64(tab, k, "similar")))
            assert over == ({"far origins": 216, "mixed": 104}.get(table_name, 0) if k >= 90 else 0), (table_name, k, over)
            if k > 0:
                assert excused == over and (table_name != "components" or k < 60 or int(np.count_nonzero(gained)) >= 120), (table_name, k)  # one flat-in-y ray per base ray
            else:
                assert excused == over + int(np.count_nonzero(X.underflows_in_fp64(tab, k, "similar")))
                assert (excused > 0) == (table_name in ("components", "near geometry")) and excused < 1900, (table_name, k, excused)


@pytest.mark.parametrize("scene_name", X.SCENES)
def test_conditions_per_table_family_and_scale(oracle, scene_name):
    """First segments reach the geometry and miss it; trust is what the family says; scaling adds no row with a NaN or an infinity
    in the oracle's answer; every table keeps its 4096 rows."""
    base_doc = S.scene_doc(scene_name)
    for table_name in X.TABLES:
        tab = S.classes()[table_name]
        nf0 = X.nonfinite_rows(oracle, base_doc, tab)
        fin = S.is_finite(tab)
        for k in X.K:
            doc = X.doc_of(scene_name, k)
            for family in X.families(k):
                r = X.rays_of(table_name, k, family)
                tag = (scene_name, table_name, family, k)
                assert r.shape == (S.W * S.H, 6) and np.array_equal(S.is_finite(r), fin), tag  # no ray skipped, none made non-finite
                ids = S.first_hits(oracle, doc, r)
                hits = int(np.count_nonzero(fin & (ids >= 0)))
                assert 0 < hits < len(r), (tag, hits)
                assert 0 < int(np.count_nonzero(fin & (ids < 0))), tag
                assert X.nonfinite_rows(oracle, doc, r) == nf0, (tag, nf0)
                if table_name == "incoherent":
                    trusted = X.is_trusted(r, k)
                    if family == "unit":
                        assert np.all(S.is_trusted_length(r)) and np.all(S.omax(r) <= 4.0 * max(X.coordinate(k), 1.0)), tag
                        # the kernels' own form (FP32 origins against origin_bound <= 3e38) agrees wherever a culled scan runs:
                        # at k = 130 the FP32 origins are infinite, and the world is on the plain loop
                        assert np.all(trusted) or k == 130, tag
                    else:
                        assert np.all(trusted) if X.similar_trusted(k) else not np.any(trusted), tag
    assert [k for k in X.K if X.similar_trusted(k)] == [-40, -4, -3, 40] and X.similar_trusted(49) and not X.similar_trusted(50)
    assert X.similar_trusted(-49) and not X.similar_trusted(-50)


def test_far_origins_straddle_the_scaled_bounds():
    """Where B scales with the scene the scaled "far origins" table has rays on both sides of 3.5 B, 4 B and 2034.5 B in either
    family; at the floor and in the keep-all band the counts say what the restated predicates see instead."""
    tab = S.classes()["far origins"]
    base = X.far_sides(tab, 0)
    assert all(a > 100 and b > 100 for a, b in base.values()), base
    for k in X.K:
        for family in X.families(k):
            sides = X.far_sides(X.rays_of("far origins", k, family), k)
            line = "scaled scenes: far origins, %-7s k %4d [%s]: inside / beyond 3.5B %d / %d, 4B %d / %d, near / far of 2034.5B %d / %d" % (
                (family, k, X.band(k)) + sides["3.5B"] + sides["4B"] + sides["2034.5B"])
            print(line)
            if X.band(k) in ("ordinary", "fp32 squares overflow"):
                # the origins scale with B: the same rows on the same sides ("similar" keeps reach / B too; "unit" keeps |o| only)
                assert sides["3.5B"] == base["3.5B"] and sides["4B"] == base["4B"], (k, family, sides)
                assert all(a > 100 and b > 100 for a, b in sides.values()), (k, family, sides)
                if family == "similar":
                    assert sides == base, (k, family, sides)
            elif X.band(k) == "keep all":
                assert sides["3.5B"][1] == sides["4B"][1] == sides["2034.5B"][1] == 0, (k, sides)  # nothing is beyond infinity
            elif X.band(k) == "floor":
                assert sides["3.5B"][0] >= base["3.5B"][0] and sides["4B"][0] >= base["4B"][0], (k, sides)  # B = 1 stays, the origins shrink
