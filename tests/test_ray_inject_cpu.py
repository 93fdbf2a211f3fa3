"""The injected-ray classes of ray_inject_support.py hold what they are for (no GPU): sizes, both sides of every threshold the
kernels decide on, mixed waves that really are mixed -- all by predicates on the rays themselves -- and, through the oracle,
that the rays reach the geometry; the oracle's two hooks reproduce ora_sample bit for bit; the entry checks its arguments."""
import ctypes as C

import numpy as np
import pytest

import ray_inject_support as S


@pytest.fixture(scope="module")
def cl():
    return S.classes()


def _dlen(r):
    with np.errstate(all="ignore"):
        return np.max(np.abs(r[:, 3:6]), axis=1)  # within a factor sqrt(3) of |d|, and never overflows


def test_layout_is_the_devices_job_order():
    # a wave is one 8x8 block of one sample; 64 waves cover the frame once, 64 lanes each
    ys, xs = np.mgrid[0:S.H, 0:S.W]
    wv, ln = S.wave_of(xs, ys), S.lane_of(xs, ys)
    assert sorted(np.unique(wv)) == list(range(64)) and np.all(np.bincount(wv.ravel()) == 64)
    for w in range(64):
        assert sorted(ln[wv == w]) == list(range(64))
        assert np.ptp(xs[wv == w]) == 7 and np.ptp(ys[wv == w]) == 7
    # job order of job_pixel (csrc/pt_kernels.h): tile, then the 16 sub-blocks row by row, then the lane row by row
    assert S.wave_of(0, 0) == 0 and S.wave_of(8, 0) == 1 and S.wave_of(0, 8) == 4 and S.wave_of(32, 0) == 16 and S.wave_of(0, 32) == 32
    assert S.lane_of(1, 0) == 1 and S.lane_of(0, 1) == 8 and S.lane_of(39, 47) == 63
    by_wave = np.arange(64 * 64 * 6, dtype=float).reshape(64, 64, 6)
    t = S.to_table(by_wave)
    assert np.array_equal(t[47 * S.W + 39], by_wave[S.wave_of(39, 47), 63])


def test_every_class_is_large_enough(cl):
    assert list(cl) == ["length", "components", "near geometry", "far origins", "incoherent", "mixed"]
    for name, r in cl.items():
        assert r.shape == (S.W * S.H, 6) and r.dtype == np.float64
        distinct = len({row.tobytes() for row in r})
        assert distinct >= 256, (name, distinct)
    assert S.indexing_rays().shape == (33 * 31 * 3, 6)
    for name in S.SCENE_NAMES:  # the bound the thresholds are stated for is the scenes' bound
        doc = S.scene_doc(name)
        assert S.scene_bound(doc) == S.BOUND, name
        kinds = {(o["type"], o["material_id"]) for o in doc["objects"]}
        assert {("sphere", "g"), ("box", "g"), ("sphere", "m"), ("sphere_light", "e"), ("plane", "d")} <= kinds, name
        assert sum(o["type"] == "plane" for o in doc["objects"]) == (2 if name == "two_planes" else 1)
    for name, (n_s, n_b) in S.SIZE_CLASSES.items():
        objs = S.scene_doc(name)["objects"]
        assert sum(o["type"] in ("sphere", "sphere_light") for o in objs) == n_s and sum(o["type"] == "box" for o in objs) == n_b


def test_length_class_straddles_every_window(cl):
    r = cl["length"]
    a, fa, n = S.dir_a(r), S.dir_fa(r), _dlen(r)
    assert np.all(S.is_finite(r)) and not np.any(S.beyond_clip(r))
    with np.errstate(all="ignore"):
        f32 = np.abs(r[:, 3:6].astype(np.float32)).max(axis=1)
    sides = {
        "fa trust low": (fa > 1e-30, fa <= 1e-30), "fa trust high": (fa < 1e30, fa >= 1e30),
        "tame low": (a >= 1e-100, a < 1e-100), "tame high": (a <= 1e100, a > 1e100),
        "FLT_MAX": (np.isinf(f32), np.isfinite(f32)),                       # (float)d overflows / does not
        "FLT_MIN": (f32 >= S.FLT_MIN, (f32 < S.FLT_MIN) & (f32 > 0)),       # normal / subnormal in FP32
        "FP32 subnormal": (f32 > 0, f32 == 0),                              # (float)d survives / flushes to zero
        "a overflows": (np.isinf(a), np.isfinite(a)),
        "a underflows": (a >= 2.0 ** -1022, a < 2.0 ** -1022),
    }
    for name, length in S.LENGTHS.items():
        near = (n >= length / 4) & (n <= length * 4)       # +-1 binade of |d| (its largest component is within sqrt(3) of it)
        tight = (n >= length * (1 - 1e-12) / np.sqrt(3)) & (n <= length * (1 + 1e-12))  # the +-3 ulp rays (and nothing a binade off)
        assert np.count_nonzero(tight) >= 7 * 20, (name, np.count_nonzero(tight))
        one, other = sides[name]
        assert np.any(one & near) and np.any(other & near), (name, np.count_nonzero(one & near), np.count_nonzero(other & near))
    # +-3 ulps of the exact threshold: axis-parallel rays of length float(s) give a = s*s, on either side of 1e-100 and 1e100
    axis = np.count_nonzero(r[:, 3:6], axis=1) == 1
    for lim in (1e-100, 1e100):
        with np.errstate(all="ignore"):
            at = axis & (np.abs(a / lim - 1) < 1e-14)
        assert np.any(a[at] < lim) and np.any(a[at] > lim), lim
    # the sweep: every binade 2^k, k in [-600, 600], down to a = 0 and up to a = inf
    exps = np.unique(np.floor(np.log2(np.linalg.norm(r[:, 3:6] * 2.0 ** -np.floor(np.log2(n))[:, None], axis=1)) + np.floor(np.log2(n))))
    assert exps.min() <= -600 and exps.max() >= 599 and len(exps) >= 1150
    assert np.any(a == 0) and np.any(np.isinf(a))
    assert np.count_nonzero(S.is_tame(r) & ~S.is_trusted_length(r)) >= 256  # tame but untrusted: must keep every candidate


def test_component_class_has_its_special_directions(cl):
    r = cl["components"]
    d = r[:, 3:6]
    assert np.all(S.is_finite(r))
    assert np.count_nonzero((d == 0) & ~np.signbit(d)) >= 300 and np.count_nonzero((d == 0) & np.signbit(d)) >= 300  # +0 and -0
    sub = (d != 0) & (np.abs(d) < 2.0 ** -1022)
    assert np.count_nonzero(sub & (d > 0)) >= 300 and np.count_nonzero(sub & (d < 0)) >= 100
    with np.errstate(all="ignore"):
        srt = np.sort(np.abs(d), axis=1)
        big = (srt[:, 1] > 0) & (srt[:, 2] == srt[:, 1] * 2.0 ** 60)
        small = (srt[:, 0] > 2.0 ** -1022) & (srt[:, 0] == srt[:, 2] * 2.0 ** -60)
    assert np.count_nonzero(big) >= 300 and np.count_nonzero(small) >= 100
    axis = np.count_nonzero(d, axis=1) == 1
    assert np.count_nonzero(axis) >= 256
    on_face = np.zeros(len(r), bool)  # axis-parallel AND the origin exactly in a probe box's face plane, moving inside that plane
    for lo, hi in S.BOXES:
        for k in range(3):
            on_face |= axis & (d[:, k] == 0) & ((r[:, k] == lo[k]) | (r[:, k] == hi[k]))
    assert np.count_nonzero(on_face) >= 128
    assert np.count_nonzero(axis & (r[:, 1] == 0) & (d[:, 1] == 0)) >= 30  # in the floor plane


def test_near_geometry_class_sits_on_the_surfaces(cl):
    r = cl["near geometry"]
    o = r[:, 0:3]
    assert np.all(S.is_finite(r)) and np.all(S.is_tame(r)) and not np.any(S.beyond_clip(r))
    for c, rad in S.SPHERES:
        dist = np.linalg.norm(o - c, axis=1)
        assert np.count_nonzero(np.abs(dist - rad) <= 8 * np.spacing(rad + np.abs(c).max())) >= 30          # on it, +-4 ulps
        for off in (S.TMIN / 2, S.TMIN, 2 * S.TMIN):
            for sgn in (1, -1):
                assert np.count_nonzero(np.abs(dist - (rad + sgn * off)) < 1e-12) >= 3, (rad, off, sgn)
    for lo, hi in S.BOXES[:2]:
        inb = np.all((o >= lo - 1e-9) & (o <= hi + 1e-9), axis=1)
        on = [(o[:, k] == lo[k]) | (o[:, k] == hi[k]) for k in range(3)]
        count = on[0].astype(int) + on[1] + on[2]
        assert np.count_nonzero(inb & (count == 1)) >= 12 and np.count_nonzero(inb & (count == 2)) >= 12 and np.count_nonzero(inb & (count == 3)) >= 12
        for k in range(3):  # 1 and 4 ulps off a face, either side
            for face in (lo[k], hi[k]):
                for u in (1, 4):
                    assert np.any(o[:, k] == S.ulps(face, u)) and np.any(o[:, k] == S.ulps(face, -u)), (face, u)
    assert np.count_nonzero(o[:, 1] == 0) >= 30 and np.any(o[:, 1] == S.ulps(0.0, 1)) and np.any(o[:, 1] == S.ulps(0.0, -4))
    for off in (S.TMIN / 2, S.TMIN, 2 * S.TMIN):
        assert np.any(o[:, 1] == off) and np.any(o[:, 1] == -off)
    assert np.count_nonzero(S.inside_glass(r)) >= 256
    assert np.count_nonzero(S.in_shell(r)) >= 256


def test_far_class_straddles_every_bound(cl):
    r = cl["far origins"]
    fin = S.is_finite(r)
    om = S.omax(r)
    with np.errstate(all="ignore"):
        towards = np.einsum("ij,ij->i", r[:, 0:3], r[:, 3:6]) < 0
    for base in (S.BOUND, S.CLIP_BOUND, S.ORIGIN_BOUND):
        for lo, hi in ((0.9, 0.99), (1.01, 1.1)):
            band = fin & (om >= lo * base) & (om <= hi * base)
            assert np.count_nonzero(band & towards) >= 40 and np.count_nonzero(band & ~towards) >= 10, (base, lo)
        assert np.any(om == base)
    assert np.any(S.beyond_clip(r) & fin) and np.any(~S.beyond_clip(r) & fin)
    assert np.any(S.beyond_origin_bound(r) & ~S.is_far(r) & fin)
    rc = S.reach(r)
    for lo, hi in ((0.9, 0.99), (1.01, 1.1)):
        band = fin & S.beyond_clip(r) & (rc >= lo * S.FAR_REACH) & (rc <= hi * S.FAR_REACH)
        assert np.count_nonzero(band & towards) >= 40 and np.count_nonzero(band & ~towards) >= 10, lo
        assert np.all(S.is_far(r[band]) == (lo > 1))
    for k in range(-3, 4):  # the tame limit, +-3 ulps
        assert np.count_nonzero(om == S.ulps(1e100, k)) >= 4, k
    assert np.any(fin & (om > 1e100) & towards) and np.any(fin & (om > 1e100) & ~towards)
    assert np.any(fin & (om == 1e100)) and np.any(S.is_tame(r) & (om > 1e99)) and np.any(~S.is_tame(r) & fin)
    for part in (slice(0, 3), slice(3, 6)):  # non-finite values in one component and in all three, origin and direction
        for test in (np.isnan, lambda v: np.isinf(v) & (v > 0), lambda v: np.isinf(v) & (v < 0)):
            cnt = np.count_nonzero(test(r[:, part]), axis=1)
            assert np.any(cnt == 1) and np.any(cnt == 3)
    assert np.count_nonzero(~fin) >= 96


def test_mixed_waves_are_mixed(cl):
    r = cl["mixed"]
    odd = S.is_odd(r)
    wv = S.waves_of_table(r)
    ys, xs = np.mgrid[0:S.H, 0:S.W]
    lane = S.lane_of(xs, ys).reshape(-1)
    by_wave, kinds = S.class_mixed()
    single, halves = {}, {}
    for w in range(S.NWAVES):
        lanes = np.sort(lane[(wv == w) & odd])
        assert 0 < len(lanes) < 64, (w, len(lanes))  # some lane switches the wave, and some lane pays for it
        assert np.array_equal(odd[wv == w][np.argsort(lane[wv == w])], S.is_odd(by_wave[w]))  # the layout kept lane and wave
        if len(lanes) == 1:
            single.setdefault(kinds[w], set()).add(int(lanes[0]))
        else:
            assert len(lanes) == 32 and (np.array_equal(lanes, np.arange(32)) or np.array_equal(lanes, np.arange(32, 64))), w
            halves.setdefault(kinds[w], set()).add(int(lanes[0]))
    assert set(single) == set(S.ODD_KINDS) and all(v == {0, 31, 32, 63} for v in single.values()), single
    assert set(halves) == set(S.ODD_KINDS) and {0, 32} <= set().union(*halves.values()), halves
    # each odd kind is what it says, on the inputs
    rng = np.random.default_rng(1)
    for kind in S.ODD_KINDS:
        q = np.array([S.odd_ray(rng, kind) for _ in range(32)])
        want = {"nan": np.isnan(q).any(axis=1), "inf": np.isinf(q).any(axis=1), "beyond tame": S.is_finite(q) & ~S.is_tame(q) & (S.omax(q) > 1e100),
                "beyond far": S.is_finite(q) & S.is_far(q) & S.is_tame(q), "beyond clip": S.is_finite(q) & S.beyond_clip(q) & ~S.is_far(q),
                "untrusted length": S.is_finite(q) & S.is_tame(q) & ~S.is_trusted_length(q) & ~S.beyond_clip(q)}[kind]
        assert np.all(want), kind
    # and the incoherent class is ordinary throughout: no lane of it switches anything
    assert not np.any(S.is_odd(cl["incoherent"]))
    inc = cl["incoherent"]
    assert np.all(np.abs(inc[:, 0:3]) <= S.BOUND) and np.allclose(np.linalg.norm(inc[:, 3:6], axis=1), 1.0)
    assert np.all(np.abs(np.mean(inc[:, 3:6], axis=0)) < 0.05)  # directions all over the sphere


def test_oracle_hooks_reproduce_the_sample(oracle):
    doc = S.scene_doc("bitmask")
    for cam in (S.CAMERA, dict(S.CAMERA, aperture=0.3, focus_dist=9.0)):  # pinhole: two camera draws; thin lens: more
        osc = oracle.Scene(dict(doc, camera=cam))
        w, h, spp = 33, 31, 3
        draws = set()
        for (x, y, s) in [(0, 0, 0), (32, 30, 2), (16, 15, 1), (5, 29, 0), (31, 2, 2), (20, 20, 1), (9, 11, 2), (1, 30, 0)]:
            o, d = oracle.primary_ray(osc, w, h, spp, S.DEPTH, S.SEED, x, y, s)
            ref = oracle.sample(osc, w, h, spp, S.DEPTH, S.SEED, x, y, s)
            got = oracle.sample_ray(osc, w, h, spp, S.DEPTH, S.SEED, x, y, s, o, d)
            assert [float.hex(v) for v in got[0]] == [float.hex(v) for v in ref[0]] and got[1:] == ref[1:], (x, y, s)
            # another ray from the same (pixel, sample): the camera draws are still counted
            other = oracle.sample_ray(osc, w, h, spp, 0, S.SEED, x, y, s, [0, 50, 0], [0, 1, 0])
            draws.add(other[2])
            assert other[0] == [0.0, 0.0, 0.0] and other[1] == 0
        assert (draws == {2}) == (cam["aperture"] == 0) and min(draws) >= 2
    # the whole frame through the batch form is ora_render's frame, bit for bit
    osc = oracle.Scene(doc)
    w, h, spp = 33, 31, 3
    rays = np.array([sum(oracle.primary_ray(osc, w, h, spp, S.DEPTH, S.SEED, x, y, s), [])
                     for y in range(h) for x in range(w) for s in range(spp)])
    o = S.oracle_frame(oracle, doc, rays, w, h, spp)
    ref = oracle.render(osc, w, h, spp, S.DEPTH, seed=S.SEED)
    assert np.array_equal(o["accum"], ref["accum"], equal_nan=True) and np.array_equal(o["rgba"], ref["rgba"])
    assert np.array_equal(o["nseg"], ref["nseg"]) and np.array_equal(o["ndraw"], ref["ndraw"])
    assert int(o["nseg"].sum()) == ref["stats"]["segments"] and int(o["ndraw"].sum()) == ref["stats"]["draws"]


def test_classes_reach_what_they_are_for(oracle, cl):
    """Through the oracle's own loop: the finite rays of the aimed classes and of the incoherent one hit spheres, boxes, glass
    and the plane, and miss; the creeping origins start paths that stay inside glass; the far rays that look at the scene find
    it and those that look away do not."""
    doc = S.scene_doc("bitmask")
    for name in ("length", "components", "near geometry", "incoherent"):
        r = cl[name]
        ids = S.first_hits(oracle, doc, r)
        kind, glass = S.hit_kinds(doc, ids)
        fin = S.is_finite(r) & (S.dir_a(r) > 0) & np.isfinite(S.dir_a(r))
        for k in ("sphere", "box", "plane", "miss"):
            # (a plane answers only while |n.d| >= 1e-6 and t = .../(n.d) >= tMin, objects.go:103-110: with |d| swept over 1200
            # binades that leaves the few rays of the length class whose |d| is between 1e-6 and 1e3)
            floor = 1 if (name, k) == ("length", "plane") else 64
            assert np.count_nonzero(fin & (kind == k)) >= floor, (name, k, np.count_nonzero(fin & (kind == k)))
        assert np.count_nonzero(fin & glass) >= 64, name
    r = cl["near geometry"]
    ids = S.first_hits(oracle, doc, r)
    _, glass = S.hit_kinds(doc, ids)
    inside = S.inside_glass(r) & ~S.in_shell(r)
    assert np.count_nonzero(inside & glass) >= 256  # from inside glass the first hit is glass again (origins ON a face may leave)
    o = S.oracle_frame(oracle, doc, r, key=("bitmask", "near geometry"))
    nseg = o["nseg"].reshape(-1)
    assert np.count_nonzero(nseg[inside] >= 4) >= 32 and nseg.max() == S.DEPTH  # long paths: bounce after bounce in the glass
    r = cl["far origins"]
    ids = S.first_hits(oracle, doc, r)
    fin = S.is_finite(r) & S.is_tame(r)
    with np.errstate(all="ignore"):
        towards = np.einsum("ij,ij->i", r[:, 0:3], r[:, 3:6]) < 0
    out = fin & S.beyond_clip(r)
    assert np.count_nonzero(out & towards & (ids >= 0)) >= 256 and np.count_nonzero(out & ~towards & (ids < 0)) >= 64
    assert np.count_nonzero(S.is_far(r) & fin & (ids >= 0)) >= 64  # even from 2000 scene sizes out


def test_named_rays_pass_beside_objects_before_their_hit(oracle):
    """The named case is what it is kept for: exactly axis-parallel rays that hit a sphere or a box of the hierarchy's scene only
    after passing beside at least 20 other objects, clear of their inflated bounds."""
    doc = S.scene_doc("bvh")
    rays = np.array(S.NAMED_RAYS["beside a core"], float)
    ids = S.first_hits(oracle, doc, rays)
    for r, i in zip(rays, ids):
        assert i >= 0 and doc["objects"][i]["type"] != "plane", (r, i)
        assert S.beside_cores(doc, r, int(i)) >= 20, (r, i)
    assert len({int(np.argmax(np.abs(r[3:6]))) for r in rays}) == 3  # along every axis
    assert len(S.named_table("beside a core")) == S.W * S.H


def test_argument_checks_need_no_device():
    from path_trace_golang_amd import build, capi

    build.build_core()
    L = capi.load()
    assert capi.has("pt_debug_set_primary_rays")
    rays = (C.c_double * 12)()
    assert L.pt_debug_set_primary_rays(None, rays, 2) == capi.PT_ERR_INVALID
    assert b"ctx is null" in L.pt_last_error()
    assert L.pt_debug_set_primary_rays(None, None, 0) == capi.PT_ERR_INVALID  # clearing needs a context too
    assert L.pt_debug_set_primary_rays(None, rays, -1) == capi.PT_ERR_INVALID
    with pytest.raises(ValueError):  # the binding refuses a table that is not [n][6] before it reaches the library
        capi.Context.set_primary_rays(object.__new__(capi.Context), np.zeros((4, 5)))
