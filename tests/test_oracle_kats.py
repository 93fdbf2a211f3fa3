"""Known-answer tests that pin the CPU oracle (oracle/pt_oracle.c).

The reference ships no tests or vectors, so these are hand-derived from the
Go source: each case states the file:line whose behaviour it checks.  CPU only.
"""
import ctypes as C
import math
import struct

import numpy as np
import pytest

from conftest import scene_path

MAXF = 1.7976931348623157e308


def _ulps(a, b):
    ia = struct.unpack("<q", struct.pack("<d", a))[0]
    ib = struct.unpack("<q", struct.pack("<d", b))[0]
    return abs(ia - ib)


# ----------------------------------------------------------------- math restatements

def test_trig_matches_libm_within_2ulp(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(7)
    for x in rng.uniform(0.0, 2 * math.pi, 20000):
        s, c = math.sin(x), math.cos(x)
        if abs(s) > 1e-3:
            assert _ulps(L.ora_sin(x), s) <= 2
        if abs(c) > 1e-3:
            assert _ulps(L.ora_cos(x), c) <= 2
    for x in rng.uniform(0.01, 1.55, 20000):
        assert _ulps(L.ora_tan(x), math.tan(x)) <= 2
    for x in rng.uniform(-40.0, 0.0, 20000):
        assert _ulps(L.ora_exp(x), math.exp(x)) <= 1
    assert L.ora_sin(0.0) == 0.0 and L.ora_cos(0.0) == 1.0 and L.ora_exp(0.0) == 1.0


def test_cephes_constants_bit_patterns(oracle):
    # Go src/math/sin.go lists both decimal and hex; the decimals used in the oracle must parse to these
    want = {7.85398125648498535156e-1: 0x3FE921FB40000000, 3.77489470793079817668e-8: 0x3E64442D00000000,
            2.69515142907905952645e-15: 0x3CE8469898CC5170, 1.58962301576546568060e-10: 0x3DE5D8FD1FD19CCD,
            -1.66666666666666307295e-1: 0xBFC5555555555548, 4.16666666666665929218e-2: 0x3FA555555555554B,
            -1.13585365213876817300e-11: 0xBDA8FA49A0861A9B}
    for v, bits in want.items():
        assert struct.unpack("<Q", struct.pack("<d", v))[0] == bits


def test_pow5_is_go_repeated_squaring(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(3)
    for x in list(rng.uniform(0.0, 2.0, 5000)) + [0.0, 1.0, 2.0 ** -53, 1e-30]:
        x = float(x)
        assert L.ora_pow(x, 5.0) == x * ((x * x) * (x * x))  # materials.go:230 via pow.go's yi loop


def test_go_min_max_special_cases(oracle):
    L = oracle.lib()
    nan, inf = float("nan"), float("inf")
    assert math.isnan(L.ora_min(nan, 1.0)) and math.isnan(L.ora_max(1.0, nan))
    assert L.ora_min(-inf, nan) == -inf and L.ora_max(nan, inf) == inf
    assert math.copysign(1.0, L.ora_min(0.0, -0.0)) == -1.0
    assert math.copysign(1.0, L.ora_max(-0.0, 0.0)) == 1.0
    assert L.ora_min(2.0, 1.0) == 1.0 and L.ora_max(2.0, 1.0) == 2.0


def test_stream_contract(oracle):
    L = oracle.lib()
    st = C.c_uint64(L.ora_stream_init(1, 0, 0))
    xs = [L.ora_stream_next(C.byref(st)) for _ in range(20000)]
    assert all(0.0 <= x < 1.0 for x in xs)
    assert all((x * 2.0 ** 53) == int(x * 2.0 ** 53) for x in xs)  # 53-bit grid, random.go:27-34
    assert abs(np.mean(xs) - 0.5) < 0.01 and abs(np.var(xs) - 1 / 12) < 0.005
    # streams are keyed by (seed, pixel, sample)
    keys = {L.ora_stream_init(s, p, k) for s in (1, 2) for p in range(50) for k in range(50)}
    assert len(keys) == 2 * 50 * 50
    # MWC64X known answers from an independent restatement (Python integers): the state after a draw and the draw itself
    A = 4294883355
    for start in (0x0000000100000001, 0x7fffffff_ffffffff, 0x12345678_9abcdef0):
        x, c = start & 0xffffffff, start >> 32
        outs = []
        for _ in range(2):
            outs.append(x ^ c)
            t = x * A + c
            x, c = t & 0xffffffff, t >> 32
        s0 = C.c_uint64(start)
        got = L.ora_stream_next(C.byref(s0))
        assert s0.value == (c << 32) | x
        assert got == ((outs[0] << 21) | (outs[1] >> 11)) / 2.0 ** 53
    # the carry of a fresh stream is in [1, 2^31]: never a fixed point of the generator ((0, 0) would draw 0.0 for ever and
    # hang the rejection loops of math.go:74-84)
    for s in (1, 2, 3):
        for p in (0, 1, 2 ** 28 - 1):
            for k in (0, 1, 2 ** 31 - 1):
                assert 1 <= (L.ora_stream_init(s, p, k) >> 32) <= 2 ** 31


def test_stream_quality(oracle):
    """The stream is this package's own definition (the reference seeds from the clock): check what the renderer relies on.
    Many short streams keyed by neighbouring (pixel, sample), as a frame uses them: every draw position uniform, consecutive
    draws (the (u, v), (r1, r2) and rejection-triple draws) jointly uniform, same position of neighbouring samples
    jointly uniform.  z-scores of chi-square statistics; a defective generator gives tens to thousands."""
    L = oracle.lib()
    nd, npix, ns = 8, 600, 32
    d = np.empty((npix * ns, nd))
    i = 0
    for p in range(npix):
        for k in range(ns):
            st = C.c_uint64(L.ora_stream_init(7, 1000 + p, k))
            for j in range(nd):
                d[i, j] = L.ora_stream_next(C.byref(st))
            i += 1
    n = d.shape[0]

    def z(counts):
        nb = counts.size
        e = counts.sum() / nb
        return (((counts - e) ** 2 / e).sum() - (nb - 1)) / math.sqrt(2.0 * (nb - 1))

    for j in range(nd):
        assert abs(z(np.bincount((d[:, j] * 64).astype(int), minlength=64))) < 5
        assert abs(d[:, j].mean() - 0.5) < 4 / math.sqrt(12 * n)
    for j in range(nd - 1):
        cell = (d[:, j] * 16).astype(int) * 16 + (d[:, j + 1] * 16).astype(int)
        assert abs(z(np.bincount(cell, minlength=256))) < 5
        assert abs(np.corrcoef(d[:, j], d[:, j + 1])[0, 1]) < 5 / math.sqrt(n)
    for j in range(nd - 2):
        cell = ((d[:, j] * 8).astype(int) * 8 + (d[:, j + 1] * 8).astype(int)) * 8 + (d[:, j + 2] * 8).astype(int)
        assert abs(z(np.bincount(cell, minlength=512))) < 5
    nxt = d.reshape(npix, ns, nd)
    for j in range(nd):  # sample k against sample k + 1 of the same pixel
        a, b = nxt[:, :-1, j].ravel(), nxt[:, 1:, j].ravel()
        assert abs(z(np.bincount((a * 16).astype(int) * 16 + (b * 16).astype(int), minlength=256))) < 5
    # the low bits of the 53-bit grid come from the second generator step
    low = (d[:, 0] * 2.0 ** 53).astype(np.uint64) & np.uint64(255)
    assert abs(z(np.bincount(low.astype(int), minlength=256))) < 5


# ----------------------------------------------------------------- primitives (objects.go)

def test_box_head_on_and_inside(oracle):
    # head-on ray vs box{min=(1.75,.25,-.75), max=(3.25,1.75,.75)}
    a, b = (1.75, 0.25, -0.75), (3.25, 1.75, 0.75)
    ok, r = oracle.hit(2, a, b, 0, (2.5, 1.0, 5.0), (0, 0, -1), 0.001, MAXF)
    assert ok and r["t"] == 4.25 and r["p"][2] == 0.75 and r["n"] == [0, 0, 1] and r["front"]
    # from that point the next hit is t = tMin (origin inside the slab intersection), objects.go:142,181
    ok, r2 = oracle.hit(2, a, b, 0, r["p"], (0, 0, -1), 0.001, MAXF)
    assert ok and r2["t"] == 0.001 and r2["front"] and r2["n"] == [0, 0, 1]
    # exclusive range: t1 <= t0 misses (objects.go:176)
    ok, _ = oracle.hit(2, a, b, 0, (2.5, 1.0, 5.0), (0, 0, -1), 0.001, 4.25)
    assert not ok
    ok, _ = oracle.hit(2, a, b, 0, (2.5, 1.0, 5.0), (0, 0, -1), 0.001, 4.2500001)
    assert ok


def test_box_axis_parallel_ray_uses_ieee_inf(oracle):
    a, b = (-1, -1, -1), (1, 1, 1)
    ok, r = oracle.hit(2, a, b, 0, (0.5, 0.5, 5.0), (0, 0, -1), 0.001, MAXF)  # dir.x = dir.y = 0 -> invD = inf
    assert ok and r["t"] == 4.0
    ok, _ = oracle.hit(2, a, b, 0, (1.5, 0.5, 5.0), (0, 0, -1), 0.001, MAXF)  # outside the x slab
    assert not ok


def test_sphere_roots_and_inclusive_range(oracle):
    c = (0.0, 1.5, 1.0)
    ok, r = oracle.hit(0, c, (0, 0, 0), 1.2, (0, 1.5, 10.0), (0, 0, -1), 0.001, MAXF)
    assert ok and abs(r["t"] - 7.8) < 1e-12 and r["front"] and abs(r["n"][2] - 1.0) < 1e-12
    # inclusive at tMax (objects.go:56): exactly t is accepted
    ok, _ = oracle.hit(0, c, (0, 0, 0), 1.2, (0, 1.5, 10.0), (0, 0, -1), 0.001, r["t"])
    assert ok
    # from inside: near root < tMin, far root taken, back face, normal flipped (objects.go:57-61,:76-86)
    ok, r2 = oracle.hit(0, c, (0, 0, 0), 1.2, (0, 1.5, 1.0), (0, 0, -1), 0.0001, MAXF)
    assert ok and abs(r2["t"] - 1.2) < 1e-12 and not r2["front"] and abs(r2["n"][2] - 1.0) < 1e-12
    # unnormalised direction: t scales inversely
    ok, r3 = oracle.hit(0, c, (0, 0, 0), 1.2, (0, 1.5, 10.0), (0, 0, -2), 0.001, MAXF)
    assert ok and abs(r3["t"] - 3.9) < 1e-12


def test_plane_rules(oracle):
    ok, r = oracle.hit(1, (0, 0, 0), (0, 1, 0), 0, (0, 2, 0), (0, -1, 0), 0.001, MAXF)
    assert ok and r["t"] == 2.0 and r["front"] and r["n"] == [0, 1, 0]
    ok, r = oracle.hit(1, (0, 0, 0), (0, 1, 0), 0, (0, -2, 0), (0, 1, 0), 0.001, MAXF)
    assert ok and not r["front"] and r["n"] == [0, -1, 0]  # objects.go:121-130
    ok, _ = oracle.hit(1, (0, 0, 0), (0, 1, 0), 0, (0, 2, 0), (1, -1e-7, 0), 0.001, MAXF)  # |denom| < 1e-6
    assert not ok


# ----------------------------------------------------------------- materials / camera / finish

def _mat(oracle, **kw):
    m = oracle.OraMaterial()
    for k, v in kw.items():
        if isinstance(v, (tuple, list)):
            getattr(m, k)[:] = v
        else:
            setattr(m, k, v)
    out = (C.c_double * 12)()
    oracle.lib().ora_convert_material(C.byref(m), out)
    return list(out)


def test_convert_material(oracle):
    # metal: smoothness overrides rough (materials.go:36-40)
    assert _mat(oracle, type=1, rough=1.0, smoothness=1.0)[4] == 0.0
    assert _mat(oracle, type=1, rough=1.0, smoothness=0.0)[4] == 1.0
    assert _mat(oracle, type=1, rough=0.3, smoothness=0.25)[4] == 0.75
    assert _mat(oracle, type=1, rough=7.0)[4] == 1.0
    # dielectric: ior 0 -> 1.5, absorption kept (materials.go:41-46)
    d = _mat(oracle, type=2, ior=0.0, absorption=(0.1, 0.05, 0.0))
    assert d[0] == 2 and d[5] == 1.5 and d[9:12] == [0.1, 0.05, 0.0]
    # emissive: emit * power, albedo dropped (materials.go:47-48)
    e = _mat(oracle, type=3, emit=(1, 0.5, 0.25), power=8.0, albedo=(1, 1, 1))
    assert e[6:9] == [8.0, 4.0, 2.0] and e[1:4] == [0, 0, 0]
    # lambert default keeps clamp(rough) (materials.go:51-53)
    assert _mat(oracle, type=0, rough=-2.0)[4] == 0.0


def test_camera_setup(oracle):
    cam = oracle.OraCamera()
    cam.position[:] = (0, 0, 1)
    cam.target[:] = (0, 0, 0)
    cam.up[:] = (0, 1, 0)
    cam.fov = 90.0
    out = (C.c_double * 22)()
    oracle.lib().ora_camera_setup(C.byref(cam), 200, 100, out)
    o = list(out)
    h = oracle.lib().ora_tan(90.0 * math.pi / 180 / 2)
    assert abs(h - 1.0) < 1e-15
    assert o[6:9] == pytest.approx([2 * 2 * h, 0, 0])          # horizontal: aspect W/H = 2, focus = |pos-target| = 1
    assert o[9:12] == pytest.approx([0, 2 * h, 0])             # vertical
    assert o[3:6] == pytest.approx([-2 * h, -h, 0.0])          # lower-left corner
    cam.aspect_ratio = 1.0                                     # scene aspect overrides W/H (camera.go:20-23)
    oracle.lib().ora_camera_setup(C.byref(cam), 200, 100, out)
    assert list(out)[6:9] == pytest.approx([2 * h, 0, 0])


def test_pixel_finish(oracle):
    L = oracle.lib()

    def fin(sum_, spp):
        o = (C.c_uint8 * 3)()
        L.ora_finish_pixel((C.c_double * 3)(*sum_), spp, o)
        return list(o)

    assert fin((4.0, 1.0, 0.0), 4) == [255, int(0.5 * 255.999), 0]       # renderer.go:190-221
    assert fin((100.0, -1.0, float("nan")), 1) == [255, 0, 0]            # clamp; sqrt(-1) = NaN -> 0 on amd64
    assert fin((0.25, 0.25, 0.25), 1) == [127, 127, 127]                 # uint8(0.5*255.999) truncates


# ----------------------------------------------------------------- closed-form scenes

def _doc(objects, materials, sky, cam=None):
    cam = cam or {"position": {"x": 0, "y": 0, "z": 5}, "target": {"x": 0, "y": 0, "z": 0},
                  "up": {"x": 0, "y": 1, "z": 0}, "fov": 40, "aperture": 0, "focus_dist": 5, "aspect_ratio": 0}
    return {"camera": cam, "objects": objects, "materials": materials, "sky": sky,
            "background": {"r": 0.3, "g": 0.2, "b": 0.1}}


def test_empty_scene_gradient_sky_closed_form(oracle):
    sky = {"type": "gradient", "horizon": {"r": 1, "g": 1, "b": 1}, "zenith": {"r": 0.2, "g": 0.4, "b": 1.0}}
    sc = oracle.Scene(_doc([], [], sky))
    w, h = 16, 9
    r = oracle.render(sc, w, h, 4, 5, seed=9)
    assert r["stats"]["segments"] == w * h * 4  # one miss per sample
    # every sample is a point on the gradient between horizon and zenith: bounded and blue >= red
    avg = r["accum"] / 4
    assert np.all(avg[..., 2] >= avg[..., 0] - 1e-12) and np.all(avg <= 1.0 + 1e-12) and np.all(avg >= 0.2 - 1e-12)
    # a missing sky falls back to the background colour exactly (renderer.go:84-91)
    sc2 = oracle.Scene(_doc([], [], None))
    r2 = oracle.render(sc2, w, h, 3, 5, seed=9)
    assert np.array_equal(r2["accum"], np.broadcast_to(np.array([0.3, 0.2, 0.1]) * 3, (h, w, 3)))
    # an unknown sky type also means background (renderer.go:84-88)
    sc3 = oracle.Scene(_doc([], [], {"type": "hdr", "color": {"r": 9, "g": 9, "b": 9}}))
    assert np.array_equal(oracle.render(sc3, w, h, 3, 5, seed=9)["accum"], r2["accum"])


def test_emissive_sphere_returns_emit_times_power(oracle):
    mats = [{"id": "l", "type": "emissive", "emit": {"r": 1, "g": 0.5, "b": 0.25}, "power": 4}]
    objs = [{"id": "s", "type": "sphere_light", "position": {"x": 0, "y": 0, "z": 0}, "size": {"x": 50, "y": 0, "z": 0},
             "material_id": "l"}]
    # camera inside the huge light: every ray hits it first (back face, still emissive)
    r = oracle.render(oracle.Scene(_doc(objs, mats, {"type": "solid", "color": {"r": 0, "g": 0, "b": 0}})), 8, 8, 2, 4)
    assert np.array_equal(r["accum"], np.broadcast_to(np.array([4.0, 2.0, 1.0]) * 2, (8, 8, 3)))
    assert r["stats"]["segments"] == 8 * 8 * 2


def test_lambert_sphere_under_solid_sky_is_albedo_times_sky(oracle):
    # a convex lambert object under a constant sky: every hit sample bounces once and escapes, so with
    # depth >= 4 (no roulette on the first bounce) L = albedo * sky exactly; misses see the sky
    mats = [{"id": "m", "type": "lambert", "albedo": {"r": 0.5, "g": 0.25, "b": 0.125}}]
    objs = [{"id": "s", "type": "sphere", "position": {"x": 0, "y": 0, "z": 0}, "size": {"x": 1, "y": 0, "z": 0},
             "material_id": "m"}]
    sky = {"type": "solid", "color": {"r": 0.8, "g": 0.6, "b": 0.4}}
    r = oracle.render(oracle.Scene(_doc(objs, mats, sky)), 24, 24, 1, 8, seed=5)
    acc = r["accum"].reshape(-1, 3)
    hit = np.array([0.5 * 0.8, 0.25 * 0.6, 0.125 * 0.4])
    miss = np.array([0.8, 0.6, 0.4])
    is_hit = np.all(acc == hit, axis=1)
    is_miss = np.all(acc == miss, axis=1)
    assert np.all(is_hit | is_miss) and is_hit.sum() > 50 and is_miss.sum() > 50
    assert np.all(r["nseg"].reshape(-1)[is_hit] == 2) and np.all(r["nseg"].reshape(-1)[is_miss] == 1)
    assert np.all(r["ndraw"].reshape(-1)[is_hit] == 4)  # u, v, r1, r2; no lens, no roulette


def test_russian_roulette_on_last_three_levels(oracle):
    # depth 3: roulette applies from the first bounce (renderer.go:375-393): survivors are divided by p
    mats = [{"id": "m", "type": "lambert", "albedo": {"r": 0.5, "g": 0.25, "b": 0.125}}]
    objs = [{"id": "s", "type": "sphere", "position": {"x": 0, "y": 0, "z": 0}, "size": {"x": 1, "y": 0, "z": 0},
             "material_id": "m"}]
    sky = {"type": "solid", "color": {"r": 1, "g": 1, "b": 1}}
    r = oracle.render(oracle.Scene(_doc(objs, mats, sky)), 24, 24, 1, 3, seed=5)
    acc = r["accum"].reshape(-1, 3)
    vals = {tuple(v) for v in acc}
    p = 0.5  # min(max albedo, 0.95)
    assert vals <= {(1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.5 / p, 0.25 / p, 0.125 / p)}
    assert (0.0, 0.0, 0.0) in vals and (1.0, 0.5, 0.25) in vals


def test_mirror_box_reflects_solid_sky(oracle):
    mats = [{"id": "m", "type": "mirror", "albedo": {"r": 0.9, "g": 0.8, "b": 0.7}}]
    objs = [{"id": "b", "type": "box", "position": {"x": 0, "y": 0, "z": 0}, "size": {"x": 2, "y": 2, "z": 2},
             "material_id": "m"}]
    sky = {"type": "solid", "color": {"r": 0.5, "g": 0.5, "b": 1.0}}
    r = oracle.render(oracle.Scene(_doc(objs, mats, sky)), 16, 16, 1, 6, seed=2)
    acc = r["accum"].reshape(-1, 3)
    ok = np.all(acc == np.array([0.45, 0.4, 0.7]), axis=1) | np.all(acc == np.array([0.5, 0.5, 1.0]), axis=1)
    assert np.all(ok)


def test_unknown_object_and_missing_material(oracle):
    mats = [{"id": "m", "type": "velvet", "albedo": {"r": 1, "g": 1, "b": 1}}]  # unknown type -> lambert default
    objs = [{"id": "t", "type": "torus", "position": {"x": 0, "y": 0, "z": 0}, "size": {"x": 1, "y": 1, "z": 1},
             "material_id": "m"},                                                 # skipped (objects.go:237-266)
            {"id": "s", "type": "sphere", "position": {"x": 0, "y": 0, "z": 0}, "size": {"x": 1, "y": 0, "z": 0},
             "material_id": "nope"}]                                               # zero material: black lambert
    sky = {"type": "solid", "color": {"r": 1, "g": 1, "b": 1}}
    r = oracle.render(oracle.Scene(_doc(objs, mats, sky)), 16, 16, 1, 8, seed=2)
    acc = r["accum"].reshape(-1, 3)
    assert np.all(np.all(acc == 0.0, axis=1) | np.all(acc == 1.0, axis=1))
    assert np.any(np.all(acc == 0.0, axis=1))


def test_glass_sphere_enters_without_exit_refraction_and_box_creeps(oracle):
    # the exit search moves the origin to the far side of a glass sphere
    mats = [{"id": "g", "type": "dielectric", "ior": 1.5, "albedo": {"r": 1, "g": 1, "b": 1}}]
    sph = [{"id": "s", "type": "sphere", "position": {"x": 0, "y": 0, "z": 0}, "size": {"x": 1, "y": 0, "z": 0},
            "material_id": "g"}]
    sky = {"type": "solid", "color": {"r": 1, "g": 1, "b": 1}}
    r = oracle.render(oracle.Scene(_doc(sph, mats, sky)), 16, 16, 4, 8, seed=4)
    assert r["stats"]["exit_scans"] > 0
    # white sky, clear glass: every path carries throughput 1 until it escapes -> radiance exactly 1 per sample
    # unless roulette at the last levels rescales; depth 8 paths through one sphere never reach depth <= 3
    assert np.all(r["accum"] == 4.0)
    # glass box: rays that refract in creep 0.001 per bounce and die at depth 0 (contribution 0), objects.go:142
    box = [{"id": "b", "type": "box", "position": {"x": 0, "y": 0, "z": 0}, "size": {"x": 2, "y": 2, "z": 2},
            "material_id": "g"}]
    rb = oracle.render(oracle.Scene(_doc(box, mats, sky)), 16, 16, 4, 8, seed=4)
    centre = rb["accum"][8, 8]
    assert np.all(centre < 4.0) and rb["nseg"][8, 8] > 4 * 4  # long creeping paths, mostly black


def test_stream_independent_of_tiling_and_workers(oracle):
    sc = oracle.Scene.load(scene_path("example_simple"))
    full = oracle.render(sc, 48, 40, 2, 5, seed=11, workers=3)
    win = oracle.render(sc, 48, 40, 2, 5, seed=11, workers=1, window=(8, 8, 40, 33))
    assert np.array_equal(full["accum"][8:33, 8:40], win["accum"][8:33, 8:40])
    assert np.array_equal(full["rgba"][8:33, 8:40], win["rgba"][8:33, 8:40])
    one, nseg, ndraw = oracle.sample(sc, 48, 40, 2, 5, 11, 20, 17, 1)
    z, _, _ = oracle.sample(sc, 48, 40, 2, 5, 11, 20, 17, 0)
    assert np.allclose(np.array(one) + np.array(z), full["accum"][17, 20], rtol=0, atol=0)


# ----------------------------------------------------------------- the surface step, one call at a time

def _v3(x, y, z):
    return {"x": x, "y": y, "z": z}


def _rgb(r, g, b):
    return {"r": r, "g": g, "b": b}


_STEP_MATS = [
    {"id": "floor", "type": "lambert", "albedo": _rgb(0.6, 0.5, 0.4), "rough": 0.3},
    {"id": "matte", "type": "lambert", "albedo": _rgb(0.2, 0.7, 0.9)},
    {"id": "steel", "type": "metal", "albedo": _rgb(0.9, 0.85, 0.8), "rough": 0.4},
    {"id": "chrome", "type": "metal", "albedo": _rgb(0.95, 0.95, 0.95), "smoothness": 1.0},
    {"id": "mirror", "type": "mirror", "albedo": _rgb(0.9, 0.9, 0.9)},
    {"id": "lamp", "type": "emissive", "emit": _rgb(1.0, 0.8, 0.6), "power": 3.0},
    {"id": "glass", "type": "dielectric", "ior": 1.5, "albedo": _rgb(1, 1, 1), "absorption": _rgb(0.3, 0.1, 0.0)},
    {"id": "clear", "type": "dielectric", "ior": 0.0, "albedo": _rgb(1, 1, 1)},
]


def _step_scene(glass):
    objs = [{"id": "f", "type": "plane", "position": _v3(0, -1, 0), "size": _v3(0, 0, 0), "material_id": "floor"},
            {"id": "a", "type": "sphere", "position": _v3(-1.6, 0, 0), "size": _v3(1, 0, 0), "material_id": "matte"},
            {"id": "b", "type": "sphere", "position": _v3(1.7, -0.2, -0.5), "size": _v3(0.8, 0, 0), "material_id": "steel"},
            {"id": "c", "type": "box", "position": _v3(0, -0.5, -2.5), "size": _v3(1.5, 1.0, 1.0), "material_id": "chrome"},
            {"id": "d", "type": "box", "position": _v3(-0.3, 1.6, -1.0), "size": _v3(1.0, 0.2, 1.0), "material_id": "mirror"},
            {"id": "e", "type": "sphere_light", "position": _v3(2.5, 2.5, 1.0), "size": _v3(0.7, 0, 0), "material_id": "lamp"},
            {"id": "m", "type": "sphere", "position": _v3(0.6, 0.1, 2.2), "size": _v3(0.3, 0, 0), "material_id": "nobody"}]
    if glass:
        objs += [{"id": "g", "type": "sphere", "position": _v3(0.1, -0.1, 1.2), "size": _v3(0.9, 0, 0), "material_id": "glass"},
                 {"id": "h", "type": "box", "position": _v3(-1.2, -0.4, 2.0), "size": _v3(0.8, 1.2, 0.8), "material_id": "clear"}]
    cam = {"position": _v3(0.3, 0.8, 6), "target": _v3(0, 0, 0), "up": _v3(0, 1, 0), "fov": 45, "aperture": 0, "focus_dist": 6,
           "aspect_ratio": 0}
    return _doc(objs, _STEP_MATS, {"type": "solid", "color": _rgb(0.7, 0.8, 1.0)}, cam)


def _chained_sample(oracle, sc, world, sky, o, d, depth, state):
    """rayColorOpt (renderer.go:286-404) with every piece an oracle call: the closest-hit scan and the exit scan as loops of
    ora_hit over the object list, the rest through the step wrappers.  Returns (rgb, segments, exit scans, draws)."""
    levels, nseg, nexit, ndraw = [], 0, 0, 0
    while True:
        if depth <= 0:
            final = [0.0, 0.0, 0.0]
            break
        nseg += 1
        closest, rec, who = MAXF, None, None
        for w in world:
            ok, h = oracle.hit(w["kind"], w["a"], w["b"], w["radius"], o, d, 0.001, closest)
            if ok:
                closest, rec, who = h["t"], h, w
        if rec is None:
            final = list(sky)
            break
        s = oracle.scatter_step(who["mat"], rec, o, d, state)
        state, ndraw = s["state"], ndraw + s["draws"]
        if not s["ok"]:
            final = s["emitted"]
            break
        att, so, sd = s["att"], s["orig"], s["dir"]
        if who["diel"] and rec["front"]:
            nexit += 1
            exit_t, exit_p = MAXF, None
            for w in world:
                ok, h = oracle.hit(w["kind"], w["a"], w["b"], w["radius"], so, sd, 0.0001, exit_t)
                if ok and w["diel"] and not h["front"] and h["t"] < exit_t:
                    dx, dy, dz = (h["p"][k] - rec["p"][k] for k in range(3))
                    dist_sq = dx * dx + dy * dy + dz * dz
                    if 1e-8 < dist_sq < 1000.0:
                        exit_t, exit_p = h["t"], h["p"]
            att, so = oracle.exit_step(who["mat"], rec["p"], exit_p, att, so)
        ended, att, state, nd = oracle.roulette_step(depth, att, state)
        ndraw += nd
        if ended:
            final = s["emitted"]
            break
        levels.append((s["emitted"], att))
        o, d, depth = so, sd, depth - 1
    col = final
    for em, att in reversed(levels):  # em + att * next, innermost first (renderer.go:403)
        col = [em[k] + att[k] * col[k] for k in range(3)]
    return col, nseg, nexit, ndraw


def _world_of(oracle, sc):
    """sceneToWorld (objects.go:225-269) for ora_hit: kind, a, b, radius, the scene material (None: missing id), dielectric or not."""
    world = []
    for i in range(sc.c.nobjects):
        ob = sc.c.objects[i]
        pos, size = list(ob.position), list(ob.size)
        mat = sc.c.materials[ob.material] if 0 <= ob.material < sc.c.nmaterials else None
        w = {"mat": mat, "diel": mat is not None and mat.type == 2, "a": pos, "b": [0.0, 0.0, 0.0], "radius": 0.0}
        if ob.type in (0, 3):
            w.update(kind=0, radius=size[0])
        elif ob.type == 1:
            w.update(kind=1, b=[0.0, 1.0, 0.0])
        elif ob.type == 2:
            w.update(kind=2, a=[pos[k] - size[k] * 0.5 for k in range(3)], b=[pos[k] + size[k] * 0.5 for k in range(3)])
        else:
            continue
        world.append(w)
    return world


@pytest.mark.parametrize("glass", [False, True], ids=["no_glass", "glass"])
def test_step_wrappers_chained_by_hand_are_the_sample(oracle, glass):
    # ora_hit + ora_scatter_step + ora_exit_step + ora_roulette_step chained in Python reproduce ora_sample, ray by ray: the
    # wrappers are what rayColorOpt does.  depth 6, so that the roulette levels are reached with and without a draw.
    L = oracle.lib()
    sc = oracle.Scene(_step_scene(glass))
    W, H, spp, depth, seed = 34, 30, 2, 6, 77
    world = _world_of(oracle, sc)
    sky = list(sc.c.sky.color)
    full = oracle.render(sc, W, H, spp, depth, seed=seed, workers=2)
    nrays, texit, kinds = 0, 0, set()
    for y in range(H):
        for x in range(W):
            for s in range(spp):
                want, wseg, wdraw = oracle.sample(sc, W, H, spp, depth, seed, x, y, s)
                o, d = oracle.primary_ray(sc, W, H, spp, depth, seed, x, y, s)
                st = C.c_uint64(L.ora_stream_init(seed, y * W + x, s))
                L.ora_stream_next(C.byref(st)); L.ora_stream_next(C.byref(st))  # u, v (renderer.go:182-183); no lens
                got, nseg, nexit, ndraw = _chained_sample(oracle, sc, world, sky, o, d, depth, st.value)
                assert (nseg, ndraw + 2) == (wseg, wdraw), (x, y, s)
                assert np.array_equal(np.array(got).view(np.uint64), np.array(want).view(np.uint64)), (x, y, s, got, want)
                nrays, texit = nrays + 1, texit + nexit
                kinds.add(nseg)
    assert nrays >= 2000 and len(kinds) > 3
    assert texit == full["stats"]["exit_scans"] and (texit > 0) == glass
