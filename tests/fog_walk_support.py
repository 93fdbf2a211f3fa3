"""The scenes of the fog walk tests (test_fog_walk_gpu.py, test_fog_walk_cpu.py) and their reference frames.

A case is a dict: name, doc (the scene file's document), sc (the product's Scene), cfg = (w, h, spp, depth, seed).  reference(case)
renders it with tests/fog_reference.c (fog_support.reference_render: a linear scan over all objects) once per process.
shadow_census(case) casts shadow rays with numpy -- from points along a fan of rays around the camera's axis, within the march's 40
units, towards the scene's lights, by the segment tests below and none of the product's code -- and says what hid them."""
from __future__ import annotations

import json

import numpy as np

import fog_support as fs
from fuzz_support import count_kinds, random_doc, random_fog_block, set_lights
from ray_inject_support import scene_bound

V = lambda x, y, z: {"x": float(x), "y": float(y), "z": float(z)}  # noqa: E731
FOG = {"density": 0.08, "color": {"r": 0.9, "g": 0.9, "b": 1.0}, "scatter": 0.8, "g": 0.3, "hetero_strength": 0.5, "noise_scale": 2.0,
       "noise_octaves": 2, "affect_sky": True, "gpu_volumetric": True}
LAMP = {"id": "fw-lamp", "type": "emissive", "albedo": {"r": 0, "g": 0, "b": 0}, "emit": {"r": 1.0, "g": 0.85, "b": 0.6}, "power": 9.0}
ADAPTIVE_TARGET = 0.6       # the block noise target of the adaptive frame: some blocks of the fogged room stop at 2 samples, some never
LINEAR_COUNTS = (1000, 800, 600, 400, 300)
LINEAR_COUNT_ACCEPTED = 1000  # the largest of LINEAR_COUNTS the PTCORE_SCAN=uniform plan takes (84 KiB of its 160 KiB of LDS)
# seeds of the random scenes; a seed whose reference frame marches no step (a fog block without a medium) is replaced here, by hand
FUZZ_SEEDS = (1, 2, 3, 4, 5, 6, 9, 8)  # (7 drew a block without a medium)
FUZZ_COUNTS = (300, 450, 700)
FUZZ_FRAMES = ((33, 20), (20, 33))
FUZZ_LIGHTS = (1, 8, 12)

_cases = {}
_refs = {}


def _case(name, doc, cfg):
    from oracle import ora
    from path_trace_golang_amd import scene

    doc = json.loads(json.dumps(doc))
    return {"name": name, "doc": doc, "sc": scene.Scene.decode(doc), "ora": ora.Scene(doc), "cfg": tuple(cfg)}


def _cached(name, make):
    if name not in _cases:
        _cases[name] = make()
    return _cases[name]


def kinds(case):
    return count_kinds(case["doc"])


def reference(case):
    """(rgba, accum, stats) of fr_render for the case, computed once."""
    if case["name"] not in _refs:
        w, h, spp, depth, seed = case["cfg"]
        _refs[case["name"]] = fs.reference_render(case["ora"], w, h, spp, depth, seed, fs.fog_of_scene(case["doc"]["fog"]))
    return _refs[case["name"]]


# ---------------------------------------------------------------- the scenes
def threshold_case():
    """129 spheres, a plane and 2 sphere lights: one sphere more than the grouped scan takes, the smallest tree.  40 x 24: ragged blocks."""
    def make():
        mats = [{"id": "floor", "type": "lambert", "albedo": {"r": 0.7, "g": 0.7, "b": 0.7}},
                {"id": "ball", "type": "lambert", "albedo": {"r": 0.3, "g": 0.5, "b": 0.7}}, dict(LAMP)]
        objs = [{"id": "ground", "type": "plane", "position": V(0, 0, 0), "size": V(0, 0, 0), "material_id": "floor"}]
        for i in range(128):  # three layers of a 7 x 7 grid, the last 19 dropped
            gx, gz, gy = i % 7, (i // 7) % 7, i // 49
            objs.append({"id": "s%d" % i, "type": "sphere", "position": V(-3 + gx, 0.4 + 1.1 * gy, -3 + gz), "size": V(0.3 + 0.02 * (i % 5), 0, 0),
                         "material_id": "ball"})
        # the 129th: a backdrop that puts the scene bound at 42, so that every march point (at most 40 from a camera 9.5 out) lies inside
        # clip_bound = 3.5 x 42 and no turn has a reason to leave the walk
        objs.append({"id": "backdrop", "type": "sphere", "position": V(0, 6, -30), "size": V(12, 0, 0), "material_id": "ball"})
        for i, p in enumerate(((-1.5, 4.5, 1.0), (2.5, 1.6, 2.5))):
            objs.append({"id": "l%d" % i, "type": "sphere_light", "position": V(*p), "size": V(0.25, 0, 0), "material_id": "fw-lamp"})
        doc = {"name": "fog-walk-threshold", "camera": {"position": V(0.5, 2.5, 9), "target": V(0, 1.2, 0), "up": V(0, 1, 0), "fov": 55},
               "materials": mats, "objects": objs, "background": {"r": 0.05, "g": 0.05, "b": 0.08}, "fog": dict(FOG)}
        return _case("threshold", doc, (40, 24, 3, 4, 5))
    return _cached("threshold", make)


ROOM_HIDDEN_LIGHT = (1.0, -1.0, 0.5)   # below the ground plane: from a march point above the ground only the plane hides it
ROOM_BOXED_LIGHT = (-2.0, 2.0, -1.0)   # inside a box of its own


def _room_doc():
    from path_trace_golang_amd import synth

    doc = synth.make_scene(400, seed=3, room=8.0, light_every=100).encode()
    doc["objects"].append({"id": "hidden", "type": "sphere_light", "position": V(*ROOM_HIDDEN_LIGHT), "size": V(0.3, 0, 0), "material_id": "lamp"})
    doc["objects"].append({"id": "boxed", "type": "sphere_light", "position": V(*ROOM_BOXED_LIGHT), "size": V(0.2, 0, 0), "material_id": "lamp"})
    doc["objects"].append({"id": "lightbox", "type": "box", "position": V(*ROOM_BOXED_LIGHT), "size": V(0.9, 0.9, 0.9), "material_id": "wall"})
    doc["fog"] = dict(FOG)
    return doc


def room_case():
    """synth.make_scene(400, seed=3, room=8, light_every=100) -- the small room makes t_hit * len < 40 decide the march's length -- with a
    heterogeneous medium, a light below the ground plane and a light enclosed in a box."""
    return _cached("room", lambda: _case("room", _room_doc(), (48, 27, 2, 4, 7)))


def far_case():
    """The room seen from 10 units beyond clip_bound = 3.5 x the scene bound on +z, through a pinhole: every primary ray starts outside
    the range the walk was analysed for, and so do the first march points."""
    def make():
        doc = _room_doc()
        b = scene_bound(doc)
        cam = doc["camera"]
        cam["position"] = V(0.0, cam["position"]["y"], 3.5 * b + 10.0)
        cam["aperture"] = 0.0
        cam["fov"] = 25.0
        return _case("far", doc, (48, 27, 2, 4, 7))
    return _cached("far", make)


def far_crossing(case):
    """Where the march along the camera's axis (the centre pixel) starts and ends, as the largest |coordinate| of its first and last
    march point, beside clip_bound.  The march is 40 long, or ends at a hit, which lies inside the scene bound (the ground plane is
    reached far beyond 40): both ends are taken at their worst."""
    doc = case["doc"]
    b = scene_bound(doc)
    pos = np.array([doc["camera"]["position"][k] for k in "xyz"])
    tgt = np.array([doc["camera"]["target"][k] for k in "xyz"])
    u = (tgt - pos) / np.linalg.norm(tgt - pos)
    assert pos[1] / -u[1] > 40.0  # the plane is out of the march's reach
    t_enter = (pos[2] - b) / -u[2]  # no finite object is hit before the axis enters the scene cube
    reach = lambda t: float(np.abs(pos + u * t).max())  # noqa: E731
    first = min(reach(0.5 * tmax / 24) for tmax in (40.0, min(40.0, t_enter)))
    last = max(reach(23.5 * tmax / 24) for tmax in (40.0, min(40.0, t_enter)))
    return {"clip_bound": 3.5 * b, "first_point": first, "last_point": last}


def _ring_lights(doc, n, y, r, radius=0.2):
    for i in range(n):
        a = 2 * np.pi * i / max(n, 1) + 0.3
        doc["objects"].append({"id": "ring%d" % i, "type": "sphere_light", "position": V(r * np.cos(a), y + 0.3 * (i % 3), r * np.sin(a)),
                               "size": V(radius, 0, 0), "material_id": "lamp"})


def lights_case(nlight):
    """A 300-object room with exactly nlight lights."""
    def make():
        from path_trace_golang_amd import synth

        doc = synth.make_scene(300, seed=5, room=8.0, light_every=0).encode()
        _ring_lights(doc, nlight, 4.0, 2.5)
        doc["fog"] = dict(FOG, hetero_strength=0.0)
        return _case("lights%d" % nlight, doc, (32, 18, 2, 3, 11))
    return _cached("lights%d" % nlight, make)


def fuzz_case(i):
    """Random geometry i: fuzz_support.random_doc untrimmed (overlapping, nested, coincident objects, several planes, missing material
    ids), a random fog block with gpu_volumetric forced on, 1 / 8 / 12 lights."""
    def make():
        seed = FUZZ_SEEDS[i]
        rng = np.random.default_rng([911, int(seed)])
        doc = random_doc(rng, FUZZ_COUNTS[i % 3])
        fog = random_fog_block(rng)
        fog["gpu_volumetric"] = True
        set_lights(doc, FUZZ_LIGHTS[i % 3], seed=seed)
        doc["fog"] = fog
        w, h = FUZZ_FRAMES[i % 2]
        return _case("fuzz%d" % i, doc, (w, h, 1 + i % 2, (1, 4, 7)[(i // 2) % 3], 100 + seed))
    return _cached("fuzz%d" % i, make)


def linear_case(n):
    """About n objects and 4 lights: what the linear fog_kernel (PTCORE_SCAN=uniform) and the walk both render."""
    def make():
        from path_trace_golang_amd import synth

        doc = synth.make_scene(n, seed=11, room=12.0, light_every=0).encode()
        _ring_lights(doc, 4, 6.0, 3.5, radius=0.3)
        doc["fog"] = dict(FOG)
        return _case("linear%d" % n, doc, (32, 18, 2, 3, 13))
    return _cached("linear%d" % n, make)


def small_case():
    """27 objects: far below the BVH path."""
    def make():
        from path_trace_golang_amd import synth

        doc = synth.make_scene(26, seed=2, room=8.0, light_every=9).encode()
        doc["fog"] = dict(FOG)
        return _case("small", doc, (32, 18, 2, 3, 3))
    return _cached("small", make)


# ---------------------------------------------------------------- what hides the shadow rays, by numpy alone
def _world(doc):
    sph, box, planes = [], [], []
    for o in doc["objects"]:
        p = np.array([o["position"][k] for k in "xyz"])
        s = np.array([o["size"][k] for k in "xyz"])
        if o["type"] in ("sphere", "sphere_light"):
            sph.append((p, s[0]))
        elif o["type"] == "box":
            box.append((p - s / 2, p + s / 2))
        elif o["type"] == "plane":
            planes.append(p[1])
    return sph, box, planes


def _blockers(world, o, d, tmax, tmin=0.001):
    """(planes, finite objects) that hit the ray o + t d (|d| = 1) in [tmin, tmax]: the tests of objects.go, in numpy."""
    sph, box, planes = world
    npl = 0
    for y in planes:
        if abs(d[1]) >= 1e-6 and tmin <= (y - o[1]) / d[1] <= tmax:
            npl += 1
    nfin = 0
    for c, r in sph:
        oc = o - c
        hb = float(oc @ d)
        disc = hb * hb - (float(oc @ oc) - r * r)
        if disc >= 0:
            sq = np.sqrt(disc)
            if tmin <= -hb - sq <= tmax or tmin <= -hb + sq <= tmax:
                nfin += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        for lo, hi in box:
            ta, tb = (lo - o) * inv, (hi - o) * inv
            t0 = max(tmin, float(np.nanmax(np.minimum(ta, tb))))
            t1 = min(tmax, float(np.nanmin(np.maximum(ta, tb))))
            if t1 > t0:
                nfin += 1
    return npl, nfin


def shadow_census(case, samples=160):
    """Shadow rays from march points of the case towards its light centres' near sides, classified: hidden by planes only, by finite
    objects only, by both, reaching the light.  March points: 24 steps of 40 / 24 along rays from the camera through a coarse fan of
    directions around its axis, kept where they lie above every plane -- points the model's march visits or may visit; the census is
    about what the scene offers, not about a pixel's exact sample."""
    doc = case["doc"]
    world = _world(doc)
    mats = {m["id"]: m for m in doc["materials"]}
    lights = [(np.array([o["position"][k] for k in "xyz"]), o["size"]["x"]) for o in doc["objects"]
              if o["type"] in ("sphere", "sphere_light") and mats.get(o.get("material_id"), {}).get("type") == "emissive"]
    pos = np.array([doc["camera"]["position"][k] for k in "xyz"])
    tgt = np.array([doc["camera"]["target"][k] for k in "xyz"])
    axis = (tgt - pos) / np.linalg.norm(tgt - pos)
    rng = np.random.default_rng(5)
    out = {"plane_only": 0, "finite_only": 0, "both": 0, "reached": 0}
    for _ in range(samples):
        u = axis + rng.uniform(-0.3, 0.3, 3)
        u /= np.linalg.norm(u)
        p = pos + u * rng.uniform(0.5, 40.0)
        if any(p[1] <= y for y in world[2]):
            continue
        for c, r in lights:
            to = c - p
            dist = float(np.linalg.norm(to))
            if dist <= r + 0.01:
                continue
            w = to / dist
            npl, nfin = _blockers(world, p, w, dist - r - 0.002)  # to the near side of the light sphere
            out["plane_only" if npl and not nfin else "finite_only" if nfin and not npl else "both" if npl else "reached"] += 1
    return out
