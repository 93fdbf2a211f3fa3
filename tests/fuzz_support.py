"""The random scene generator shared by the fuzz tests (test_fuzz_gpu.py, test_fog_fuzz_gpu.py, test_glshade_fuzz_gpu.py and
the host-build fuzz of test_fog_cpu.py / test_glshade_cpu.py).

Objects overlap, touch, nest, share centres and sizes on a coarse grid on purpose: exact ties and rays that start inside
several objects are the cases where a culled strategy could differ from the sequential loop.  `random_doc` draws from the
caller's generator in a fixed order (the scenes of test_fuzz_gpu.py depend on it); everything else here either draws from
the generator it is handed, after the scene, or from a generator of its own (`set_lights`)."""
from __future__ import annotations

import numpy as np

MAT_KINDS = ["lambert", "metal", "dielectric", "emissive", "mirror"]


def random_doc(rng, nobj):
    mats = []
    for i in range(rng.integers(1, 8)):
        k = MAT_KINDS[int(rng.integers(len(MAT_KINDS)))]
        m = {"id": "m%d" % i, "type": k, "albedo": dict(zip("rgb", rng.uniform(0.1, 1.0, 3).round(3).tolist())),
             "rough": float(rng.choice([0.0, 0.0, 0.05, 0.5, 1.0])), "ior": float(rng.choice([0.0, 1.1, 1.5, 2.4])),
             "emit": dict(zip("rgb", rng.uniform(0.2, 1.0, 3).round(3).tolist())), "power": float(rng.uniform(1, 8)),
             "absorption": dict(zip("rgb", rng.choice([0.0, 0.0, 0.2, 1.0], 3).tolist())),
             "smoothness": float(rng.choice([0.0, 0.0, 0.7, 1.0]))}
        mats.append(m)
    objs = []
    grid = lambda lo, hi: float(rng.integers(lo * 2, hi * 2 + 1)) / 2.0  # half-unit grid: coincident faces are common
    for i in range(nobj):
        kind = rng.choice(["sphere", "box", "box", "sphere", "sphere_light", "plane"], p=[0.3, 0.25, 0.15, 0.15, 0.1, 0.05])
        pos = {"x": grid(-3, 3), "y": grid(0, 4), "z": grid(-3, 3)}
        if kind == "box":
            size = {"x": grid(0, 3), "y": grid(0, 3), "z": grid(0, 3)}
        else:
            size = {"x": float(rng.choice([0.25, 0.5, 1.0, 1.5])), "y": 0, "z": 0}
        objs.append({"id": "o%d" % i, "type": str(kind), "position": pos, "size": size,
                     "material_id": "m%d" % int(rng.integers(len(mats) + 1))})  # sometimes a missing id
    cam = {"position": {"x": grid(-2, 2), "y": grid(1, 3), "z": 7.0}, "target": {"x": 0, "y": 1.5, "z": 0},
           "up": {"x": 0, "y": 1, "z": 0}, "fov": float(rng.choice([35, 60, 90])), "aperture": float(rng.choice([0, 0, 0.2])),
           "focus_dist": float(rng.choice([0, 7])), "aspect_ratio": float(rng.choice([0, 1.7777778]))}
    sky = [None, {"type": "gradient", "horizon": {"r": 1, "g": 1, "b": 1}, "zenith": {"r": 0.3, "g": 0.5, "b": 1}},
           {"type": "solid", "color": {"r": 0.7, "g": 0.8, "b": 0.9}}][int(rng.integers(3))]
    return {"camera": cam, "objects": objs, "materials": mats, "sky": sky, "background": {"r": 0.1, "g": 0.1, "b": 0.15}}


def random_fog_block(rng) -> dict:
    """A scene file's "fog" object over the corners of the parameter resolution and of mediumCoeffs that FOG_TABLE of
    test_fog_cpu.py enumerates one by one: scatter 0 and 1, explicit and negative sigmas, g at and beyond +-0.9, hetero 0,
    between and above 1, noise scale 0, ordinary and huge, octaves 0..7, affect_sky either way, gpu_volumetric mostly true."""
    pick = lambda *v: float(v[int(rng.integers(len(v)))])
    fog = {"density": pick(0.0, 0.02, 0.05, 0.15, 0.6),
           "color": dict(zip("rgb", rng.uniform(0.2, 1.0, 3).round(3).tolist())),
           "scatter": pick(0.0, 0.0, 0.3, 0.5, 1.0, 1.0, 2.0),
           "g": pick(0.0, 0.3, -0.4, 0.9, -0.9, 1.7, -3.0),
           "hetero_strength": pick(0.0, 0.0, 0.3, 0.6, 1.0, 1.5),
           "noise_scale": pick(0.0, 2.0, 2.5, 50.0, 3e7),
           "noise_octaves": int(rng.integers(0, 8)),
           "affect_sky": bool(rng.integers(2)),
           "gpu_volumetric": bool(rng.random() < 0.9)}
    mode = int(rng.integers(4))
    if mode == 1:    # explicit coefficients
        fog["sigma_s"], fog["sigma_a"] = pick(0.02, 0.04, 0.2), pick(0.0, 0.01, 0.05)
    elif mode == 2:  # one or both negative: falls back to the density or stands as given
        fog["sigma_s"], fog["sigma_a"] = pick(-0.2, 0.05), pick(-0.1, 0.03)
    elif mode == 3 and rng.random() < 0.3:  # coefficients without a density
        fog["density"], fog["sigma_s"], fog["sigma_a"] = 0.0, 0.05, 0.02
    return fog


def random_gl_extras(doc: dict, rng) -> dict:
    """Adds to the materials of `doc` the GL-only fields the loader reads: absorption_scale, tint, reflectivity (zero, which
    takes the per-type default, ordinary, and out of range)."""
    for m in doc["materials"]:
        if rng.random() < 0.6:
            m["reflectivity"] = float(rng.choice([0.0, 0.4, 0.7, 1.0, 1.4, -1.0]))
        if rng.random() < 0.5:
            m["absorption_scale"] = float(rng.choice([0.0, 0.01, 0.3, 1.0, -0.2]))
        if rng.random() < 0.5:
            m["tint"] = dict(zip("rgb", [[0.0, 0.0, 0.0], [0.6, 1.0, 0.7], [1.0, 1.0, 1.0], [0.5, 0.2, 0.9]][int(rng.integers(4))]))
    return doc


def set_lights(doc: dict, n: int, kind: str = "sphere_light", seed: int = 0) -> dict:
    """Makes `doc` a scene with exactly `n` lights, all of them `kind` ("sphere_light", or "sphere" for plain emissive
    spheres): the light list of the fog term (emissive spheres) and of GL shading (any object whose material is emissive)
    then both have n entries, so 0, 1, 8, 9 and more walk GL's 8-light subset rule and the fog's per-light draws.

    The materials the generator made emissive become lambert (they keep their place, so material 0 -- what a missing id
    means to GL -- is no light either); the lights get materials of their own, appended.  Positions, sizes and the places in
    the object list come from a generator seeded by (seed, n) alone: the result does not depend on what else was drawn
    from which generator before."""
    assert kind in ("sphere_light", "sphere")
    rng = np.random.default_rng([int(seed), int(n), 0x11687])
    for m in doc["materials"]:
        if m.get("type") == "emissive":
            m["type"] = "lambert"
    nm = min(n, 3)
    for i in range(nm):
        doc["materials"].append({"id": "lamp%d" % i, "type": "emissive", "albedo": {"r": 0, "g": 0, "b": 0},
                                 "emit": dict(zip("rgb", rng.uniform(0.3, 1.0, 3).round(3).tolist())),
                                 "power": float(rng.uniform(1, 8))})
    for i in range(n):
        pos = {"x": float(rng.integers(-6, 7)) / 2.0, "y": float(rng.integers(2, 11)) / 2.0, "z": float(rng.integers(-6, 7)) / 2.0}
        o = {"id": "lamp%d" % i, "type": kind, "position": pos,
             "size": {"x": float(rng.choice([0.15, 0.25, 0.5])), "y": 0, "z": 0}, "material_id": "lamp%d" % int(rng.integers(nm))}
        doc["objects"].insert(int(rng.integers(len(doc["objects"]) + 1)), o)
    return doc


def count_kinds(doc: dict):
    """(spheres incl. sphere_light, boxes, planes) of a document."""
    t = [o["type"] for o in doc["objects"]]
    return sum(1 for k in t if k in ("sphere", "sphere_light")), t.count("box"), t.count("plane")


def trim_to_limits(doc: dict, max_spheres: int = 128, max_boxes: int = 128) -> dict:
    """Drops the spheres and boxes beyond the grouped scan's limits (128 of a kind), last first, so a large random scene stays
    off the BVH path."""
    ns = nb = 0
    keep = []
    for o in doc["objects"]:
        if o["type"] in ("sphere", "sphere_light"):
            ns += 1
            if ns > max_spheres:
                continue
        elif o["type"] == "box":
            nb += 1
            if nb > max_boxes:
                continue
        keep.append(o)
    doc["objects"] = keep
    return doc


# ---------------------------------------------------------------- the scenes of the host-build fuzz and of the device probe
LIGHT_COUNTS = (None, 0, 1, 8, 9, 12, None, 3)  # None: the lights the generator happened to make
HOST_FUZZ_DEPTHS = (1, 3, 7, 12)


def host_fuzz_case(i: int) -> dict:
    """Case i of the per-ray / per-job fuzz (test_fog_cpu.py, test_glshade_cpu.py, test_device_math_gpu.py): a random scene of
    1..150 objects with a fog block and GL extras, a light count from LIGHT_COUNTS, and the depth and fog switch of the case.
    A function of i alone."""
    rng = np.random.default_rng([20261017, int(i)])
    nobj = [1, 2, 150, 33, 129][i] if i < 5 else int(rng.integers(1, 45)) if rng.random() < 0.6 else int(rng.integers(45, 151))
    doc = random_doc(rng, nobj)
    doc["fog"] = random_fog_block(rng)
    random_gl_extras(doc, rng)
    lights = LIGHT_COUNTS[i % len(LIGHT_COUNTS)]
    if lights is not None and nobj >= 3:
        del doc["objects"][max(1, nobj - lights):]  # keep the object count: the lights replace the last objects
        set_lights(doc, lights, "sphere_light" if (i // len(LIGHT_COUNTS)) % 2 == 0 else "sphere", seed=i)
    return {"doc": doc, "depth": HOST_FUZZ_DEPTHS[i % len(HOST_FUZZ_DEPTHS)], "fog": (i // 2) % 2 == 0, "nobj": len(doc["objects"])}
