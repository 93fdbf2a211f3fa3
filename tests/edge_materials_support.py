"""Scenes and material sets of test_edge_materials_cpu.py / test_edge_materials_gpu.py: whole frames whose materials are cut from the
table of the surface-step probe (shade_probe_support.py).  The probe runs the surface step itself; these frames cover
what it cannot: glass_kernel as launched, and the host's way from pt_scene to DevMat on the device."""
from __future__ import annotations

import copy

import shade_probe_support as sp

W, H, SPP, DEPTH, SEED = 32, 20, 2, 8, 5
CAM = {"position": {"x": 0, "y": 1.4, "z": 6}, "target": {"x": 0, "y": 0.8, "z": 0}, "up": {"x": 0, "y": 1, "z": 0}, "fov": 50,
       "aperture": 0, "focus_dist": 6, "aspect_ratio": 0}
SKY = {"type": "gradient", "horizon": {"r": 1, "g": 1, "b": 1}, "zenith": {"r": 0.4, "g": 0.6, "b": 1.0}}
SLOTS = ("floor", "s1", "s2", "b1", "b2", "gs", "gb", "small")


def V(x, y, z):
    return {"x": x, "y": y, "z": z}


def C3(r, g, b):
    return {"r": r, "g": g, "b": b}


def objects(large: bool):
    """A floor, two spheres, two boxes, a glass box inside a glass sphere; `large`: 140 small spheres more, which takes the hierarchy."""
    objs = [{"type": "plane", "position": V(0, 0, 0), "material_id": "floor"},
            {"type": "sphere", "position": V(-2.2, 0.8, 0.3), "size": V(0.8, 0, 0), "material_id": "s1"},
            {"type": "sphere", "position": V(2.2, 0.7, 0.6), "size": V(0.7, 0, 0), "material_id": "s2"},
            {"type": "box", "position": V(-1.0, 0.5, -2.0), "size": V(1.4, 1.0, 1.0), "material_id": "b1"},
            {"type": "box", "position": V(1.3, 0.6, -1.8), "size": V(1.0, 1.2, 1.0), "material_id": "b2"},
            {"type": "sphere", "position": V(0.0, 1.0, 1.0), "size": V(1.0, 0, 0), "material_id": "gs"},
            {"type": "box", "position": V(0.0, 1.0, 1.0), "size": V(0.8, 0.8, 0.8), "material_id": "gb"}]
    if large:
        for k in range(140):
            i, j = k % 14, k // 14
            objs.append({"type": "sphere", "position": V(-3.25 + 0.5 * i, 0.12, 2.2 + 0.3 * j), "size": V(0.12, 0, 0), "material_id": "small"})
    return objs


def _m(typ, **kw):
    d = {"type": typ, "albedo": C3(0.8, 0.6, 0.4), "rough": 0.3, "smoothness": 0.0, "ior": 1.5, "emit": C3(1.0, 0.8, 0.6), "power": 3.0,
         "absorption": C3(0.3, 0.1, 0.05)}   # every type carries every field (shade_probe_support.BASE)
    d.update(kw)
    return d


_GLASS = dict(gs=_m("dielectric"), gb=_m("dielectric", ior=1.1, absorption=C3(0, 0, 0)))
_PLAIN = dict(floor=_m("lambert", rough=0.0), s1=_m("metal"), s2=_m("lambert"), b1=_m("mirror"), b2=_m("lambert", rough=0.0), small=_m("lambert", rough=0.0))

# six finite sets, by what they put on the paths; values from shade_probe_support's lists
SETS = {
    "ior": dict(_PLAIN, gs=_m("dielectric", ior=0.5), gb=_m("dielectric", ior=sp.up(1.0)), s1=_m("dielectric", ior=-1.0),
                s2=_m("dielectric", ior=2.4), b1=_m("dielectric", ior=0.0), b2=_m("dielectric", ior=sp.down(1.0))),
    "albedo": dict(_PLAIN, **_GLASS, floor=_m("lambert", albedo=C3(0.95, sp.down(0.95), sp.up(0.95))),
                   s1=_m("lambert", albedo=C3(1e-6, sp.down(1e-6), sp.up(1e-6))), s2=_m("metal", albedo=C3(5.0, 0.0, -0.0)),
                   b1=_m("mirror", albedo=C3(1.0, 1.0, 1.0)), b2=_m("lambert", albedo=C3(0.0, 5e-324, -0.25)),
                   small=_m("lambert", albedo=C3(sp.down(1e-6), 2e-6, 0.0))),
    "absorption": dict(_PLAIN, gs=_m("dielectric", absorption=C3(0.4, -0.2, -0.1)), gb=_m("dielectric", ior=1.1, absorption=C3(1e3, 2e3, 5e2)),
                       s1=_m("dielectric", absorption=C3(1e-300, 1e-300, 1e-300)), s2=_m("dielectric", absorption=C3(-0.0, -0.0, -0.0)),
                       b1=_m("dielectric", absorption=C3(1e308, 1e308, 1e308)), b2=_m("dielectric", ior=2.4, absorption=C3(0, 0, 0))),
    "rough": dict(_PLAIN, **_GLASS, floor=_m("lambert", rough=sp.up(1e-6)), s1=_m("lambert", rough=1e-6), s2=_m("metal", rough=sp.down(1e-6)),
                  b1=_m("metal", rough=sp.up(1e-6)), b2=_m("metal", rough=1.5, smoothness=0.3), small=_m("lambert", rough=1.5)),
    "emission": dict(_PLAIN, **_GLASS, s1=_m("emissive"), s2=_m("emissive", emit=C3(1.0, -0.8, 0.6)), b1=_m("emissive", power=0.0),
                     b2=_m("emissive", emit=C3(1e300, 1.0, 1e-300), power=1.0), small=_m("emissive", emit=C3(0.0, -0.0, 5e-324))),
    "mix": dict(_PLAIN, gs=_m("dielectric", ior=0.5, absorption=C3(0.4, -0.2, -0.1)), gb=_m("dielectric", ior=-1.5, absorption=C3(1e3, 2e3, 5e2)),
                floor=_m("lambert", rough=sp.up(1e-6), albedo=C3(0.95, sp.down(0.95), sp.up(0.95))), s1=_m("metal", rough=1.0, albedo=C3(5.0, 0.0, -0.0)),
                s2=_m("emissive", emit=C3(1.0, -0.8, 0.6)), b1=_m("metal", rough=0.0, smoothness=2.0), b2=_m("lambert", albedo=C3(0.0, 5e-324, -0.25))),
}
# the seventh: non-finite fields, patched into the decoded scenes (JSON cannot carry them): (slot, field, component or None, value)
NONFINITE = "nonfinite"
NONFINITE_BASE = dict(_PLAIN, **_GLASS, floor=_m("lambert"), s2=_m("metal"), b2=_m("dielectric", ior=2.4))
NONFINITE_PATCHES = (("floor", "rough", None, float("inf")), ("s1", "albedo", "g", float("nan")), ("s2", "rough", None, float("nan")),
                     ("b1", "albedo", "r", float("nan")), ("b2", "ior", None, float("inf")), ("gs", "absorption", "b", float("nan")),
                     ("gb", "ior", None, float("nan")), ("small", "smoothness", None, float("nan")))
SET_NAMES = tuple(SETS) + (NONFINITE,)


def ordinary_materials():
    """The same slots with the everyday materials of test_edge_scenes_gpu.MATS: what the edge sets are measured against."""
    from test_edge_scenes_gpu import MATS

    by_id = {m["id"]: m for m in MATS}
    pick = dict(floor="d", s1="m", s2="r", b1="d", b2="m", gs="g", gb="g", small="d")
    return [dict(copy.deepcopy(by_id[pick[s]]), id=s) for s in SLOTS]


def document(set_name: str, large: bool):
    """The scene document of a set (the non-finite set: before its patches)."""
    if set_name == "ordinary":
        mats = ordinary_materials()
    else:
        src = NONFINITE_BASE if set_name == NONFINITE else SETS[set_name]
        mats = [dict(copy.deepcopy(src[s]), id=s) for s in SLOTS]
    return {"camera": CAM, "sky": SKY, "objects": objects(large), "materials": mats}


def oracle_scene(oracle, set_name: str, large: bool):
    sc = oracle.Scene(document(set_name, large))
    if set_name == NONFINITE:
        for slot, field, comp, val in NONFINITE_PATCHES:
            m = sc._mats[SLOTS.index(slot)]
            if comp is None:
                setattr(m, field, val)
            else:
                getattr(m, field)["rgb".index(comp)] = val
    return sc


def product_scene(set_name: str, large: bool):
    from path_trace_golang_amd import scene

    sc = scene.Scene.decode(document(set_name, large))
    if set_name == NONFINITE:
        for slot, field, comp, val in NONFINITE_PATCHES:
            m = sc.materials[SLOTS.index(slot)]
            if comp is None:
                setattr(m, field, val)
            else:
                setattr(getattr(m, field), comp, val)
    return sc


_frames = {}


def oracle_frame(oracle, set_name: str, large: bool):
    key = (set_name, large)
    if key not in _frames:
        _frames[key] = oracle.render(oracle_scene(oracle, set_name, large), W, H, SPP, DEPTH, seed=SEED)
    return _frames[key]
