"""Chosen primary rays for pt_debug_set_primary_rays (include/ptcore.h), the scenes they are traced in, the predicates that
say what each ray is for, and the comparison with the oracle's ora_sample_ray.  Shared by test_ray_inject_cpu.py (no GPU:
the generators hold what they claim) and test_ray_inject_gpu.py (every ray through every scan form, ray by ray).

A frame is 64 x 64 pixels with one sample each: 4096 rays, 64 waves.  Ray generation numbers the jobs of a chunk tile by
tile, 8x8 sub-block by sub-block, sample by sample (job_pixel in csrc/pt_kernels.h), so a wave is one 8x8 pixel block of
one sample: wave_of(x, y) names it, lane_of(x, y) is the lane.  Every class is built as [64 waves][64 lanes][6] and laid
out through these two, so "lane 31 of wave 5" below is lane 31 of a wave on the device.

The thresholds are the kernels' (csrc/pt_kernels.h, csrc/pt_primary.h, build_broad in csrc/ptcore.hip), restated on the
inputs: B = 8 is the scene bound (the wall reaches it), m = B/4096 the margin of every FP32 bound,
  tame      a = d.d in [1e-100, 1e100] and every |origin component| <= 1e100, else the reference's own loop for the wave
  trusted   fa (a in FP32) in (1e-30, 1e30) and every |origin component| <= 4 B, else the lane keeps every candidate
  clip      some |origin component| > 3.5 B: the ray is clipped against the scene cube first
  far       reach * 3e-8 > m / 4 (reach = |o|_1 + |d|_1 |t_entry|): about 2034.5 B
"""
import numpy as np

W = H = 64
DEPTH = 6
SEED = 21
NWAVES = (W // 8) * (H // 8)
BOUND = 8.0
MARGIN = BOUND / 4096.0
TMIN = 0.001                      # renderer.go:296
CLIP_BOUND = 3.5 * BOUND
ORIGIN_BOUND = 4.0 * BOUND
FAR_REACH = MARGIN * 0.25 / 3.0e-8   # 2034.5 B
TAME = 1e100
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_TRUE_MIN = 2.0 ** -149
# |d| around which class 1 is dense, with what happens there
LENGTHS = {"fa trust low": 1e-15, "fa trust high": 1e15, "tame low": 1e-50, "tame high": 1e50, "FLT_MAX": FLT_MAX,
           "FLT_MIN": FLT_MIN, "FP32 subnormal": FLT_TRUE_MIN, "a overflows": 2.0 ** 511, "a underflows": 2.0 ** -511}

V = lambda x, y, z: {"x": float(x), "y": float(y), "z": float(z)}  # noqa: E731
MATS = [{"id": "d", "type": "lambert", "albedo": {"r": 0.7, "g": 0.6, "b": 0.5}},
        {"id": "g", "type": "dielectric", "ior": 1.5, "albedo": {"r": 1, "g": 1, "b": 1}, "absorption": {"r": 0.2, "g": 0.1, "b": 0}},
        {"id": "m", "type": "metal", "albedo": {"r": 0.9, "g": 0.9, "b": 0.9}, "rough": 0.0},
        {"id": "r", "type": "metal", "albedo": {"r": 0.8, "g": 0.7, "b": 0.6}, "rough": 0.4},
        {"id": "e", "type": "emissive", "emit": {"r": 1, "g": 1, "b": 1}, "power": 4}]
SKY = {"type": "gradient", "horizon": {"r": 1, "g": 1, "b": 1}, "zenith": {"r": 0.4, "g": 0.6, "b": 1.0}}
CAMERA = {"position": V(0, 3, 12), "target": V(0, 2, 0), "up": V(0, 1, 0), "fov": 40, "aperture": 0, "focus_dist": 0, "aspect_ratio": 0}

# the probes every scene starts with (the rays aim at these): (type, centre, size, material)
PROBES = [("plane", (0, 0, 0), (0, 0, 0), "d"),
          ("sphere", (0, 2, 0), (1.5, 0, 0), "d"),
          ("sphere", (-4, 1, 2), (1, 0, 0), "g"),           # glass, tangent to the floor
          ("sphere", (4.5, 3, -3), (0.25, 0, 0), "m"),      # small, far from the centre
          ("box", (3, 1, 2), (2, 2, 2), "d"),               # faces at x = 2, 4; y = 0, 2; z = 1, 3
          ("box", (-2, 2.5, -4), (3, 1, 1), "g"),           # glass slab
          ("box", (0, 4, -7.5), (16, 8, 1), "r"),           # wall out to the scene bound B = 8
          ("sphere_light", (2, 5, 3), (0.5, 0, 0), "e"),
          ("sphere", (-1, 4.5, 3), (0.75, 0, 0), "g"),      # a second glass sphere, off the floor
          ("sphere", (5, 1, 5), (1, 0, 0), "r")]
SPHERES = [(np.array(c, float), s[0]) for t, c, s, _ in PROBES if t in ("sphere", "sphere_light")]
GLASS_SPHERES = [(np.array(c, float), s[0]) for t, c, s, m in PROBES if t == "sphere" and m == "g"]
BOXES = [(np.array(c, float) - np.array(s, float) / 2, np.array(c, float) + np.array(s, float) / 2) for t, c, s, _ in PROBES[:6] if t == "box"]
GLASS_BOX = BOXES[1]
# spheres / boxes per size class: candidate bitmask (<= 32 of a kind), grouped masks (<= 128), hierarchy with its primary pass
SIZE_CLASSES = {"bitmask": (10, 10), "grouped": (44, 40), "bvh": (180, 160)}
VERIFY_MODE = {"bitmask": "verify", "grouped": "verify_wide", "bvh": "verify_bvh"}
SCENE_NAMES = list(SIZE_CLASSES) + ["two_planes"]


def scene_doc(name):
    """The scene of a size class: the probes, then filler on a half-unit grid inside the bound (coincident faces and centres
    are common).  "two_planes" is the small scene with a second plane, which turns the single-plane shortcut (plane0 in
    DevFrame) off; the engine builds every plane with the normal (0, 1, 0) (objects.go:246-249), so the second one is a
    ceiling, not a tilted plane."""
    n_s, n_b = SIZE_CLASSES.get(name, SIZE_CLASSES["bitmask"])
    rng = np.random.default_rng(11)
    objs = [{"type": t, "position": V(*c), "size": V(*s), "material_id": m} for t, c, s, m in PROBES]
    if name == "two_planes":
        objs.insert(4, {"type": "plane", "position": V(0, 7.75, 0), "size": V(0, 0, 0), "material_id": "r"})
    while sum(o["type"] in ("sphere", "sphere_light") for o in objs) < n_s:
        p = [float(rng.integers(-12, 13)) / 2, float(rng.integers(1, 12)) / 2, float(rng.integers(-12, 13)) / 2]
        objs.append({"type": "sphere_light" if rng.random() < 0.05 else "sphere", "position": V(*p),
                     "size": V(float(rng.choice([0.25, 0.5, 0.75])), 0, 0), "material_id": str(rng.choice(list("ddgmre")))})
    while sum(o["type"] == "box" for o in objs) < n_b:
        p = [float(rng.integers(-12, 13)) / 2, float(rng.integers(1, 12)) / 2, float(rng.integers(-12, 13)) / 2]
        s = [float(rng.integers(1, 4)) / 2 for _ in range(3)]
        objs.append({"type": "box", "position": V(*p), "size": V(*s), "material_id": str(rng.choice(list("ddgmr")))})
    return {"camera": CAMERA, "sky": SKY, "objects": objs, "materials": MATS}


def scene_bound(doc):
    """B as build_broad computes it: the largest |coordinate| any sphere or box reaches (at least 1)."""
    b = 1.0
    for o in doc["objects"]:
        p, s = [o["position"][k] for k in "xyz"], [o["size"][k] for k in "xyz"]
        if o["type"] in ("sphere", "sphere_light"):
            b = max(b, max(abs(c) + abs(s[0]) for c in p))
        elif o["type"] == "box":
            b = max(b, max(max(abs(c - e / 2), abs(c + e / 2)) for c, e in zip(p, s)))
    return b


# ---------------------------------------------------------------- layout

def wave_of(x, y):
    """The wave (0 .. 63) that traces pixel (x, y) of the 64 x 64 frame: its 8x8 block, in job order (tile, sub-block)."""
    tile = (y // 32) * (W // 32) + (x // 32)
    return tile * 16 + ((y % 32) // 8) * 4 + (x % 32) // 8


def lane_of(x, y):
    return (y % 8) * 8 + (x % 8)


def to_table(by_wave):
    """[64 waves][64 lanes][6] -> the [W*H][6] table pt_debug_set_primary_rays takes at spp = 1 (index y*W + x)."""
    by_wave = np.asarray(by_wave, float).reshape(NWAVES, 64, 6)
    ys, xs = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(by_wave[wave_of(xs, ys), lane_of(xs, ys)].reshape(W * H, 6))


def waves_of_table(table):
    """The wave of every row of a [W*H][6] table."""
    ys, xs = np.mgrid[0:H, 0:W]
    return wave_of(xs, ys).reshape(-1)


# ---------------------------------------------------------------- predicates on the inputs

def dir_a(r):
    """a = d.d as the kernels and objects.go:41 compute it (FP64, left to right; inf on overflow, 0 on underflow)."""
    with np.errstate(all="ignore"):
        return r[:, 3] * r[:, 3] + r[:, 4] * r[:, 4] + r[:, 5] * r[:, 5]


def dir_fa(r):
    """a from the FP32 direction, as scan_broad_narrow forms it (components overflow to inf or flush to 0 first)."""
    with np.errstate(all="ignore"):
        d = r[:, 3:6].astype(np.float32)
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(np.float64)


def is_finite(r):
    return np.all(np.isfinite(r), axis=1)


def omax(r):
    with np.errstate(all="ignore"):
        return np.max(np.abs(r[:, 0:3]), axis=1)


def is_tame(r):
    a = dir_a(r)
    with np.errstate(all="ignore"):
        return (a >= 1e-100) & (a <= 1e100) & (omax(r) <= TAME)


def is_trusted_length(r):
    fa = dir_fa(r)
    with np.errstate(all="ignore"):
        return (fa > 1e-30) & (fa < 1e30)


def beyond_clip(r, bound=BOUND):
    with np.errstate(all="ignore"):
        return omax(r) > 3.5 * bound


def beyond_origin_bound(r, bound=BOUND):
    with np.errstate(all="ignore"):
        return omax(r) > 4.0 * bound


def reach(r, bound=BOUND):
    """clip_ray's `reach` for rays that start outside the clip bound (FP64 division where the kernel takes a reciprocal
    accurate to 2^-26: the both-sides bands below are 1 % wide)."""
    with np.errstate(all="ignore"):
        bs = bound * (1.0 + 1.0 / 512.0)
        o, d = r[:, 0:3], r[:, 3:6]
        t0, t1 = (-bs - o) / d, (bs - o) / d
        lo = np.fmin(t0, t1)  # fmin / fmax skip the NaN of a 0 * inf slab, like the kernel's
        te = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
        return np.abs(o).sum(axis=1) + np.abs(d).sum(axis=1) * np.abs(te)


def is_far(r, bound=BOUND):
    with np.errstate(all="ignore"):
        return beyond_clip(r, bound) & ~(reach(r, bound) * 3.0e-8 <= bound / 4096.0 * 0.25)


def is_odd(r):
    """What makes a wave leave the common path because of ONE lane: a ray that is not finite, not tame, far, outside the clip
    bound, or of untrusted length."""
    return ~is_finite(r) | ~is_tame(r) | beyond_clip(r) | ~is_trusted_length(r)


# ---------------------------------------------------------------- building blocks

def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere_dirs(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _targets(rng, n):
    """Points inside the probes: three in eight in a sphere, three in eight in a box, the rest on the floor."""
    out = np.zeros((n, 3))
    for i in range(n):
        if i % 8 >= 6:
            out[i] = [rng.uniform(-7, 7), 0.0, rng.uniform(-6, 7)]
        elif i % 2 == 0:
            c, rad = SPHERES[rng.integers(len(SPHERES))]
            out[i] = c + _sphere_dirs(rng, 1)[0] * rad * 0.6 * rng.random()
        else:
            lo, hi = BOXES[rng.integers(len(BOXES))]
            out[i] = lo + (hi - lo) * rng.random(3)
    return out


def _inside_origins(rng, n):
    return np.stack([rng.uniform(-6, 6, n), rng.uniform(0.2, 7.5, n), rng.uniform(-6, 6.5, n)], axis=1)


def _aimed(rng, n):
    """n rays from inside the scene towards the probes, unit directions."""
    o = _inside_origins(rng, n)
    return np.concatenate([o, _unit(_targets(rng, n) - o)], axis=1)


def ulps(x, k):
    """x moved by k units in the last place (k of either sign)."""
    x = np.array(x, float)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def _fill(rays, n=NWAVES * 64):
    """Exactly n rays: the list, repeated from its start to fill the frame (nothing is ever cut)."""
    rays = np.asarray(rays, float).reshape(-1, 6)
    assert 256 <= len(rays) <= n, len(rays)
    reps = -(-n // len(rays))
    return np.tile(rays, (reps, 1))[:n]


def incoherent(rng, n):
    """Class 5's rays: origins uniform in the scene cube, directions uniform on the sphere."""
    return np.concatenate([rng.uniform(-BOUND, BOUND, (n, 3)), _sphere_dirs(rng, n)], axis=1)


# ---------------------------------------------------------------- the classes

def class_length():
    """1: unit directions towards the probes scaled by 2^k, k in [-600, 600], and densely (+-3 ulps, +-1 binade) around the
    lengths of LENGTHS.  Every sixth dense ray is axis-parallel, so that a = s*s lands on a known side."""
    rng = np.random.default_rng(101)
    ks = np.arange(-600, 601)
    sweep = _aimed(rng, len(ks))
    sweep[:, 3:6] *= (2.0 ** ks)[:, None]
    dense = []
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    for length in LENGTHS.values():
        scales = [float(ulps(length, k)) for k in range(-3, 4)] + [length / 2, length * 2]
        base = _aimed(rng, 30)
        for j, b in enumerate(base):
            for s in scales:
                d = axes[j % 6] if j < 6 else b[3:6]
                dense.append(np.concatenate([b[0:3] if j >= 6 else np.array([0.3, 2.1, 0.2]) - 5.0 * d, d * s]))
    return _fill(np.concatenate([sweep, np.array(dense)]))


def class_components():
    """2: directions with +-0 and subnormal components, one component 2^+-60 of the others, and exactly axis-parallel rays
    along box faces and in the floor plane."""
    rng = np.random.default_rng(102)
    out = []
    for b in _aimed(rng, 120):
        for axis in range(3):
            for val in (0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1060, 2.0 ** -1030):
                r = b.copy()
                r[3 + axis] = val
                out.append(r)
            for e in (60, -60):
                r = b.copy()
                r[3 + axis] = np.copysign(max(abs(r[3 + (axis + 1) % 3]), abs(r[3 + (axis + 2) % 3])) * 2.0 ** e, r[3 + axis])
                out.append(r)
        two = b.copy()  # two zero components: axis-parallel from a random origin
        k = int(np.argmax(np.abs(b[3:6])))
        two[3:6] = 0.0
        two[3 + k] = np.sign(b[3 + k])
        out.append(two)
    for lo, hi in BOXES:  # along every face plane of every probe box, through the face and beside it
        for axis in range(3):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            for face in (lo[axis], hi[axis]):
                for fu in (-0.25, 0.0, 0.5, 1.0, 1.25):
                    for sign in (1.0, -1.0):
                        o = np.zeros(3)
                        o[axis] = face
                        o[u] = lo[u] + (hi[u] - lo[u]) * fu
                        o[v] = (lo[v] - 3.0) if sign > 0 else (hi[v] + 3.0)
                        d = np.zeros(3)
                        d[v] = sign
                        out.append(np.concatenate([o, d]))
    for x in np.linspace(-7, 7, 15):  # in the floor plane y = 0 (and a hair above it), along x and z
        for y in (0.0, TMIN / 2):
            out.append([x, y, 7.5, 0.0, 0.0, -1.0])
            out.append([-7.5, y, x, 1.0, 0.0, 0.0])
    return _fill(np.array(out, float))


def _surface_points(rng):
    """(point, outward normal, a tangent) on the probes: sphere surfaces, box faces, edges and corners, the plane."""
    pts = []
    for c, rad in SPHERES:
        for n in _sphere_dirs(rng, 4):
            t = _unit(np.cross(n, [0.3, 0.5, 0.81]))
            pts.append((c + n * rad, n, t))
    for lo, hi in BOXES[:2]:
        for axis in range(3):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            for face, sgn in ((lo[axis], -1.0), (hi[axis], 1.0)):
                n = np.zeros(3)
                n[axis] = sgn
                t = np.zeros(3)
                t[u] = 1.0
                for fu, fv in ((0.3, 0.8), (0.0, 0.4), (1.0, 0.0)):  # on the face, on an edge, in a corner
                    p = np.zeros(3)
                    p[axis] = face
                    p[u] = lo[u] + (hi[u] - lo[u]) * fu
                    p[v] = lo[v] + (hi[v] - lo[v]) * fv
                    pts.append((p, n, t))
    for x, z in rng.uniform(-7, 7, (8, 2)):
        pts.append((np.array([x, 0.0, z]), np.array([0.0, 1.0, 0.0]), np.array([0.6, 0.0, 0.8])))
    return pts


def _off_ulps(p, n, k):
    """p moved k ulps along the normal n: every coordinate the normal has a part in, by k ulps in the normal's direction."""
    q = np.array(p, float)
    for c in range(3):
        if n[c] != 0:
            q[c] = ulps(p[c], k if n[c] > 0 else -k)
    return q


def class_near_geometry():
    """3: origins on the probes' surfaces and off them by +-{0, 1, 4} ulps and +-{tMin/2, tMin, 2 tMin} along the normal, looking
    outward, inward and along the surface; origins inside the glass spheres and the glass box (the creeping case); origins in
    the shell between an object and its inflated FP32 bound (margin B/4096)."""
    rng = np.random.default_rng(103)
    out = []
    for p, n, t in _surface_points(rng):
        starts = [p]
        for k in (1, 4):
            for sgn in (1, -1):
                starts.append(_off_ulps(p, n, sgn * k))
        for dist in (TMIN / 2, TMIN, 2 * TMIN):
            for sgn in (1.0, -1.0):
                starts.append(p + n * (sgn * dist))
        for o in starts:
            for d in (n, -n, t):
                out.append(np.concatenate([o, d]))
    for c, rad in GLASS_SPHERES:  # inside the glass spheres, from the centre out to 4 ulps under the surface
        for n, f in zip(_sphere_dirs(rng, 96), np.tile([0.0, 0.5, 0.9, 0.999, 1 - TMIN / 2, 1 - 1e-9, 1 - 2.0 ** -50, 0.2], 12)):
            out.append(np.concatenate([c + n * rad * f, _sphere_dirs(rng, 1)[0]]))
    lo, hi = GLASS_BOX
    for _ in range(192):  # inside the glass box, many of them within 2 tMin of a face, flat along it (creeping)
        o = lo + (hi - lo) * rng.random(3)
        d = _sphere_dirs(rng, 1)[0]
        if rng.random() < 0.5:
            axis = int(rng.integers(3))
            o[axis] = (lo[axis] + rng.choice([0.0, TMIN / 4, TMIN, 2 * TMIN])) if rng.random() < 0.5 else (hi[axis] - rng.choice([0.0, TMIN / 4, TMIN, 2 * TMIN]))
            d[axis] *= 1e-3
        out.append(np.concatenate([o, d]))
    for c, rad in SPHERES:  # the shell between the surface and the inflated bound: r < |o - c| < r + m
        for n in _sphere_dirs(rng, 24):
            o = c + n * (rad + MARGIN * rng.uniform(0.02, 0.98))
            out.append(np.concatenate([o, _unit(np.cross(n, rng.normal(size=3))) if rng.random() < 0.5 else -n]))
    for lo, hi in BOXES:
        for _ in range(48):
            axis = int(rng.integers(3))
            o = lo + (hi - lo) * rng.random(3)
            side = rng.random() < 0.5
            o[axis] = (lo[axis] - MARGIN * rng.uniform(0.02, 0.98)) if side else (hi[axis] + MARGIN * rng.uniform(0.02, 0.98))
            d = _sphere_dirs(rng, 1)[0]
            d[axis] = abs(d[axis]) * (1e-3 if rng.random() < 0.5 else 1.0) * (1.0 if side else -1.0)  # towards the face, often flat
            out.append(np.concatenate([o, d]))
    return _fill(np.array(out, float))


def in_shell(r):
    """Origins strictly between a probe's surface and its inflated bound."""
    o = r[:, 0:3]
    hit = np.zeros(len(r), bool)
    for c, rad in SPHERES:
        dist = np.linalg.norm(o - c, axis=1)
        hit |= (dist > rad) & (dist < rad + MARGIN)
    for lo, hi in BOXES:
        inside_big = np.all((o > lo - MARGIN) & (o < hi + MARGIN), axis=1)
        inside = np.all((o >= lo) & (o <= hi), axis=1)
        hit |= inside_big & ~inside
    return hit


def inside_glass(r):
    o = r[:, 0:3]
    hit = np.zeros(len(r), bool)
    for c, rad in GLASS_SPHERES:
        hit |= np.linalg.norm(o - c, axis=1) < rad
    lo, hi = GLASS_BOX
    return hit | np.all((o >= lo) & (o <= hi), axis=1)


FAR_FACTORS = np.concatenate([np.linspace(0.9, 0.99, 10), np.linspace(1.01, 1.1, 10), [0.999, 1.0, 1.001]])


def class_far_origins():
    """4: origins whose largest component is 0.9 ... 1.1 of B, 3.5 B (the clip switch and the primary pass's bound) and 4 B (the
    origin bound of `trusted`); whose reach is 0.9 ... 1.1 of the far threshold; with a component at 1e100 +-3 ulps and
    +-1 binade (the tame limit); with +-inf and NaN in one or all components of the origin or the direction.  Each looking at
    the scene and looking away."""
    rng = np.random.default_rng(104)
    out = []
    for base in (BOUND, CLIP_BOUND, ORIGIN_BOUND):
        for f in FAR_FACTORS:
            for j in range(14):
                u = _sphere_dirs(rng, 1)[0] if j >= 3 else np.eye(3)[j] * (1.0 if rng.random() < 0.5 else -1.0) + rng.uniform(-0.3, 0.3, 3) * (1 - np.eye(3)[j])
                u = u / np.max(np.abs(u))
                if u[1] < 0 and base > BOUND:
                    u[1] = -u[1] * 0.5  # keep the origin above the floor, the scene in view
                o = u * (base * f / np.max(np.abs(u)))
                d = _unit(_targets(rng, 1)[0] - o)
                out.append(np.concatenate([o, d if j % 4 else -d]))
    thr = FAR_REACH
    for f in FAR_FACTORS:
        for j in range(12):
            u = _sphere_dirs(rng, 1)[0]
            u[1] = abs(u[1])
            o = u * thr
            tgt = _targets(rng, 1)[0]
            r = np.concatenate([o, _unit(tgt - o)])[None, :]
            o = o * (f * thr / reach(r)[0])
            r = np.concatenate([o, _unit(tgt - o)])[None, :]
            o = o * (f * thr / reach(r)[0])
            d = _unit(tgt - o)
            out.append(np.concatenate([o, d]))
            if j % 4 == 0:
                out.append(np.concatenate([o, -d]))
    for k in (-3, -2, -1, 0, 1, 2, 3, "half", "twice"):
        big = 5e99 if k == "half" else 2e100 if k == "twice" else float(ulps(1e100, k))
        for axis in range(3):
            for sgn in (1.0, -1.0):
                for away in (False, True):
                    o = rng.uniform(-2, 2, 3)
                    o[axis] = sgn * big
                    d = rng.uniform(-1e-3, 1e-3, 3)
                    d[axis] = sgn if away else -sgn
                    out.append(np.concatenate([o, d]))
    # the oracle's arithmetic is plain IEEE double throughout (no conversion to an integer before ora_finish_pixel's clamp and
    # NaN test), so every non-finite value below is defined for it
    for bad in (np.inf, -np.inf, np.nan):
        for part in (0, 3):
            for which in ((0,), (1,), (2,), (0, 1, 2)):
                for b in _aimed(rng, 4):
                    r = b.copy()
                    for c in which:
                        r[part + c] = bad
                    out.append(r)
    return _fill(np.array(out, float))


def class_incoherent():
    """5: 64 independent rays per wave."""
    return incoherent(np.random.default_rng(105), NWAVES * 64)


ODD_KINDS = ("nan", "inf", "beyond tame", "beyond far", "beyond clip", "untrusted length")


def odd_ray(rng, kind):
    """One ray of an odd kind, looking at the scene where that means something."""
    r = _aimed(rng, 1)[0]
    if kind == "nan":
        r[int(rng.integers(6))] = np.nan
    elif kind == "inf":
        r[int(rng.integers(6))] = np.inf if rng.random() < 0.5 else -np.inf
    elif kind == "beyond tame":
        r[int(rng.integers(3))] = 3e100
    elif kind in ("beyond far", "beyond clip"):
        u = _sphere_dirs(rng, 1)[0]
        u[1] = abs(u[1])
        o = u / np.max(np.abs(u)) * (4.0 * FAR_REACH if kind == "beyond far" else rng.uniform(1.05, 3.0) * CLIP_BOUND)
        r = np.concatenate([o, _unit(_targets(rng, 1)[0] - o)])
    elif kind == "untrusted length":
        r[3:6] *= 1e-20 if rng.random() < 0.5 else 1e20
    return r


def class_mixed():
    """6: waves of 63 incoherent rays and one odd ray at lane 0, 31, 32 or 63, and waves that are half odd (lanes 0-31 or 32-63).
    Returns ([64][64][6], the odd kind of every wave)."""
    rng = np.random.default_rng(106)
    waves = incoherent(rng, NWAVES * 64).reshape(NWAVES, 64, 6)
    kinds = []
    for wv in range(NWAVES):
        kind = ODD_KINDS[wv % 6]
        if wv % 32 < 24:
            waves[wv, (0, 31, 32, 63)[(wv % 32) // 6]] = odd_ray(rng, kind)
        else:
            half = range(0, 32) if (wv // 6) % 2 == 0 else range(32, 64)
            for lane in half:
                waves[wv, lane] = odd_ray(rng, kind)
        kinds.append(kind)
    return waves, kinds


def build_classes():
    """{name: [W*H][6] table} of the six classes, laid out by wave."""
    return {"length": to_table(class_length()), "components": to_table(class_components()),
            "near geometry": to_table(class_near_geometry()), "far origins": to_table(class_far_origins()),
            "incoherent": to_table(class_incoherent()), "mixed": to_table(class_mixed()[0])}


_CLASSES = None


def classes():
    global _CLASSES
    if _CLASSES is None:
        _CLASSES = build_classes()
    return _CLASSES


# Named cases: the kind of ray a disagreement with the oracle was found on, in its plainest form.
# "beside a core": exactly axis-parallel rays through the scene of the "bvh" size class.  Two direction components are zero, so
# their FP32 reciprocals are infinite and the slab parameters of those axes are NaN, which constrain nothing.  The FP32 walk of
# PTCORE_PIPELINE=walk32 took that for "the ray pierces the core" of every object whose extent along the ray lies ahead, wherever
# the object is sideways, and shrank its bound to hits that do not exist: the object the ray really hits, further on, was culled
# (segments 13689 instead of the oracle's 15766 on the components class).  Each ray passes beside several objects (beside_cores)
# before the one it hits.
NAMED_RAYS = {"beside a core": [
    (-7.75, 0.25, -5.75, 1.0, 0.0, 0.0),    # hits box 221 after passing 109 objects
    (7.75, 0.25, -5.75, -1.0, 0.0, 0.0),    # a sphere light, 23
    (-4.25, 7.75, -5.75, 0.0, -1.0, 0.0),   # box 187, 73
    (-5.75, 0.25, 7.75, 0.0, 0.0, -1.0)]}   # box 206, 120


def _extent(o):
    """(lo, hi) of a sphere's or a box's bounding box."""
    p = np.array([o["position"][k] for k in "xyz"])
    s = np.array([o["size"][k] for k in "xyz"])
    h = np.full(3, s[0]) if o["type"] in ("sphere", "sphere_light") else s / 2
    return p - h, p + h


def beside_cores(doc, ray, hit):
    """For an exactly axis-parallel ray that first hits object `hit`: how many other spheres and boxes lie wholly between the
    origin and that object along the ray while the ray's line passes clear of their inflated bounds sideways."""
    ray = np.asarray(ray, float)
    axis = int(np.argmax(np.abs(ray[3:6])))
    assert np.count_nonzero(ray[3:6]) == 1
    sign = ray[3 + axis]
    hlo, hhi = _extent(doc["objects"][hit])
    near = hlo[axis] if sign > 0 else hhi[axis]
    n = 0
    for i, o in enumerate(doc["objects"]):
        if i == hit or o["type"] == "plane":
            continue
        lo, hi = _extent(o)
        ahead = (ray[axis] < lo[axis] and hi[axis] < near) if sign > 0 else (ray[axis] > hi[axis] and lo[axis] > near)
        clear = any(ray[k] < lo[k] - 2 * MARGIN or ray[k] > hi[k] + 2 * MARGIN for k in range(3) if k != axis)
        n += bool(ahead and clear)
    return n


def named_table(name):
    """The [W*H][6] table of a named case: its rays repeated to fill the frame."""
    rays = np.array(NAMED_RAYS[name], float)
    return to_table(np.tile(rays, (-(-W * H // len(rays)), 1))[:W * H])


def indexing_rays(w=33, h=31, spp=3):
    """The ragged case: one incoherent ray per (pixel, sample), index (y*w + x)*spp + s."""
    return incoherent(np.random.default_rng(107), w * h * spp)


# ---------------------------------------------------------------- the oracle's side

def first_hits(oracle, doc, rays):
    """Index of the object every ray hits first (-1: none) by the oracle's own loop: the scene with every object emissive in its
    own colour under a black sky, one segment deep -- the sample's red channel is the hit object's index + 1."""
    objs = [dict(o, material_id="id%d" % i) for i, o in enumerate(doc["objects"])]
    mats = [{"id": "id%d" % i, "type": "emissive", "emit": {"r": i + 1, "g": 0, "b": 0}, "power": 1} for i in range(len(objs))]
    d = {"camera": doc["camera"], "background": {"r": 0, "g": 0, "b": 0}, "objects": objs, "materials": mats}
    n = len(rays)
    rgb, _, _ = oracle.sample_rays(oracle.Scene(d), n, 1, 1, 1, SEED, rays)  # an n x 1 frame: the table order is the ray order
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(rgb[:, 0]), rgb[:, 0], 0).astype(np.int64) - 1


def hit_kinds(doc, ids):
    """Per ray: 'sphere', 'box', 'plane' or 'miss', and whether the object is glass."""
    types = np.array([{"sphere_light": "sphere"}.get(o["type"], o["type"]) for o in doc["objects"]] + ["miss"])
    glass = np.array([o["material_id"] == "g" for o in doc["objects"]] + [False])
    return types[ids], glass[ids]


_ORACLE_FRAMES = {}


def oracle_frame(oracle, doc, rays, w=W, h=H, spp=1, depth=DEPTH, seed=SEED, key=None):
    """The oracle's frame for a table of primary rays: per pixel the sum of ora_sample_ray's radiances in sample order
    (renderer.go:186), the counts, and ora_finish_pixel of the sum.  Cached under `key`: computed once, never changed."""
    import ctypes as C

    if key is not None and key in _ORACLE_FRAMES:
        return _ORACLE_FRAMES[key]
    rgb, nseg, ndraw = oracle.sample_rays(oracle.Scene(doc), w, h, spp, depth, seed, rays)
    per = rgb.reshape(h, w, spp, 3)
    acc = np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        for s in range(spp):
            acc = acc + per[:, :, s]
    rgba = np.zeros((h, w, 4), np.uint8)
    rgba[:, :, 3] = 255
    L = oracle.lib()
    px = (C.c_uint8 * 3)()
    flat = np.ascontiguousarray(acc.reshape(-1, 3))
    for i in range(w * h):
        L.ora_finish_pixel(flat[i].ctypes.data_as(C.POINTER(C.c_double)), spp, px)
        rgba[i // w, i % w, 0:3] = px[:]
    out = {"accum": acc, "rgba": rgba, "nseg": nseg.reshape(h, w, spp).sum(axis=2, dtype=np.uint32),
           "ndraw": ndraw.reshape(h, w, spp).sum(axis=2, dtype=np.uint32), "samples": w * h * spp}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    if key is not None:
        _ORACLE_FRAMES[key] = out
    return out


# ---------------------------------------------------------------- the GPU's side

def render_injected(ctx, sc, rays, w=W, h=H, spp=1, depth=DEPTH, seed=SEED, chunk=0, stats=True):
    """One frame on ctx with `rays` as the primary rays (None: the camera's).  The table is cleared again before returning.
    Returns (img, acc, nseg, ndraw, pt_stats); nseg / ndraw are None in the shipping build (stats=False)."""
    from path_trace_golang_amd import capi, hip

    img = np.zeros((h, w, 4), np.uint8)
    acc = np.zeros((h, w, 3))
    nseg = np.zeros((h, w), np.uint32) if stats else None
    ndraw = np.zeros((h, w), np.uint32) if stats else None
    ctx.set_primary_rays(rays)
    try:
        st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, seed, chunk, capi.PT_FLAG_PIXEL_STATS if stats else 0), img, None,
                        acc, nseg, ndraw, ctx=ctx)
    finally:
        ctx.set_primary_rays(None)
    return img, acc, nseg, ndraw, st


def sums_agree(got, ref, depth):
    """The suite's criterion for the FP64 sums (render_vs_oracle in conftest.py): relative 4 * max(depth, 1) * 2^-52, NaN where
    the oracle has NaN -- and equal infinities are equal."""
    with np.errstate(all="ignore"):
        return ((np.isnan(got) & np.isnan(ref)) | (got == ref) |
                (np.abs(got - ref) <= 4 * max(depth, 1) * 2.0 ** -52 * np.maximum(np.abs(ref), 1e-300)))


def injected_vs_oracle(ctx, sc, o, rays, w=W, h=H, spp=1, depth=DEPTH, seed=SEED, chunk=0, tag="", forms=("stats", "shipping")):
    """Renders `rays` on ctx in the counting build and the shipping build and holds each to the oracle frame `o` (oracle_frame),
    every pixel: counts equal, 8-bit image equal, sums by sums_agree, totals equal, and the two builds bit-equal to each other.
    Returns {form: (img, acc, nseg, ndraw, stats)}."""
    out = {}
    for form in forms:
        img, acc, nseg, ndraw, st = render_injected(ctx, sc, rays, w, h, spp, depth, seed, chunk, stats=form == "stats")
        t = (tag, form)
        assert st["samples"] == o["samples"], (t, "samples", st["samples"])
        assert st["segments"] == int(o["nseg"].sum(dtype=np.uint64)), (t, "segments", st["segments"], int(o["nseg"].sum(dtype=np.uint64)))
        assert st["draws"] == int(o["ndraw"].sum(dtype=np.uint64)), (t, "draws", st["draws"], int(o["ndraw"].sum(dtype=np.uint64)))
        if form == "stats":
            bad = np.argwhere((nseg != o["nseg"]) | (ndraw != o["ndraw"]))
            assert len(bad) == 0, (t, "counts differ at (y, x)", bad[:8].tolist(), _rays_at(rays, bad[:4], w, spp))
        bad = np.argwhere(~np.all(sums_agree(acc, o["accum"], depth), axis=2))
        assert len(bad) == 0, (t, "sums differ at (y, x)", bad[:8].tolist(), _rays_at(rays, bad[:4], w, spp))
        bad = np.argwhere(np.any(img != o["rgba"], axis=2))
        assert len(bad) == 0, (t, "pixels differ at (y, x)", bad[:8].tolist())
        out[form] = (img, acc, nseg, ndraw, st)
    if len(out) == 2:
        a, b = out["stats"], out["shipping"]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True), (tag, "the two builds differ")
        for k in ("samples", "segments", "exit_scans", "draws"):
            assert a[4][k] == b[4][k], (tag, k)
    return out


def _rays_at(rays, yx, w, spp):
    return [[float.hex(float(v)) for v in rays[(int(y) * w + int(x)) * spp]] for y, x in yx]
