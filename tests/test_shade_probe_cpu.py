"""The probe of the surface step (tests/shade_probe.hip) without a GPU: it cross-compiles for gfx950 with the library's
flags against the unchanged pt_kernels.h and exports what test_shade_probe_gpu.py calls; and the conditions that keep that test from
passing on tables that miss the point -- every branch of material.scatter, of the exit epilogue and of the roulette in numbers, the
critical angle straddled, the basis switch met on both sides and on the value itself, directions whose squared length underflows --
are asserted here on the reference's results alone."""
from __future__ import annotations

import re
import subprocess

import numpy as np

import shade_probe_support as sp


def test_probe_compiles_for_gfx950_with_the_library_flags():
    from path_trace_golang_amd import build

    assert "-ffp-contract=off" in build.HIP_FLAGS and "--offload-arch=gfx950" in build.HIP_FLAGS
    lib = sp.compile_probe()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (\w+)", syms))
    assert set(sp.SYMBOLS) <= exported, sorted(set(sp.SYMBOLS) - exported)
    with open(lib, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob
    for kernel in (b"shade_wrap", b"glass_wrap", b"normal_wrap", b"reflect_wrap", b"exit_wrap", b"roulette_wrap"):
        assert kernel in blob, kernel


def test_probe_source_wraps_the_product_functions_and_has_no_inline_assembly():
    with open(sp.SOURCE) as f:
        src = f.read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code
    for inc in ('#include "pt_kernels.h"', '#include "probe_common.h"', '#include "pt_convert.h"'):
        assert inc in src
    for name in sp.PRODUCT:
        assert name in code, name
    # the four instantiations of shade_hit, each through LDS and through global memory; both of roulette_advance
    for st in ("false", "true"):
        for gl in ("false", "true"):
            assert re.search(r"SHADE_CASE\(\d, %s, %s\)" % (st, gl), code)
        assert "roulette_wrap<%s>" % st in code and "glass_wrap<%s>" % st in code
    assert "shade_wrap<ST, GL, true>" in code and "shade_wrap<ST, GL, false>" in code
    # the copy of glass_kernel's sequence and the kernel body name each other
    with open(sp.SOURCE.replace("tests/shade_probe.hip", "path_trace_golang_amd/csrc/pt_kernels.h")) as f:
        kernels = f.read()
    assert "MUST STAY THE SAME" in src and "tests/shade_probe.hip" in kernels and "MUST STAY THE SAME" in kernels
    body = kernels[kernels.index("            // hit record of the winner\n            const DevObj &o = lds_obj[best];"):]
    body = body[:body.index("double attx = 1, atty = 1, attz = 1;")]
    strip = lambda s: re.sub(r"\s+", "", re.sub(r"//.*", "", s)).replace("ptk::", "")
    mine = src[src.index("    // hit record of the winner"):src.index("        exits = ff;")]
    assert strip(mine.replace("in.objs[i]", "lds_obj[best]")) == strip(body)


def test_every_type_meets_every_object_kind_on_both_faces():
    T, ref = sp.cases(), sp.reference()
    assert T["n"] % 64 != 0 and 30000 < T["n"] < 300000
    for typ in range(5):
        for kind in (sp.SPHERE, sp.PLANE, sp.BOX):
            for front in (False, True):
                assert ((T["typ"] == typ) & (T["kind"] == kind) & (ref["front"] == front)).sum() >= 20, (typ, kind, front)
    for oi in range(len(sp.OBJECTS)):
        assert (T["obj"] == oi).sum() > 500, sp.OBJECT_NAMES[oi]
    # neighbouring lanes differ in type and branch in table order
    assert (np.diff(T["typ"]) != 0).mean() > 0.5


def test_no_class_is_empty_and_few_generated_rays_are_dropped():
    T = sp.cases()
    G = T["rays"]
    shares = {}
    for ci, name in enumerate(sp.CLASSES):
        m = (G["cls"] == ci) & G["kept"]
        assert m.sum() > 0 and (T["cls"] == ci).sum() > 0, name
        shares[name] = 1.0 - G["ok"][m].mean()
        assert shares[name] <= 0.25, (name, shares[name])
    print("dropped share per class:", {k: round(float(v), 3) for k, v in shares.items()})
    # which (scale, object, origin) combinations the reference hits at all: only those are cases
    hit = {}
    for tag, (h, k) in G["combos"].items():
        si, oi, moved = tag // 2 // len(sp.OBJECTS), tag // 2 % len(sp.OBJECTS), tag % 2
        if 4 * h >= 3 * k:
            hit.setdefault(sp.SCALES[si], []).append(sp.OBJECT_NAMES[oi] + ("'" if moved else ""))
    print("scales the reference hits:", hit)
    assert all("box" in hit[s] for s in (1.0, 1e-150, 1e-160, 1e-170, 1e-200, 1e-300))   # t = 4e170 and beyond
    assert hit[1e-170] == ["box", "box'"] and 1e100 in hit and 1e150 in hit              # the rest cannot divide by |d|^2 = 0


def test_branches_of_scatter_in_numbers():
    T, M, ref = sp.cases(), sp.materials(), sp.reference()
    br, B = ref["branch"], sp.BRANCHES.index
    count = {name: int((br == k).sum()) for k, name in enumerate(sp.BRANCHES)}
    print("cases per branch:", count)
    assert count["glass_tir"] >= 200 and count["glass_reflect"] >= 200 and count["glass_refract"] >= 200
    assert count["metal_fallback"] >= 100    # dot <= 0: the blend points below the surface
    # (the other fallback, lenSq < 1e-8, cannot be reached with finite operands: the mirror direction and the cosine sample are
    # unit vectors, alpha lies in (1e-12, 1], and the blend's mirror component 1 - alpha * (1 - cos) cannot vanish together with the
    # tangential one.  So it is covered only through the non-finite operands: the hit records with a NaN in them that the huge
    # direction scales give, where lenSq is NaN and the comparison must come out false on the device as it does in the reference.)
    rough = M["conv"][T["mat"], 4]
    nan_rec = (T["typ"] == sp.METAL) & (rough > 1e-6) & np.isnan(T["hit"][:, 0:7]).any(axis=1) & (ref["ok"] != 0)
    assert nan_rec.sum() >= 20 and np.isnan(ref["out"][nan_rec, 9:12]).all()
    # rough lambert: 2 draws for the cosine sample and 3 per turn of the rejection loop
    lr = br == B("lambert_rough")
    draws = ref["draws"][lr]
    assert np.all((draws - 2) % 3 == 0)
    tally = {d: int((draws == d).sum()) for d in (5, 8, 11)}
    tally["14+"] = int((draws >= 14).sum())
    print("rough lambert draws:", tally)
    assert min(tally.values()) >= 50
    assert np.all(ref["draws"][br == B("lambert_smooth")] == 2) and np.all(ref["draws"][br == B("mirror")] == 0)
    # both sides of rough > 1e-6 on lambert and metal
    for typ, lo, hi in ((sp.LAMBERT, "lambert_smooth", "lambert_rough"), (sp.METAL, "metal_smooth", "metal_rough")):
        for r_, name in ((1e-6, lo), (sp.down(1e-6), lo), (sp.up(1e-6), hi)):
            m = (T["typ"] == typ) & (rough == r_) & (ref["ok"] != 0)
            assert m.sum() >= 20 and np.all(br[m] == B(name)), (typ, r_)


def test_directions_whose_squared_length_underflows_stop_the_specular_types_only():
    T, ref = sp.cases(), sp.reference()
    d = T["ray"][:, 3:6]
    under = np.any(d != 0, axis=1) & (np.sum(d * d, axis=1) == 0)      # dirLen == 0 with a non-zero direction
    assert under.sum() >= 100 and np.all(T["kind"][under] == sp.BOX)
    for typ in (sp.METAL, sp.DIELECTRIC, sp.MIRROR):
        m = under & (T["typ"] == typ)
        assert m.sum() >= 20 and not ref["ok"][m].any(), typ
    lam = under & (T["typ"] == sp.LAMBERT)
    assert lam.sum() >= 20 and ref["ok"][lam].all()
    assert (ref["branch"] == sp.BRANCHES.index("zero_dir")).sum() == (under & np.isin(T["typ"], (sp.METAL, sp.DIELECTRIC, sp.MIRROR))).sum()


def test_critical_angle_is_straddled_one_ulp_apart():
    T, M, ref = sp.cases(), sp.materials(), sp.reference()
    crit = T["cls"] == sp.CLASSES.index("critical")
    for ci, ior in enumerate(sp.CRITICAL_IORS):
        m = np.flatnonzero(crit & (T["tag"] == ci))
        assert np.all(M["conv"][T["mat"][m], 5] == ior) and np.all(ref["front"][m] == (ior < 1))
        # cases of one ray follow each other; compare the first of each ray with the first of the next
        first = m[np.r_[True, np.any(T["ray"][m][1:] != T["ray"][m][:-1], axis=1)]]
        tir = ref["draws"][first] == 0
        step = np.abs(np.diff(T["ray"][first, 3].view(np.int64)))
        pairs = (tir[1:] != tir[:-1]) & (step == 1)
        assert pairs.sum() >= 1 and tir.sum() >= 50 and (~tir).sum() >= 50, ior


def test_basis_switch_is_met_on_both_sides_and_on_the_value():
    T, M, ref = sp.cases(), sp.materials(), sp.reference()
    rough = M["conv"][T["mat"], 4]
    # lambert: w is the face normal; rough metal: w is the mirror direction (the reference's own, from a mirror on the same ray)
    for name, m, w in (("lambert", (T["typ"] == sp.LAMBERT) & (ref["ok"] != 0), T["hit"][:, 4]),
                       ("rough metal", (T["typ"] == sp.METAL) & (rough > 1e-6) & (ref["ok"] != 0), ref["mirror"][:, 0])):
        ax = np.abs(w[m])
        for v in (0.9, sp.down(0.9), sp.up(0.9)):
            assert (ax == v).sum() >= 10, (name, v)
        assert (ax > 0.9).sum() >= 100 and (ax <= 0.9).sum() >= 100, name
        assert (w[m] == 0.9).any() and (w[m] == -0.9).any(), name


def test_box_normals_are_asked_on_edges_corners_and_beside_them():
    T = sp.cases()
    box = np.array(sp.OBJECTS[4][1:3])
    for cls, least in (("box_edge", 2), ("box_corner", 3)):
        m = T["cls"] == sp.CLASSES.index(cls)
        p = T["hit"][m, 1:4]
        on = ((p == box[0]) | (p == box[1])).sum(axis=1)
        assert (on >= least).sum() >= 50, cls          # exactly on it: minDist ties decide the normal
        assert (on < least).sum() >= 50, cls           # a few ulps beside it
        n = T["hit"][m, 4:7]
        assert len(np.unique(n, axis=0)) == 6, cls     # every face wins somewhere
    # rays exactly perpendicular to the chosen normal: the reference calls that a back face
    d, n = T["ray"][:, 3:6], T["hit"][:, 4:7]
    perp = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1] + d[:, 2] * n[:, 2]) == 0
    assert perp.sum() >= 20 and not T["hit"][perp, 7].any()


def test_incidence_from_normal_to_grazing():
    T = sp.cases()
    sph = T["obj"] == 0
    d, n = T["ray"][sph, 3:6], T["hit"][sph, 4:7]
    cos = -np.sum(d * n, axis=1) / np.linalg.norm(d, axis=1)
    assert (cos > 0.999999).sum() >= 100 and ((cos > 0) & (cos < 1e-5)).sum() >= 20 and (T["hit"][sph, 7] == 0).sum() >= 1000


def test_roulette_table_reaches_every_outcome(oracle):
    R = sp.roulette_table()
    assert R["n"] % 64 != 0
    ref = oracle.roulette_steps(R["depth"], R["att"], R["T"], R["state"])
    cl = sp.roulette_classes(R, ref)
    count = {k: int(v.sum()) for k, v in cl.items()}
    print("roulette cases:", count)
    assert set(count) == set(sp.ROULETTE_CLASSES) and min(count.values()) >= 100
    # a draw equal to the survival probability survives, one ulp above it ends the path
    eq = np.flatnonzero(cl["draw_equals_prob"])
    assert np.isin(ref["ended"][eq], (0, 3)).all() and (ref["ended"][eq + 1] == 2).sum() >= 100   # the next case: down(xi) in the same slot
    assert set(np.unique(R["depth"])) == set(sp.ROULETTE_DEPTHS)
    # the maximum sits in each component in turn
    fin = ~np.isnan(R["att"]).any(axis=1)
    assert set(np.argmax(R["att"][fin], axis=1)) == {0, 1, 2}
    with np.errstate(all="ignore"):
        assert np.isinf(ref["T"]).any() and np.isnan(ref["T"]).any() and (ref["T"] == 0).any()


def test_exit_table_reaches_every_outcome(oracle):
    E, M = sp.exit_table(), sp.materials()
    assert E["n"] % 64 != 0
    att, orig = oracle.exit_steps(M["arr"], E["mat"], E["ray"], E["tmax"], E["best"], E["att"])
    none = E["best"] < 0
    assert none.sum() > 100 and np.all(att[none] == 1.0) and np.array_equal(orig[none], E["ray"][none, 0:3])
    moved = np.any(orig != E["ray"][:, 0:3], axis=1) | np.isnan(orig).any(axis=1)
    assert moved[~none].mean() > 0.5    # (a step of 1e-4 * 1e-150 moves nothing)
    a = att[~none]
    print("exit cases: %d, no exit %d, unchanged att %d, att 0 %d, att inf %d, att nan %d"
          % (E["n"], none.sum(), np.all(a == 1.0, axis=1).sum(), (a == 0).any(axis=1).sum(), np.isinf(a).any(axis=1).sum(), np.isnan(a).any(axis=1).sum()))
    assert np.all(a == 1.0, axis=1).sum() >= 100          # no positive absorption: the attenuation stays
    assert (a == 0).any(axis=1).sum() >= 100              # exp underflows
    assert np.isinf(a).any(axis=1).sum() >= 20            # a negative component next to a positive one, over a long way
    assert ((a > 0) & (a < 1)).any(axis=1).sum() >= 100
    assert set(np.unique(E["tmax"])) == {1e-4, 1.0, 1e3, 1e300}
