"""ptd::LdsLayout (csrc/pt_device.h) is the one description of the dynamic LDS of trace_kernel's flat scans and of glass_kernel: the
host sizes the launches from it and the kernels take their pointers from it.  Here a stand-alone C++ program prints it for a table of
counts, and the figures are held to the expressions the host and the kernels each wrote out by hand before the struct existed."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

OBJ, MAT, INT = 80, 128, 4  # sizeof(DevObj), sizeof(DevMat), sizeof(int): static_asserts of pt_device.h

#        nobj nmat n_bsph n_bbox n_dsph n_dbox
CASES = [(3, 2, 0, 0, 0, 0),        # no records at all (planes only)
         (1, 2, 1, 0, 0, 0),        # one record; index count 1 mod 4
         (65, 4, 32, 32, 10, 11),   # 32 + 32 full records; 85 = 1 mod 4, dielectric tables 21 = 1 mod 4
         (5, 3, 1, 1, 0, 0),        # index count 2 mod 4; no dielectric record
         (6, 3, 2, 1, 0, 0),        # index count 3 mod 4
         (7, 3, 3, 2, 1, 1),        # 7 = 3 mod 4 in the trace shape, 2 mod 4 in the glass shape
         (9, 4, 4, 3, 2, 1),        # 10 = 2 mod 4 / 3 mod 4
         (4, 2, 2, 2, 2, 2),        # every record dielectric; index count 0 mod 4: no pad
         (5, 2, 3, 1, 1, 0),        # odd nobj, even nmat
         (4, 3, 2, 1, 0, 1)]        # even nobj, odd nmat


def align16(v):
    return (v + 15) & ~15


def parent_host(nobj, nmat, nbs, nbb, nds, ndb, ro):
    """world_lds, sd.lds_bytes (flat branch) and sd.glass_lds_bytes as scene_prepare computed them."""
    world_lds = nobj * OBJ + nmat * MAT + (nbs + nbb + nds + ndb) * INT
    lds = nobj * OBJ + nmat * MAT + (nbs + nbb + nds + ndb) * INT
    if ro:
        lds = align16(lds) + (nbs + nbb + nds + ndb) * OBJ
    glass = nobj * OBJ + nmat * MAT + (nds + ndb) * INT
    if ro:
        glass = align16(glass) + (nds + ndb) * OBJ
    return world_lds, lds, glass


def parent_kernels(nobj, nmat, nbs, nbb, nds, ndb):
    """The pointer arithmetic of trace_kernel (with its nested exit search) and of glass_kernel, as byte offsets into smem."""
    t = {"mat": nobj * OBJ,
         "kidx": nobj * OBJ + nmat * MAT,
         "kidx_diel": nobj * OBJ + nmat * MAT + (nbs + nbb) * INT,                       # lds_kidx + n_bsph + n_bbox
         "rec": align16(nobj * OBJ + nmat * MAT + (nbs + nbb + nds + ndb) * INT)}
    t["rec_diel"] = t["rec"] + (nbs + nbb) * OBJ                                         # lds_rec + n_bsph + n_bbox
    g = {"mat": nobj * OBJ,
         "kidx_diel": nobj * OBJ + nmat * MAT,                                           # glass_kernel's lds_kidx
         "rec_diel": align16(nobj * OBJ + nmat * MAT + (nds + ndb) * INT)}                # glass_kernel's lds_rec
    return t, g


def _build(tmp, flags, name):
    exe = os.path.join(tmp, name)
    cxx = os.environ.get("CXX") or shutil.which("g++") or "g++"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + os.path.join(ROOT, "path_trace_golang_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lds_layout_probe.cpp"), "-o", exe], check=True)
    return exe


def _run(exe):
    args = [str(v) for c in CASES for v in c]
    r = subprocess.run([exe, *args], check=True, capture_output=True, text=True)
    assert r.stderr == "", r.stderr  # a sanitizer report goes there
    rows = {}
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 4 * len(CASES)
    for i, ln in enumerate(lines):
        f = ln.split()
        rows[(CASES[i // 4], f[0], int(f[1]))] = dict(zip(("mat", "kidx", "kidx_diel", "world", "rec", "rec_diel", "total"), map(int, f[2:])))
    return rows


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    return _run(_build(str(tmp_path_factory.mktemp("lds_layout")), [], "lds_layout_probe"))


@pytest.mark.parametrize("case", CASES)
def test_layout_gives_the_sizes_the_host_computed_and_the_offsets_the_kernels_computed(layouts, case):
    nobj, nmat, nbs, nbb, nds, ndb = case
    kt, kg = parent_kernels(*case)
    for ro in (0, 1):
        world_lds, lds, glass = parent_host(*case, ro)
        t, g = layouts[(case, "trace", ro)], layouts[(case, "glass", ro)]
        assert t["world"] == world_lds  # leaves the record-order copy out whatever `ro`: it decides wide_ok against 30 KiB
        assert t["total"] == lds and g["total"] == glass
        for k, v in kt.items():
            assert t[k] == v, (k, ro)
        for k, v in kg.items():
            assert g[k] == v, (k, ro)


@pytest.mark.parametrize("case", CASES)
def test_regions_do_not_overlap_and_end_at_the_total(layouts, case):
    nobj, nmat, nbs, nbb, nds, ndb = case
    t = layouts[(case, "trace", 1)]
    # each region is exactly as long as what is staged into it, in this order, and the last one ends at the total
    assert t["mat"] == nobj * OBJ
    assert t["kidx"] - t["mat"] == nmat * MAT
    assert t["kidx_diel"] - t["kidx"] == (nbs + nbb) * INT
    assert t["world"] - t["kidx_diel"] == (nds + ndb) * INT
    assert t["world"] <= t["rec"] < t["world"] + 16 and t["rec"] % 16 == 0
    assert t["rec_diel"] - t["rec"] == (nbs + nbb) * OBJ
    assert t["total"] - t["rec_diel"] == (nds + ndb) * OBJ
    # without the record-order copies the launch ends behind the tables
    assert layouts[(case, "trace", 0)]["total"] == t["world"]
    # the glass shape has no full tables: its records sit behind the two dielectric tables only
    g = layouts[(case, "glass", 1)]
    assert g["kidx"] == g["kidx_diel"] == nobj * OBJ + nmat * MAT
    assert g["world"] == g["kidx_diel"] + (nds + ndb) * INT
    assert g["rec"] == g["rec_diel"] == align16(g["world"])
    assert g["total"] == g["rec_diel"] + (nds + ndb) * OBJ
    assert layouts[(case, "glass", 0)]["total"] == g["world"]


def test_the_cases_reach_every_pad():
    """nobj * 80 + nmat * 128 is a multiple of 16, so the pad in front of the record-order copy is 16 - 4 * (index count mod 4)."""
    pads_t = {align16(parent_host(*c, 0)[0]) - parent_host(*c, 0)[0] for c in CASES}
    pads_g = {align16(parent_host(*c, 0)[2]) - parent_host(*c, 0)[2] for c in CASES}
    assert pads_t == {0, 4, 8, 12} and pads_g >= {4, 8, 12}


def test_probe_is_clean_under_asan_and_ubsan(tmp_path, layouts):
    """Host code on the CPU: the same program once more with the sanitizers, run stand-alone."""
    exe = _build(str(tmp_path), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "lds_layout_probe_san")
    assert _run(exe) == layouts
