"""convert_material (csrc/pt_convert.h, the header ptcore.hip includes) against the oracle, on any machine: a g++ build of the header
with -ffp-contract=off, as the fog and GL host builds are made, over the material table of the surface-step probe
(shade_probe_support.materials: every field's edge values on every type, and a non-finite set).  Every DevMat field is compared on
its uint64 view, a NaN where the reference has one."""
from __future__ import annotations

import ctypes as C

import numpy as np

import shade_probe_support as sp


def _converted():
    M = sp.materials()
    out = np.zeros(M["n"], sp.DEVMAT)
    sp.convert_host().shim_convert(C.addressof(M["arr"]), M["n"], sp.ptr(out))
    return M, out


def test_material_layouts_agree(oracle):
    from path_trace_golang_amd import capi

    # the table is handed to the product as pt_material[]: the two structs are one layout
    assert C.sizeof(oracle.OraMaterial) == C.sizeof(capi.PtMaterial)
    for (a, _), (b, _) in zip(oracle.OraMaterial._fields_, capi.PtMaterial._fields_):
        assert getattr(oracle.OraMaterial, a).offset == getattr(capi.PtMaterial, b).offset


def test_table_holds_every_listed_value_on_every_type():
    M = sp.materials()
    assert M["n"] % 5 == 0 and np.array_equal(M["typ"], np.arange(M["n"]) % 5)
    for name, count in (("rough", len(sp.ROUGHS)), ("smoothness", len(sp.SMOOTHS)), ("ior", len(sp.IORS)), ("albedo", len(sp.ALBEDOS)),
                        ("emit", len(sp.EMITS)), ("absorption", len(sp.ABSORBS)), ("nonfinite", 33)):
        assert (M["set"] == name).sum() == 5 * count, name
    arr = M["arr"]
    raw = lambda f: np.array([getattr(arr[k], f) for k in range(M["n"])])
    for f, vals in (("rough", sp.ROUGHS), ("smoothness", sp.SMOOTHS), ("ior", sp.IORS)):
        have = set(sp.bits(raw(f)).tolist())
        assert set(sp.bits(np.array(vals)).tolist()) <= have, f
    for f in ("rough", "smoothness", "ior", "power"):
        x = raw(f)[~M["finite"]]
        assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any(), f
    emit = M["conv"][M["typ"] == sp.EMISSIVE, 6:9]
    assert np.isinf(emit).any() and (emit < 0).any() and np.any(np.all(emit == 0, axis=1))   # emit * power overflows, is negative, is 0


def test_convert_material_equals_the_reference_field_by_field(oracle):
    M, dev = _converted()
    L = oracle.lib()
    der = np.zeros((M["n"], 5))
    for k in range(M["n"]):
        L.ora_material_derived(C.byref(M["arr"][k]), der[k].ctypes.data_as(C.POINTER(C.c_double)))
    conv = M["conv"]
    assert np.array_equal(dev["typ"], conv[:, 0].astype(np.int32))
    bad = {}
    for name, ref in (("albedo", conv[:, 1:4]), ("rough", conv[:, 4]), ("ior", conv[:, 5]), ("emit", conv[:, 6:9]),
                      ("absorption", conv[:, 9:12]), ("rough_sq", der[:, 3])):   # rough * rough (materials.go:121)
        bad[name] = int((~sp.same(dev[name], ref)).sum())
    # 1 / ior and reflectance's r0 with ratio = 1 / ior and with ratio = ior (materials.go:183, :227-228), as the reference forms
    # them on every dielectric hit; the other types never read them and keep the zero the record started with
    diel = M["typ"] == sp.DIELECTRIC
    for name, col in (("inv_ior", 0), ("r0_front", 1), ("r0_back", 2)):
        bad[name] = int((~sp.same(dev[name][diel], der[diel, col])).sum()) + int(np.any(sp.bits(dev[name][~diel]) != 0))
    bad["absorbs"] = int((dev["absorbs"] != der[:, 4].astype(np.int32)).sum())   # renderer.go:360's test
    print("convert_material: %d materials, fields that differ: %s" % (M["n"], bad))
    assert not any(bad.values()), bad
    # the cases that make the comparison worth having: 1 + ior == 0, ior at the ends of the range, ior 0 -> 1.5
    assert np.isinf(dev["r0_back"][diel]).any() and np.isnan(dev["r0_front"][diel]).any()
    assert (dev["ior"][diel] == 1.5).sum() > 10 and (dev["inv_ior"][diel] == np.inf).any() and (dev["inv_ior"][diel] == 0).any()
    assert dev["absorbs"][diel].min() == 0 and dev["absorbs"][diel].max() == 1 and not dev["absorbs"][~diel].any()


def test_front_and_back_r0_differ_where_a_swap_would_show():
    _, dev = _converted()
    diel = dev["typ"] == sp.DIELECTRIC
    assert (sp.bits(dev["r0_front"][diel]) != sp.bits(dev["r0_back"][diel])).sum() > 20
