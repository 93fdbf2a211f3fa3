"""The object index plane on the MI355X (pt_set_object_ids, pt_read_object_ids, the id store of feature_kernel).
The reference is tests/object_ids_reference.c on the oracle: ora_primary_ray's sample 0 of every pixel against the scene's objects
in file order.  Frames are small (40 x 24: two tiles, ragged; 37 x 21; 70 x 45 for the gather); every comparison runs with contexts
of its own."""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest

import adaptive_support as ad
import moments_support as ms
import temporal_motion_support as tm
from conftest import render_vs_oracle, scene_path
from moments_support import H, W

pytestmark = pytest.mark.gpu

SPP = 4
ID_SCENES = [("example_simple", 4), ("gpu_showcase", 4), ("metal_glass_room", 4)]  # the last two have a thin lens


@pytest.fixture(autouse=True, scope="module")
def _built(gpu_ctx):
    return gpu_ctx


def _doc(name):
    if name == "unknown in the middle":
        return tm.doc_with_an_unknown_object("example_simple")
    with open(scene_path(name), "r", encoding="utf-8") as fh:
        return json.load(fh)


def _scene(name):
    from path_trace_golang_amd import scene

    return scene.Scene.decode(_doc(name))


def _frame(ctx, sc, w, h, spp, depth, k=2, seed=1, chunk=0, **kw):
    """One frame with moments, k feature samples and object ids on: dict(ids, img, st)."""
    from path_trace_golang_amd import hip

    img, acc, m2 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    st = hip.render(sc, hip.RenderConfig(w, h, spp, depth, seed, chunk), img, None, acc, ctx=ctx, moments=m2, features=k, object_ids=True, **kw)
    ids = np.full((h, w), -9, np.int32)
    hip.read_object_ids(ctx, ids)
    return dict(ids=ids, img=img, st=st)


def _oracle_ids(name, w, h, seed=1):
    from oracle import ora

    return tm.oracle_ids(ora.Scene(_doc(name)), w, h, seed)


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("name,depth", ID_SCENES + [("unknown in the middle", 4)])
def test_ids_match_the_oracle(name, depth):
    from path_trace_golang_amd import capi

    sc = _scene(name)
    with capi.Context(ndev=1) as ctx:
        for (w, h) in ((W, H), (37, 21)):
            got = _frame(ctx, sc, w, h, SPP, depth)["ids"]
            want, tie = _oracle_ids(name, w, h)
            assert not tie.any(), (name, int(tie.sum()))
            assert np.array_equal(got, want), (name, w, h, int(np.count_nonzero(got != want)))
            assert len(np.unique(got)) > 4 and got.min() >= -1 and got.max() < len(sc.objects)
    if name == "unknown in the middle":
        assert 5 not in set(got.reshape(-1).tolist()) and got.max() > 5


# ---------------------------------------------------------------- 2. invariance, bit for bit
INV = ("metal_glass_room", 4, 6)  # scene, depth, k


@pytest.fixture(scope="module")
def inv_ref(_built):
    from path_trace_golang_amd import capi

    name, depth, k = INV
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, _scene(name), W, H, 16, depth, k)
    assert np.array_equal(f["ids"], _oracle_ids(name, W, H)[0])
    return f


@pytest.mark.parametrize("chunk", [3, 5])
def test_ids_do_not_depend_on_the_chunk(inv_ref, chunk):
    from path_trace_golang_amd import capi

    name, depth, k = INV
    with capi.Context(ndev=1) as ctx:
        f = _frame(ctx, _scene(name), W, H, 16, depth, k, chunk=chunk)
    assert f["st"]["spp_chunk"] == chunk and np.array_equal(f["ids"], inv_ref["ids"]) and np.array_equal(f["img"], inv_ref["img"])


@pytest.mark.parametrize("step", [1, 7])
def test_ids_do_not_depend_on_the_steps(inv_ref, step):
    from path_trace_golang_amd import capi, hip

    name, depth, k = INV
    L = capi.load()
    flat = hip.FlatScene(_scene(name))
    pc = hip.pt_config(hip.RenderConfig(W, H, 16, depth, 1))
    ids = np.full((H, W), -9, np.int32)
    with capi.Context(ndev=1) as ctx:
        hip.set_moments(ctx, True)
        hip.set_features(ctx, k)
        hip.set_object_ids(ctx, True)
        capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
        assert L.pt_set_object_ids(ctx.handle, 0) == capi.PT_ERR_STATE and b"frame is open" in L.pt_last_error()
        done = C.c_int32(0)
        while done.value < 16:
            capi.check(L.pt_step(ctx.handle, step, C.byref(done)))
            if done.value == step:  # the plane is complete after the first step: it is sample 0's
                hip.read_object_ids(ctx, ids)
                assert np.array_equal(ids, inv_ref["ids"])
                ids[:] = -9
        capi.check(L.pt_end(ctx.handle, None))
        hip.read_object_ids(ctx, ids)
    assert np.array_equal(ids, inv_ref["ids"])


@pytest.mark.parametrize("env", [{"PTCORE_PIPELINE": "wavefront"}, {"PTCORE_SCAN": "uniform"}], ids=["wavefront", "uniform"])
def test_ids_do_not_depend_on_the_trace_form(monkeypatch, inv_ref, env):
    from path_trace_golang_amd import capi

    name, depth, k = INV
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    with capi.Context(ndev=1) as ctx:  # both are read by pt_create
        f = _frame(ctx, _scene(name), W, H, 16, depth, k)
    assert np.array_equal(f["ids"], inv_ref["ids"]) and np.array_equal(f["img"], inv_ref["img"])


def test_an_adaptive_frame_has_the_ids_of_the_plain_one():
    from path_trace_golang_amd import capi, hip

    name, depth, seed, cap, step, min_spp, target = ad.CASE
    sc = _scene(name)
    with capi.Context(ndev=1) as ctx:
        hip.set_features(ctx, 4)
        _, _, _, counts, _, _, _ = ad.render_adaptive(ctx, sc, W, H, cap, depth, seed, target, step, min_spp, features=4, object_ids=True)
        assert counts.tolist() == ad.expand(ad.CASE_MAP).tolist()
        ids = np.full((H, W), -9, np.int32)
        hip.read_object_ids(ctx, ids)
    assert np.array_equal(ids, _oracle_ids(name, W, H, seed)[0])


def test_four_virtual_devices_gather_the_plane_of_one():
    from path_trace_golang_amd import capi

    name, depth = "example_simple", 4
    w, h = ad.GATHER_W, ad.GATHER_H  # 70 x 45: 6 tiles = 2, 2, 1, 1
    sc = _scene(name)
    with capi.Context(ndev=1) as one, capi.Context(devices=[0, 0, 0, 0]) as four:
        a = _frame(one, sc, w, h, SPP, depth)
        b = _frame(four, sc, w, h, SPP, depth)
        assert b["st"]["num_devices"] == 4
    want, tie = _oracle_ids(name, w, h)
    assert not tie.any() and np.array_equal(a["ids"], want) and np.array_equal(b["ids"], want)


def _edge_rays(doc, n):
    """n rays from the camera's position at the silhouettes of the scene's spheres (tangent, and a hair inside and outside) and at the
    corners and edge midpoints of its boxes."""
    cam = doc["camera"]["position"]
    o = np.array([cam["x"], cam["y"], cam["z"]], float)
    out = []
    for ob in doc["objects"]:
        c = np.array([ob["position"][a] for a in "xyz"], float)
        s = np.array([ob["size"][a] for a in "xyz"], float)
        if ob["type"] in ("sphere", "sphere_light"):
            to = c - o
            dist = np.linalg.norm(to)
            side = np.cross(to, [0.0, 1.0, 0.0])
            side /= np.linalg.norm(side)
            up = np.cross(side, to / dist)
            for t in (side, -side, up, -up):
                for f in (1.0, 1.0 - 1e-12, 1.0 + 1e-12, 0.999, 1.001):
                    # the tangent point of a ray from o: at angle asin(r / dist) off the axis
                    sin = s[0] / dist * f
                    if sin < 1:
                        out.append(np.concatenate([o, to / dist * np.sqrt(1 - sin * sin) + t * sin]))
        elif ob["type"] == "box":
            lo, hi = c - s / 2, c + s / 2
            for fx in (0.0, 0.5, 1.0):
                for fy in (0.0, 0.5, 1.0):
                    for fz in (0.0, 0.5, 1.0):
                        if (fx == 0.5) + (fy == 0.5) + (fz == 0.5) <= 1:  # corners and edge midpoints
                            p = lo + (hi - lo) * np.array([fx, fy, fz])
                            out.append(np.concatenate([o, p - o]))
    out = np.array(out)
    assert 64 < len(out)
    reps = -(-n // len(out))
    return np.tile(out, (reps, 1))[:n]


def test_injected_rays_at_object_edges_give_the_ids_of_the_injected_rays():
    from oracle import ora
    from path_trace_golang_amd import capi, hip

    name, depth, spp = "example_simple", 4, 2
    doc = _doc(name)
    sc = _scene(name)
    edge = _edge_rays(doc, W * H)
    rays = np.repeat(edge, spp, axis=0)
    rays[1::spp, 3:6] = [0.0, 1.0, 0.0]  # sample 1 looks at the sky: the id must be sample 0's
    want, tie = tm.oracle_ids_of_rays(ora.Scene(doc), edge)
    with capi.Context(ndev=1) as ctx:
        ctx.set_primary_rays(rays)
        try:
            got = _frame(ctx, sc, W, H, spp, depth)["ids"].reshape(-1)
        finally:
            ctx.set_primary_rays(None)
        camera = _frame(ctx, sc, W, H, spp, depth)["ids"]  # ... and the camera's again once the table is cleared
    keep = ~tie
    print("edge rays: %d, %d ties, %d hits, %d distinct objects" % (len(edge), int(tie.sum()), int((want >= 0).sum()), len(np.unique(want))))
    assert keep.sum() > len(edge) * 0.9 and len(np.unique(want)) > 10 and (want == -1).any()
    assert np.array_equal(got[keep], want[keep]), int(np.count_nonzero(got[keep] != want[keep]))
    assert np.array_equal(camera, _oracle_ids(name, W, H)[0])


# ---------------------------------------------------------------- 3. refusals
def test_state_rules_and_every_refusal_leaves_a_usable_context(oracle):
    from path_trace_golang_amd import capi, hip, synth

    L = capi.load()
    name, depth = "example_simple", 4
    sc = _scene(name)
    o = oracle.render(ms.ora_scene(name), W, H, SPP, depth, seed=1)
    flat = hip.FlatScene(sc)
    ids = np.full((H, W), -9, np.int32)
    ip = ids.ctypes.data_as(C.POINTER(C.c_int32))
    img = np.zeros((H, W, 4), np.uint8)
    with capi.Context(ndev=1) as ctx:
        assert L.pt_read_object_ids(ctx.handle, ip) == capi.PT_ERR_STATE  # no frame yet
        # ids on, features off: refused before anything is launched
        hip.set_moments(ctx, True)
        hip.set_features(ctx, 0)
        hip.set_object_ids(ctx, True)
        pc = hip.pt_config(hip.RenderConfig(W, H, SPP, depth, 1))
        assert L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)) == capi.PT_ERR_INVALID and b"object ids" in L.pt_last_error()
        assert L.pt_render(ctx.handle, C.byref(flat.c), C.byref(pc), img.ctypes.data_as(C.c_void_p), W * 4, None, None, None, None) == capi.PT_ERR_INVALID
        assert L.pt_read_object_ids(ctx.handle, ip) == capi.PT_ERR_STATE
        # a frame with features and ids off records none
        hip.set_object_ids(ctx, False)
        hip.render(sc, hip.RenderConfig(W, H, SPP, depth, 1), img, ctx=ctx, moments=np.zeros((H, W, 3)), features=2)
        assert L.pt_read_object_ids(ctx.handle, ip) == capi.PT_ERR_STATE and b"object ids off" in L.pt_last_error()
        assert L.pt_read_object_ids(ctx.handle, None) == capi.PT_ERR_INVALID
        # moments off: pt_read_features' own refusal
        hip.render(sc, hip.RenderConfig(W, H, SPP, depth, 1), img, ctx=ctx, features=2, object_ids=True)
        assert L.pt_read_object_ids(ctx.handle, ip) == capi.PT_ERR_STATE and b"moments" in L.pt_last_error()
        # the features' own refusals: GL shading, the hierarchy path
        with pytest.raises(capi.PtError, match="GL shading"):
            hip.render(sc, hip.RenderConfig(W, H, 1, depth, 1), img, ctx=ctx, shading="gl", moments=np.zeros((H, W, 3)), features=2, object_ids=True)
        # ... 300 objects lie on the hierarchy path: ids on with k > 0 is the features' refusal, through pt_begin and through hip.render
        big = synth.make_scene(300)
        bigflat = hip.FlatScene(big)
        hip.set_shading(ctx, "cpu")
        hip.set_moments(ctx, True)
        hip.set_features(ctx, 2)
        hip.set_object_ids(ctx, True)
        pcb = hip.pt_config(hip.RenderConfig(W, H, 4, 3, 1))
        assert L.pt_begin(ctx.handle, C.byref(bigflat.c), C.byref(pcb)) == capi.PT_ERR_INVALID and b"BVH" in L.pt_last_error()
        assert L.pt_read_object_ids(ctx.handle, ip) == capi.PT_ERR_STATE
        with pytest.raises(capi.PtError, match="BVH"):
            hip.render(big, hip.RenderConfig(W, H, 4, 3, 1), img, ctx=ctx, moments=np.zeros((H, W, 3)), features=2, object_ids=True)
        assert L.pt_read_object_ids(ctx.handle, ip) == capi.PT_ERR_STATE
        # the same scene without features and ids renders
        hip.render(big, hip.RenderConfig(W, H, 4, 3, 1), img, ctx=ctx, moments=np.zeros((H, W, 3)))
        assert L.pt_read_object_ids(ctx.handle, ip) == capi.PT_ERR_STATE and img[..., 3].min() == 255
        assert (ids == -9).all()  # no refused read wrote anything
        # ... and the context is usable: an oracle-exact frame with the ids of the oracle
        got = _frame(ctx, sc, W, H, SPP, depth)
        assert np.array_equal(got["ids"], _oracle_ids(name, W, H)[0])
        hip.set_object_ids(ctx, False)
        hip.set_features(ctx, 0)
        hip.set_moments(ctx, False)
        render_vs_oracle(ctx, sc, o, W, H, SPP, depth, 1, tag="at the end")


def test_tiles_device_neither_collects_nor_fails():
    import torch

    from path_trace_golang_amd import capi, hip

    L = capi.load()
    sc = _scene("example_simple")
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(W, H, 2, 2, 1))
    ntiles = ((W + 31) // 32) * ((H + 31) // 32)
    rgba = torch.zeros(ntiles * 1024 * 4, dtype=torch.uint8, device=torch.device("cuda", 0))
    ids = np.full((H, W), -9, np.int32)
    with capi.Context(ndev=1) as ctx:
        hip.set_object_ids(ctx, True)  # with features off: pt_begin would refuse, this entry point does not look
        capi.check(L.pt_render_tiles_device(ctx.handle, C.byref(flat.c), C.byref(pc), None, C.c_void_p(rgba.data_ptr()), None, None, None))
        torch.cuda.synchronize()
        assert L.pt_read_object_ids(ctx.handle, ids.ctypes.data_as(C.POINTER(C.c_int32))) == capi.PT_ERR_STATE
        assert (ids == -9).all() and int(rgba.count_nonzero()) > 0
