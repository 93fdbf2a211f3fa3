"""A frame read before its first step, and after it (pt_begin, pt_read, pt_step, pt_read): finish_kernel's `zero` path and its
first real finish, plain and in an adaptive frame with moments.  37 x 21: two tiles, both cut in height, the second 5 pixels
wide, so the last block column and row hold out-of-frame slots.  The reference of the stepped frame is pt_render of the same
configuration, bit for bit; the oracle says that the scene has no non-finite radiance at these sizes, so that equal bits mean
equal numbers."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import scene_path

W, H, DEPTH, SEED = 37, 21, 4, 1
NAME = "example_simple"


def test_the_scene_has_no_non_finite_radiance(oracle):
    sc = oracle.Scene.load(scene_path(NAME))
    for spp in (2, 3):
        o = oracle.render(sc, W, H, spp, DEPTH, seed=SEED, want=("accum",))
        assert np.all(np.isfinite(o["accum"])), spp


def _begin_read_step_read(ctx, sc, spp):
    """pt_begin, pt_read (asserted empty), one pt_step of spp samples, pt_read: the image and the sums of that read."""
    from path_trace_golang_amd import capi, hip

    L = capi.load()
    flat = hip.FlatScene(sc)
    pc = hip.pt_config(hip.RenderConfig(W, H, spp, DEPTH, SEED))
    img = np.full((H, W, 4), 7, np.uint8)
    acc = np.full((H, W, 3), 7.0)
    capi.check(L.pt_begin(ctx.handle, C.byref(flat.c), C.byref(pc)))
    try:
        capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), W * 4, acc.ctypes.data_as(C.c_void_p)))
        assert np.all(img == np.array([0, 0, 0, 255], np.uint8)), "a frame without samples is black and opaque"
        assert not np.any(acc.view(np.uint64)), "a frame without samples has all-zero sums"
        done = C.c_int32(0)
        capi.check(L.pt_step(ctx.handle, spp, C.byref(done)))
        assert done.value == spp
        capi.check(L.pt_read(ctx.handle, img.ctypes.data_as(C.c_void_p), W * 4, acc.ctypes.data_as(C.c_void_p)))
    finally:
        capi.check(L.pt_end(ctx.handle, None))
    return img, acc


@pytest.mark.gpu
def test_read_before_and_after_the_first_step(gpu_ctx):
    from path_trace_golang_amd import capi, hip, scene

    sc = scene.load(scene_path(NAME))
    ref_img, ref_acc = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3))
    with capi.Context(ndev=1) as ctx:
        hip.render(sc, hip.RenderConfig(W, H, 3, DEPTH, SEED), ref_img, None, ref_acc, ctx=ctx)
        img, acc = _begin_read_step_read(ctx, sc, 3)
    assert np.any(ref_acc != 0.0)
    assert np.array_equal(img, ref_img)
    assert np.array_equal(acc.view(np.uint64), ref_acc.view(np.uint64))


@pytest.mark.gpu
def test_read_before_and_after_the_first_step_adaptive_with_moments(gpu_ctx):
    from path_trace_golang_amd import capi, hip, scene

    sc = scene.load(scene_path(NAME))
    target, step = 1e-3, 2
    ref_img, ref_acc = np.zeros((H, W, 4), np.uint8), np.zeros((H, W, 3))
    with capi.Context(ndev=1) as ctx:
        hip.render(sc, hip.RenderConfig(W, H, 2, DEPTH, SEED), ref_img, None, ref_acc, ctx=ctx, moments=np.zeros((H, W, 3)),
                   noise=target, adaptive=True, noise_step=step)
        hip.set_moments(ctx, True)  # (what that frame had on)
        hip.set_adaptive(ctx, target, 0, step)
        _, acc = _begin_read_step_read(ctx, sc, 2)
    assert np.any(ref_acc != 0.0)
    assert np.array_equal(acc.view(np.uint64), ref_acc.view(np.uint64))
