"""Whole frames with the edge materials of the surface-step probe (edge_materials_support.py) against the oracle, both
builds, through conftest.render_vs_oracle: the small scene (candidate bitmasks) in the default context, without split rounds and in
the wavefront pipeline; the large one (the hierarchy) in the default context and in the walk32 pipeline.  This is what the probe
cannot do: glass_kernel as the host launches it, and the way from pt_scene to DevMat on the device."""
from __future__ import annotations

import pytest

import edge_materials_support as em
from conftest import render_vs_oracle
from test_ray_inject_gpu import _context_with

pytestmark = pytest.mark.gpu

CONTEXTS = {"default": None, "split rounds 0": {"PTCORE_SPLIT_ROUNDS": "0"}, "wavefront": {"PTCORE_PIPELINE": "wavefront"},
            "walk32": {"PTCORE_PIPELINE": "walk32"}}
RUNS = ((False, ("default", "split rounds 0", "wavefront")), (True, ("default", "walk32")))


@pytest.fixture(scope="module")
def contexts(gpu_ctx):
    out = {name: gpu_ctx if env is None else _context_with(env) for name, env in CONTEXTS.items()}
    yield out
    for name, c in out.items():
        if name != "default":
            c.close()


@pytest.mark.parametrize("name", em.SET_NAMES)
def test_edge_material_frames_match_the_oracle(contexts, oracle, name):
    for large, forms in RUNS:
        o = em.oracle_frame(oracle, name, large)
        sc = em.product_scene(name, large)
        for form in forms:
            render_vs_oracle(contexts[form], sc, o, em.W, em.H, em.SPP, em.DEPTH, em.SEED, tag=(name, "large" if large else "small", form))
