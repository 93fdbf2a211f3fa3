"""Every refusal of pt_atrous, pt_atrous_halves and pt_temporal, by the whole text of pt_last_error() and by the code returned.

The expected strings below were copied from the source text of csrc/ptcore.hip as it stood before the filter host was rewritten
around one configuration check, one table of frame conditions and one launch sequence -- not from running the
library.  The other tests look for a few words of a message; this one pins what such a rewrite could silently reword, and, with the
two calls that are wrong in two ways, which of two refusals comes first.  One shipped scene at 16 x 8, 4 samples, depth 2; after the
refusals the context still renders the oracle's frame."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import adaptive_support as ad
import atrous_support as at
import moments_support as ms
import temporal_support as ts
from conftest import render_vs_oracle, scene_path

pytestmark = pytest.mark.gpu

NAME, W, H, SPP, DEPTH, SEED = "example_simple", 16, 8, 4, 2, 1
ENTRY_POINTS = ("pt_atrous", "pt_atrous_halves", "pt_temporal")

NO_FRAME = "%s: no frame with samples on this context (pt_step or pt_render first)"
MOMENTS_OFF = "%s: the frame was rendered with moments off (pt_set_moments)"
HALVES_OFF = "pt_atrous_halves: the frame was rendered with halves off (pt_set_halves)"
FEATURES_OFF = "pt_temporal: the frame was rendered with features off (pt_set_features)"
GL_FRAME = "%s: not available for a frame rendered with GL shading (pt_set_shading)"
TWO_SAMPLES = "%s: every pixel needs at least 2 samples"
FOUR_SAMPLES = "pt_atrous_halves: every pixel needs at least 4 samples (the frame's smallest count is %d)"
STRIDE = "stride smaller than 4*width"
ACCUMULATED = "pt_temporal: already accumulated (this frame, at this number of samples, is in the history)"
TEMPORAL_CONFIG = "pt_temporal: alpha must be 0..1, tol_z and tol_a >= 0, n_min a number, max_len >= 1"
# the two wordings of a bad filter configuration x the three prefixes
ITERATIONS = {"pt_atrous": "pt_atrous: iterations must be 0..6", "pt_atrous_halves": "pt_atrous_halves: iterations must be 0..6",
              "pt_temporal": "pt_temporal: filter iterations must be 0..6"}
SIGMAS = {"pt_atrous": "pt_atrous: sigma_l must be > 0, sigma_n, sigma_z and sigma_a >= 0 (0 = term off)",
          "pt_atrous_halves": "pt_atrous_halves: sigma_l must be > 0, sigma_n, sigma_z and sigma_a >= 0 (0 = term off)",
          "pt_temporal": "pt_temporal: filter sigma_l must be > 0, sigma_n, sigma_z and sigma_a >= 0 (0 = term off)"}
BAD_FILTERS = ((dict(iterations=7), ITERATIONS), (dict(iterations=-1), ITERATIONS), (dict(sigma_l=0.0), SIGMAS),
               (dict(sigma_l=float("nan")), SIGMAS), (dict(sigma_n=-0.1), SIGMAS), (dict(sigma_n=float("nan")), SIGMAS),
               (dict(sigma_z=-0.1), SIGMAS), (dict(sigma_z=float("nan")), SIGMAS), (dict(sigma_a=-1.0), SIGMAS),
               (dict(sigma_a=float("nan")), SIGMAS))
BAD_TEMPORAL = (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(tol_z=-1.0), dict(tol_z=float("nan")), dict(tol_a=-1.0),
                dict(tol_a=float("nan")), dict(n_min=float("nan")), dict(max_len=0))


def test_every_refusal_has_the_text_and_the_code_it_had(gpu_ctx, oracle):
    from path_trace_golang_amd import capi, hip, scene

    L = capi.load()
    sc = scene.load(scene_path(NAME))
    img = np.zeros((H, W, 4), np.uint8)
    rgba = img.ctypes.data_as(C.c_void_p)
    wrong = []

    def call(ctx, who, flt=None, tcfg=None, stride=0):
        f = C.byref(flt) if flt is not None else None
        out = rgba if stride else None
        if who == "pt_atrous":
            return L.pt_atrous(ctx.handle, f, out, stride, None, None, None)
        if who == "pt_atrous_halves":
            return L.pt_atrous_halves(ctx.handle, f, None, None, None, None)
        return L.pt_temporal(ctx.handle, C.byref(tcfg) if tcfg is not None else None, f, out, stride, None, None, None)

    def refused(ctx, who, code, text, what, **kw):
        rc = call(ctx, who, **kw)
        got = L.pt_last_error().decode() if rc != capi.PT_OK else ""
        if rc != code or got != text:
            wrong.append((what, who, rc, got, code, text))

    def frame(ctx, spp=SPP, **kw):
        return hip.render(sc, hip.RenderConfig(W, H, spp, DEPTH, SEED), img, ctx=ctx, **kw)

    def full(ctx, spp=SPP):  # a frame every entry point accepts
        return frame(ctx, spp, moments=np.zeros((H, W, 3)), features=4, halves=True)

    with capi.Context(ndev=1) as ctx:
        for who in ENTRY_POINTS:
            refused(ctx, who, capi.PT_ERR_STATE, NO_FRAME % who, "no frame")
        frame(ctx)
        for who in ENTRY_POINTS:
            refused(ctx, who, capi.PT_ERR_STATE, MOMENTS_OFF % who, "moments off")
        frame(ctx, moments=np.zeros((H, W, 3)))
        refused(ctx, "pt_atrous_halves", capi.PT_ERR_STATE, HALVES_OFF, "halves off")
        refused(ctx, "pt_temporal", capi.PT_ERR_STATE, FEATURES_OFF, "features off")
        assert call(ctx, "pt_atrous") == capi.PT_OK  # (needs neither)

        # a frame all three accept: the bad configurations, the short stride, the second accumulation
        full(ctx)
        for bad, texts in BAD_FILTERS:
            c = dict(at.DEFAULTS, **bad)
            flt = capi.PtAtrousConfig(c["iterations"], 0, c["sigma_l"], c["sigma_n"], c["sigma_z"], c["sigma_a"])
            for who in ENTRY_POINTS:
                refused(ctx, who, capi.PT_ERR_INVALID, texts[who], bad, flt=flt)
        for bad in BAD_TEMPORAL:
            c = dict(ts.T_DEFAULTS, **bad)
            tcfg = capi.PtTemporalConfig(c["alpha"], c["tol_z"], c["n_min"], c["tol_a"], c["max_len"], 0)
            refused(ctx, "pt_temporal", capi.PT_ERR_INVALID, TEMPORAL_CONFIG, bad, tcfg=tcfg)
        for who in ("pt_atrous", "pt_temporal"):
            refused(ctx, who, capi.PT_ERR_INVALID, STRIDE, "short stride", stride=W * 4 - 1)
        for who in ENTRY_POINTS:
            assert call(ctx, who, stride=W * 4) == capi.PT_OK, (who, L.pt_last_error())
        refused(ctx, "pt_temporal", capi.PT_ERR_STATE, ACCUMULATED, "already accumulated")

        # too few samples: one, three, and the adaptive frame whose blocks all stop at three
        full(ctx, 1)
        refused(ctx, "pt_atrous", capi.PT_ERR_STATE, TWO_SAMPLES % "pt_atrous", "1 sample")
        refused(ctx, "pt_temporal", capi.PT_ERR_STATE, TWO_SAMPLES % "pt_temporal", "1 sample")
        refused(ctx, "pt_atrous_halves", capi.PT_ERR_STATE, FOUR_SAMPLES % 1, "1 sample")
        full(ctx, 3)
        refused(ctx, "pt_atrous_halves", capi.PT_ERR_STATE, FOUR_SAMPLES % 3, "3 samples")
        counts = ad.render_adaptive(ctx, sc, W, H, 12, DEPTH, SEED, 1e9, 3, 0, halves=True)[3]
        assert counts.min() == 3
        refused(ctx, "pt_atrous_halves", capi.PT_ERR_STATE, FOUR_SAMPLES % 3, "adaptive, count 3")

        # a GL frame; with a short stride as well, pt_atrous names the frame and pt_temporal the stride
        frame(ctx, shading="gl", moments=np.zeros((H, W, 3)), halves=True)
        for who in ENTRY_POINTS:
            refused(ctx, who, capi.PT_ERR_STATE, GL_FRAME % who, "GL frame")
        refused(ctx, "pt_atrous", capi.PT_ERR_STATE, GL_FRAME % "pt_atrous", "GL frame and short stride", stride=W * 4 - 1)
        refused(ctx, "pt_temporal", capi.PT_ERR_INVALID, STRIDE, "GL frame and short stride", stride=W * 4 - 1)

        for w in wrong:
            print("%s, %s: got %d %r, want %d %r" % w)
        assert not wrong, "%d refusals differ" % len(wrong)
        o = oracle.render(ms.ora_scene(NAME), W, H, SPP, DEPTH, seed=SEED)
        render_vs_oracle(ctx, sc, o, W, H, SPP, DEPTH, SEED, tag="after the refusals")
