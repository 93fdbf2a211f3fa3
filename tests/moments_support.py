"""Helpers of the second-moment tests (test_moments_cpu.py, test_moments_gpu.py): the oracle's per-sample radiances of a
40 x 24 frame, computed once per (scene, depth, seed) and shared, and the sums and the noise figure derived from them."""
from __future__ import annotations

import numpy as np

from conftest import scene_path

W, H = 40, 24  # two tiles wide, the second 8 pixels wide, both cut in height: out-of-frame slots in every block row

_samples = {}
_scenes = {}


def ora_scene(name):
    from oracle import ora

    if name not in _scenes:
        _scenes[name] = ora.Scene.load(scene_path(name))
    return _scenes[name]


def samples(name: str, depth: int, seed: int, n: int) -> np.ndarray:
    """The oracle's radiance of samples 0..n-1 of every pixel, float64 [H, W, n, 3] (read-only; a longer list computed
    earlier for the same scene, depth and seed is reused: a sample does not depend on the frame's sample count)."""
    from oracle import ora

    key = (name, depth, seed)
    have = _samples.get(key)
    if have is None or have.shape[2] < n:
        sc = ora_scene(name)
        a = np.empty((H, W, n, 3), np.float64)
        k0 = 0
        if have is not None:
            k0 = have.shape[2]
            a[:, :, :k0] = have
        for y in range(H):
            for x in range(W):
                for s in range(k0, n):
                    a[y, x, s] = ora.sample(sc, W, H, n, depth, seed, x, y, s)[0]
        a.setflags(write=False)
        _samples[key] = have = a
    return have[:, :, :n]


def sums(l: np.ndarray):
    """(S, Q) = per pixel and channel the sums of l and of l*l over the samples, added in sample order from zero."""
    S = np.zeros(l.shape[:2] + (3,), np.float64)
    Q = np.zeros_like(S)
    for s in range(l.shape[2]):
        S = S + l[:, :, s]
        Q = Q + l[:, :, s] * l[:, :, s]
    return S, Q


def noise_restated(S: np.ndarray, Q: np.ndarray, n: int) -> dict:
    """The metric of include/ptcore.h, pixel by pixel in plain Python floats (independent of hip.noise_estimate_host)."""
    import math

    total, worst, bad, pixels = 0.0, 0.0, 0, 0
    for y in range(S.shape[0]):
        for x in range(S.shape[1]):
            pixels += 1
            m = [float(S[y, x, c]) / n for c in range(3)]
            d = [float(Q[y, x, c]) / n - m[c] * m[c] for c in range(3)]
            v = [(0.0 if dc < 0.0 else dc) / (n - 1) for dc in d]  # (a NaN stays a NaN)
            den = (m[0] + m[1] + m[2]) / 3.0
            den = 0.01 if den < 0.01 else den
            e2 = ((v[0] + v[1] + v[2]) / 3.0) / (den * den)
            if math.isnan(e2) or math.isinf(e2):
                bad += 1
                continue
            total += e2
            worst = max(worst, e2)
    return {"noise": math.sqrt(total / pixels), "max_pixel": worst, "pixels": pixels, "bad_pixels": bad, "spp": n}
