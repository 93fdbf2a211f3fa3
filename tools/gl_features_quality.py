"""What the a-trous filter at its default sigmas does to a GL-shaded frame (pt_set_shading_features), on the CPU.

The five shipped scenes at 80 x 48, 4 GL passes, k = 1 (16 feature paths per pixel), depth 8: the relative MSE of the unfiltered and
of the filtered mean against a 512-pass frame of the GL model's CPU restatement (tests/glshade_reference.c), through the host builds
of csrc/pt_gl_features.h and csrc/pt_atrous.h (tests/gl_features_support.quality).  No GPU is needed; one JSON line per scene.

    python tools/gl_features_quality.py [--scenes a,b] [--out profiles/gl_features_quality.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    import gl_features_support as gf

    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(gf.SHIPPED))
    ap.add_argument("--width", type=int, default=80)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--ref-passes", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in [s for s in a.scenes.split(",") if s]:
        rows.append(gf.quality(name, a.width, a.height, a.passes, a.ref_passes))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
