"""The device probe (tests/device_probe.hip) without a GPU: it cross-compiles for gfx950 with the library's flags against the
unchanged product headers and exports what test_device_math_gpu.py calls, so a header change that breaks the probe shows
on any machine."""
from __future__ import annotations

import re
import subprocess

import device_probe_support as dp


def test_probe_compiles_for_gfx950_with_the_library_flags():
    from path_trace_golang_amd import build

    assert "-ffp-contract=off" in build.HIP_FLAGS and "--offload-arch=gfx950" in build.HIP_FLAGS
    lib = dp.compile_probe()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (\w+)", syms))
    assert set(dp.SYMBOLS) <= exported, sorted(set(dp.SYMBOLS) - exported)
    with open(lib, "rb") as f:
        blob = f.read()
    # the device code object is inside, for the target the library ships for, with the wrappers as kernels
    assert b"gfx950" in blob
    for kernel in (b"pass_kernel", b"inscatter_kernel", b"unary_kernel", b"sincos_kernel", b"streams_kernel"):
        assert kernel in blob, kernel


def test_probe_source_has_no_inline_assembly_and_does_not_touch_the_headers():
    with open(dp.SOURCE) as f:
        src = f.read()
    assert "asm" not in re.sub(r"//.*", "", src)
    assert '#include "pt_glshade.h"' in src
    # the product's names, not copies of its code
    for name in ("ptm::go_sin", "ptm::go_tan", "ptm::go_exp", "ptm::go_pow5", "ptm::go_min", "ptm::go_max", "ptm::sincos_pos",
                 "ptm::f_sqrt<true>", "ptm::f_sqrt<false>", "ptm::stream_init", "ptm::stream_next", "ptf::hash31",
                 "ptf::volume_noise", "ptf::phase_hg", "ptf::fog_inscatter", "ptg::gl_pass"):
        assert name in src, name
