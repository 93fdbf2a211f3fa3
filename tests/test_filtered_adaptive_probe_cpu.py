"""tests/filtered_adaptive_probe.hip without a GPU: it compiles for gfx950 with the library's flags and exports its entry points, it
includes the product headers unchanged and launches through the product's sequences, and the reference of its list test agrees
with the order of a device's first active list."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np

import adaptive_support as ad
import filtered_adaptive_probe_support as fp
import filtered_adaptive_support as fa


def code_of(path):
    text = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_probe_compiles_and_exports_its_entry_points():
    lib = fp.compile_probe()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert set(fp.SYMBOLS) <= set(re.findall(r"\bT (\w+)", syms))


def test_the_probe_launches_the_products_own_sequences():
    code = code_of(fp.SOURCE)
    core = code_of(os.path.join(fp.CSRC, "ptcore.hip"))
    launch = code_of(os.path.join(fp.CSRC, "pt_filter_launch.h"))
    assert '#include "pt_filter_launch.h"' in code and '#include "pt_kernels.h"' in code
    for where, text in (("probe", code), ("ptcore.hip", core)):  # neither has a launch of its own
        for kernel in ("block_err_kernel", "block_pool_kernel", "keep_from_map_kernel"):
            assert "ptk::" + kernel not in text, (where, kernel)
        assert "ptl::block_map_sequence(" in text and "ptl::keep_sequence(" in text, where
    for kernel in ("block_err_kernel", "block_pool_kernel", "keep_from_map_kernel"):
        assert launch.count("ptk::" + kernel) == 1, kernel
    assert "asm" not in code


def test_the_list_reference_follows_the_block_order():
    for w, h, si, sc in fp.LISTS:
        order = ad.block_order(w, h, si, sc)
        ns = fp.shard_slots(w, h, si, sc)
        nby, nbx = fa.grid(w, h)
        assert np.all(np.diff(order[:, 0]) > 0) and order[:, 0].max() < ns // 64
        assert order[:, 1].max() < nby and order[:, 2].max() < nbx
        stop = np.zeros((nby, nbx), np.uint8)
        stop[order[0, 1], order[0, 2]] = 1
        pooled = np.arange(nby * nbx, dtype=np.float64).reshape(nby, nbx) + 1.0
        r = fp.keep_reference(order, ns, 8, pooled, stop)
        assert r["nact"] == len(order) - 1 and r["next"][0] == order[1, 0] and r["next"][-1] == fp.SENTINEL
        assert r["worst"] == pooled[order[1:, 1], order[1:, 2]].max() and (r["blk_spp"] == 8).sum() == len(order)
    assert len(ad.block_order(293, 253, 0, 1)) > 1024  # more than one strip of compact_kernel
