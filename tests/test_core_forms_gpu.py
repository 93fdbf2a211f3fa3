"""trace_kernel, its nested exit search and glass_kernel take their LDS pointers from one layout (ptd::LdsLayout) and share their
staging loops, queue window, entry store / load and dielectric exit search (pt_kernels.h).  Small scenes whose record counts put the
record-order object copy behind every possible pad, a full single-group scene and a grouped one are rendered in every form of the
render loop and held to the oracle in both builds; a larger frame makes waves of trace_kernel open a second queue window."""
import pytest

from conftest import render_vs_oracle

pytestmark = pytest.mark.gpu

V = lambda x, y, z: {"x": x, "y": y, "z": z}  # noqa: E731
CAM = {"position": V(0, 1.2, 5), "target": V(0, 1, 0), "up": V(0, 1, 0), "fov": 45, "aperture": 0.05, "focus_dist": 5, "aspect_ratio": 0}
SKY = {"type": "gradient", "horizon": {"r": 1, "g": 1, "b": 1}, "zenith": {"r": 0.4, "g": 0.6, "b": 1.0}}
MATS = [{"id": "d", "type": "lambert", "albedo": {"r": 0.7, "g": 0.6, "b": 0.5}},
        {"id": "g", "type": "dielectric", "ior": 1.5, "albedo": {"r": 1, "g": 1, "b": 1}},
        {"id": "t", "type": "dielectric", "ior": 1.33, "albedo": {"r": 1, "g": 1, "b": 1}, "absorption": {"r": 0.3, "g": 0.05, "b": 0.0}},
        {"id": "m", "type": "metal", "albedo": {"r": 0.9, "g": 0.9, "b": 0.9}, "rough": 0.2},
        {"id": "e", "type": "emissive", "emit": {"r": 1, "g": 0.9, "b": 0.8}, "power": 6}]
W, H, SPP, DEPTH, SEED = 33, 17, 5, 8, 5


def _scene(spheres, boxes):
    """spheres / boxes: material ids, laid out left to right in two rows in front of the camera, over a ground plane."""
    objs = [{"type": "plane", "position": V(0, 0, 0), "material_id": "d"}]
    ns, nb = len(spheres), len(boxes)
    for i, m in enumerate(spheres):
        cols = min(ns, 11)
        x, z = (i % cols - (cols - 1) / 2) * 0.75, -1.5 * (i // cols)
        objs.append({"type": "sphere", "position": V(x, 0.35 + 0.5 * ((i // cols) % 2), z), "size": V(0.3, 0, 0), "material_id": m})
    for i, m in enumerate(boxes):
        cols = min(nb, 11)
        x, z = (i % cols - (cols - 1) / 2) * 0.75, 1.0 - 1.5 * (i // cols)
        objs.append({"type": "box", "position": V(x, 1.6 + 0.45 * ((i // cols) % 2), z), "size": V(0.5, 0.4, 0.5), "material_id": m})
    return {"camera": CAM, "sky": SKY, "objects": objs, "materials": MATS}


def _third_glass(n, first):
    return [("g", "t")[i % 2] if i % 3 == first else ("d", "m", "e")[i % 3] for i in range(n)]


# name -> (sphere materials, box materials).  The pad in front of the record-order copy is 16 - 4 * (index count mod 4): the index
# count is every record plus every dielectric record in trace_kernel, the dielectric records in glass_kernel.
SCENES = {
    "pad12_glass8": (["m", "g"], ["t"]),                       # 3 + 2 = 5 entries -> 12 bytes; glass_kernel 2 -> 8
    "pad8_glass12": (["e", "t", "d"], ["m", "d"]),              # 5 + 1 = 6 -> 8; 1 -> 12
    "pad4_glass4": (["g", "m", "t"], ["g"]),                    # 4 + 3 = 7 -> 4; 3 -> 4
    "full_32_32": (_third_glass(32, 0), _third_glass(32, 1)),  # every bit of both candidate masks
    "grouped_33": (_third_glass(33, 0), []),                   # one sphere more than a mask holds: the scan in groups of 32
}
FORMS = {
    "default": {},
    "rounds0": {"PTCORE_SPLIT_ROUNDS": "0"},
    "rounds3": {"PTCORE_SPLIT_ROUNDS": "3"},
    "tail_trip": {"PTCORE_TAIL": "trip"},
    "verify": {"PTCORE_SCAN": "verify"},
    "verify_wide": {"PTCORE_SCAN": "verify_wide"},
}


def test_the_scenes_have_the_pads_their_names_say():
    def pads(spheres, boxes):
        nd = sum(m in ("g", "t") for m in spheres + boxes)
        return (16 - 4 * ((len(spheres) + len(boxes) + nd) % 4)) % 16, (16 - 4 * (nd % 4)) % 16

    assert pads(*SCENES["pad12_glass8"]) == (12, 8)
    assert pads(*SCENES["pad8_glass12"]) == (8, 12)
    assert pads(*SCENES["pad4_glass4"]) == (4, 4)
    s, b = SCENES["full_32_32"]
    assert (len(s), len(b)) == (32, 32) and sum(m in ("g", "t") for m in s + b) == 22
    assert len(SCENES["grouped_33"][0]) == 33 and any(m in ("g", "t") for m in SCENES["grouped_33"][0])


@pytest.fixture(scope="module")
def references(oracle):
    """The oracle's frame of every scene, computed once and left unchanged."""
    docs = {name: _scene(*sb) for name, sb in SCENES.items()}
    return {name: (doc, oracle.render(oracle.Scene(doc), W, H, SPP, DEPTH, seed=SEED)) for name, doc in docs.items()}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(SCENES))
def test_every_form_gives_the_oracle_frame_in_both_builds(monkeypatch, references, gpu_ctx, name, form):
    from path_trace_golang_amd import capi, scene

    doc, o = references[name]
    assert o["stats"]["exit_scans"] > 0  # the glass is in view
    for k in ("PTCORE_SPLIT_ROUNDS", "PTCORE_TAIL", "PTCORE_SCAN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    L = capi.load()
    with capi.Context(ndev=1) as ctx:  # the knobs are read by pt_create
        before = L.pt_debug_scan_mismatches(ctx.handle)
        out = render_vs_oracle(ctx, scene.Scene.decode(doc), o, W, H, SPP, DEPTH, SEED, tag=(name, form))
        if form.startswith("verify"):
            assert out["stats"][4]["segments"] > 0 and L.pt_debug_scan_mismatches(ctx.handle) - before == 0


def test_waves_of_trace_kernel_open_a_second_glass_window(monkeypatch, oracle, gpu_ctx):
    """The glass box that fills the view (test_split_passes_gpu.py), large enough that with one block per CU the first trace pass
    parks more paths than PT_QUEUE_BLOCK = 256 slots for each of its 4 * CU waves: by pigeonhole some wave reserved a second window,
    so a push straddled two windows (the by-slot store) and the cursor moved to a new base."""
    import torch

    from path_trace_golang_amd import capi, scene

    objs = [{"type": "plane", "position": V(0, 0, 0), "material_id": "d"},
            {"type": "box", "position": V(0, 1.2, 1.5), "size": V(6, 3, 1.5), "material_id": "g"},
            {"type": "sphere", "position": V(-0.8, 1, -1), "size": V(0.8, 0, 0), "material_id": "t"},
            {"type": "sphere", "position": V(1, 0.7, -0.5), "size": V(0.7, 0, 0), "material_id": "m"},
            {"type": "sphere_light", "position": V(0, 4, 0), "size": V(0.6, 0, 0), "material_id": "e"}]
    doc = {"camera": CAM, "sky": SKY, "objects": objs, "materials": MATS}
    w, h, spp, depth, seed = 640, 360, 4, 6, 3
    o = oracle.render(oracle.Scene(doc), w, h, spp, depth, seed=seed)
    monkeypatch.setenv("PTCORE_SPLIT_ROUNDS", "1")
    monkeypatch.setenv("PTCORE_BLOCKS_PER_CU", "1")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    with capi.Context(ndev=1) as ctx:
        out = render_vs_oracle(ctx, scene.Scene.decode(doc), o, w, h, spp, depth, seed, tag="second window")
    for form in ("stats", "shipping"):
        assert out[form][4]["glass_events"] > 256 * 4 * cus, (form, out[form][4]["glass_events"], cus)
