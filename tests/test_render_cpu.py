"""Host half of the label-map renderer: the numpy restatement (tests/render_ref.py), which the GPU tests hold the
kernel to, against PIL's grey conversion, scipy's maximum / minimum filters and hand answers; the colour map and the
palettes; the kernel's logic (csrc/render_logic.h) run sequentially on the host against the restatement
(tools/render_host.cpp, built with the address and undefined-behaviour sanitizers); the C ABI entry and its
host-side argument checks; PredictionVisualizer's file naming, the panel layout on stub tensors; the config keys."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import render_ref as R
from cat_seg import _lib as L
from cat_seg import build_model, ops
from cat_seg import visualize as V

from conftest import ROOT
from test_boundary_cpu import tiny_cfg


# ------------------------------------------------------------------ the restatement against PIL, scipy and hand answers
def test_grey_is_pil_convert_l():
    from PIL import Image
    rng = np.random.default_rng(0)
    ext = np.array([[r, g, b] for r in (0, 1, 127, 128, 254, 255) for g in (0, 1, 127, 128, 254, 255)
                    for b in (0, 1, 127, 128, 254, 255)], np.uint8)
    rgb = np.concatenate([ext, rng.integers(0, 256, (4000, 3)).astype(np.uint8)])[None]
    assert np.array_equal(R.gray(rgb), np.asarray(Image.fromarray(rgb).convert("L")).astype(np.int64))


@pytest.mark.parametrize("edge_px", [1, 2, 3, 8])
def test_edge_mask_is_max_filter_ne_min_filter(edge_px):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(edge_px)
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 7), (34, 25), (5, 40)):
        coarse = rng.integers(0, 4, (H // 4 + 1, W // 4 + 1))
        m = np.repeat(np.repeat(coarse, 4, 0), 4, 1)[:H, :W]
        m = np.where(rng.random((H, W)) < 0.03, rng.integers(0, 4, (H, W)), m)
        size = 2 * edge_px + 1
        want = ndi.maximum_filter(m, size=size, mode="nearest") != ndi.minimum_filter(m, size=size, mode="nearest")
        assert np.array_equal(R.edge_mask(m, edge_px), want), (H, W)


def test_edge_mask_hand_maps():
    for e in (1, 3, 8):
        assert not R.edge_mask(np.full((9, 13), 5), e).any()                # uniform: no edge, the border included
        m = np.zeros((21, 25), np.int64)
        m[10, 12] = 1
        want = np.zeros((21, 25), bool)
        want[10 - e:10 + e + 1, 12 - e:12 + e + 1] = True                   # the square of side 2 e + 1
        assert np.array_equal(R.edge_mask(m, e), want)
        m = np.zeros((21, 25), np.int64)
        m[0, 24] = 1                                                        # in a corner: the square clipped
        want = np.zeros((21, 25), bool)
        want[:e + 1, 24 - e:] = True
        assert np.array_equal(R.edge_mask(m, e), want)
    assert not R.edge_mask(np.zeros((1, 1), np.int64), 8).any()


def test_blend_and_s8_hand_answers():
    assert R.blend(200, 100, 0) == 200 and R.blend(200, 100, 256) == 100
    assert R.blend(200, 100, 128) == 150 and R.blend(255, 0, 128) == 128 and R.blend(0, 255, 128) == 128
    assert R.blend(7, 250, 64) == (7 * 192 + 250 * 64 + 128) >> 8 == 68
    s = np.array([0.0, 0.5, 1.0, 1.5, -1.0, np.nan, 0.999, 1 / 512, -0.0, np.inf], np.float32)
    assert R.s8(s).tolist() == [0, 128, 256, 256, 0, 0, 255, 0, 0, 256]
    # the score scales alpha: 128 * 128 >> 8 = 64
    pal = np.array([[250, 250, 250]], np.uint8)
    img = np.full((1, 1, 3), 7, np.uint8)
    out = R.render(np.zeros((1, 1), np.int32), pal, image=img, alpha_q8=128, score=np.array([[0.5]], np.float32))
    assert out.tolist() == [[[68, 68, 68]]]
    assert R.source_index(5, 5).tolist() == [0, 1, 2, 3, 4]
    assert R.source_index(4, 2).tolist() == [0, 0, 1, 1] and R.source_index(2, 4).tolist() == [1, 3]
    assert R.source_index(3, 1).tolist() == [0, 0, 0]


def test_cell_means_with_partial_cells():
    """factor 3 on a 4 x 5 map: cells of 3 x 3, 3 x 2, 1 x 3 and 1 x 2 pixels, by hand."""
    lab = np.arange(20, dtype=np.int32).reshape(4, 5)
    pal = np.stack([np.arange(20) * 10, np.arange(20), 255 - np.arange(20) * 3], 1).astype(np.uint8)
    out = R.render(lab, pal, factor=3)
    assert out.shape == (2, 2, 3)
    r = lambda idx: [(sum(v) + len(idx) // 2) // len(idx) for v in zip(*[pal[i].astype(int).tolist() for i in idx])]
    assert out[0, 0].tolist() == r([0, 1, 2, 5, 6, 7, 10, 11, 12]) == [60, 6, 237]
    assert out[0, 1].tolist() == r([3, 4, 8, 9, 13, 14]) == [85, 9, 230]            # 8.5 rounds up, 229.5 up
    assert out[1, 0].tolist() == r([15, 16, 17]) == [160, 16, 207]
    assert out[1, 1].tolist() == r([18, 19]) == [185, 19, 200]                      # 18.5 -> 19, 199.5 -> 200
    assert np.array_equal(R.render(lab, pal, factor=64)[0, 0], r(list(range(20))))  # one cell larger than the map
    assert np.array_equal(R.render(lab, pal), pal[lab])


def test_order_of_the_steps():
    """gt before the blend, the edge after it and opaque, labels outside the palette in other_rgb."""
    pal = np.array([[10, 20, 30], [200, 100, 50]], np.uint8)
    lab = np.array([[0, 0, 0, 1], [0, 0, 0, 5]], np.int32)
    gt = np.array([[0, 1, 255, 1], [0, 0, 0, 0]], np.int32)
    img = np.full((2, 4, 3), 100, np.uint8)
    kw = dict(error_rgb=(255, 0, 0), ignore_rgb=0x000000, other_rgb=(1, 2, 3), edge_rgb=(255, 255, 255))
    out = R.render(lab, pal, image=img, gt=gt, alpha_q8=256, **kw)
    assert out[0].tolist() == [[10, 20, 30], [255, 0, 0], [0, 0, 0], [200, 100, 50]]
    assert out[1, 3].tolist() == [255, 0, 0]                                        # label 5 != gt 0: an error
    assert R.render(lab, pal, **kw)[1, 3].tolist() == [1, 2, 3]
    out = R.render(lab, pal, image=img, alpha_q8=128, edge_px=1, **kw)
    assert out[0, 0].tolist() == [55, 60, 65] and out[0, 2].tolist() == [255, 255, 255] == out[1, 3].tolist()
    assert R.render(lab, pal, clamp_pred=1, **kw)[1, 3].tolist() == [200, 100, 50]  # 5 folds to 1


# ------------------------------------------------------------------ colour map and palettes
def test_label_colormap_and_palette_for():
    assert V.label_colormap(8).tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128],
                                            [128, 0, 128], [0, 128, 128], [128, 128, 128]]
    cm = V.label_colormap(256)
    assert cm.dtype == np.uint8 and cm[8].tolist() == [64, 0, 0] and cm[255].tolist() == [224, 224, 192]     # VOC's void colour
    assert len({tuple(c) for c in cm.tolist()}) == 256
    from cat_seg.data.catalog import MetadataCatalog
    meta = MetadataCatalog.get("voc_2012_test_sem_seg")
    voc = V.palette_for("voc_2012_test_sem_seg", device="cpu")
    assert voc.dtype == torch.uint8 and voc.shape == (len(meta.stuff_colors), 3)
    assert voc.tolist() == [list(c) for c in meta.stuff_colors]
    assert V.palette_for(meta, 3, device="cpu").tolist() == [list(c) for c in meta.stuff_colors[:3]]
    more = V.palette_for("voc_2012_test_sem_seg", len(meta.stuff_colors) + 2, device="cpu")       # beyond the colours
    assert more[-1].tolist() == cm[len(meta.stuff_colors) + 1].tolist()
    for name in ("ade20k_150_test_sem_seg", "no such dataset", "", None):
        assert V.palette_for(name, 12, device="cpu").tolist() == cm[:12].tolist(), name
    with pytest.raises(ValueError):
        V.palette_for(None, 8193, device="cpu")


# ------------------------------------------------------------------ the kernel's logic on the host
def _write_case(path, rng, H, W, f, e):
    P = int(rng.integers(1, 9))
    lab = rng.integers(-1, P + 2, (H // 3 + 1, W // 3 + 1)).astype(np.int32)
    lab = np.repeat(np.repeat(lab, 3, 0), 3, 1)[:H, :W].copy()
    lab[rng.random((H, W)) < 0.03] = 255
    clamp = int(rng.choice([-1, 3]))
    pal = rng.integers(0, 256, (P, 3)).astype(np.uint8)
    has_img, has_s, has_g, gray = (int(v) for v in rng.integers(0, 2, 4))
    ih, iw = (H, W) if rng.random() < 0.3 else (int(rng.integers(1, 60)), int(rng.integers(1, 60)))
    img = rng.integers(0, 256, (ih, iw, 3)).astype(np.uint8)
    sc = rng.choice(np.array([0, .5, 1, 1.5, -1, np.nan, .123, .999, np.inf, -0.0], np.float32), (H, W))
    gt = np.where(rng.random((H, W)) < .2, 255, np.where(rng.random((H, W)) < .2, 0, lab)).astype(np.int32)
    alpha = int(rng.integers(0, 257))
    hdr = np.array([H, W, clamp, P, 0x102030, has_img, ih, iw, gray, has_s, has_g, 255, 0xff0001, 0x050607, alpha, e,
                    0xfffefd, f], np.int32)
    with open(path, "wb") as fh:
        for a, on in ((hdr, 1), (lab, 1), (pal, 1), (img, has_img), (sc.astype(np.float32), has_s), (gt, has_g)):
            if on:
                fh.write(np.ascontiguousarray(a).tobytes())
    return R.render(lab, pal, factor=f, image=img if has_img else None, gray_image=bool(gray), alpha_q8=alpha,
                    score=sc if has_s else None, gt=gt if has_g else None, ignore_label=255, error_rgb=0xff0001,
                    ignore_rgb=0x050607, edge_px=e, edge_rgb=0xfffefd, other_rgb=0x102030, clamp_pred=clamp)


def test_kernel_logic_on_the_host_against_the_restatement(tmp_path):
    """tools/render_host.cpp: the functions the kernel calls, pass by pass and sequentially, under the address and
    undefined-behaviour sanitizers, on random cases against the restatement.  A stand-alone program: nothing is
    loaded into this process."""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "render_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cat-seg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "render_host.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(11)
    shapes = [(1, 1), (1, 70), (70, 1), (17, 23), (16, 64), (17, 65), (40, 50)]
    for k in range(42):
        H, W = shapes[k % len(shapes)]
        f, e = (1, 2, 3, 7, 64)[k % 5], (0, 1, 3, 8)[(k // 2) % 4]
        want = _write_case(str(tmp_path / "case.bin"), rng, H, W, f, e)
        r = subprocess.run([exe, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok"), (k, r.stdout[-2000:], r.stderr[-2000:])
        got = np.fromfile(str(tmp_path / "out.bin"), np.uint8).reshape(want.shape)
        assert np.array_equal(got, want), (k, H, W, f, e)


# ------------------------------------------------------------------ the C ABI
NEW = ("catseg_render_labels",)


def test_header_and_lib_carry_exactly_the_new_symbol():
    text = open(os.path.join(ROOT, "include", "catseg_hip_render.h")).read()
    declared = set(re.findall(r"\b(catseg_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))
    assert declared == set(NEW) == set(L.EXPORTED_RENDER)
    assert L.RENDER_HEADERS == ("catseg_hip_render.h",)
    assert "struct" not in re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert '#include "catseg_hip_render.h"' in open(os.path.join(ROOT, "include", "catseg_hip.h")).read()
    lib = L.load()
    assert hasattr(lib, NEW[0]) and len(lib.catseg_render_labels.argtypes) == 29
    assert lib.catseg_abi_version() == 1


def test_the_old_groups_are_unchanged():
    assert L.PRODUCT_HEADERS == ("catseg_hip.h", "catseg_hip_train.h")
    assert L.INCLUDED_HEADERS == ("catseg_hip_simplify.h",) and L.EXTENSION_HEADERS == ("catseg_hip_boundary.h",)
    assert len(L._PROTOS) == 116 and len(L._STRUCTS) == 18
    assert len(L.EXPORTED_INCLUDED) == 4 and len(L.EXPORTED_EXTENSIONS) == 3
    old = set(L.EXPORTED) | set(L.EXPORTED_INCLUDED) | set(L.EXPORTED_EXTENSIONS) | set(L._PROTOS)
    assert not set(NEW) & old


def test_argument_checks_without_gpu():
    """Every refused argument returns -1 with its text before anything is launched: no device is needed, and the
    addresses are never dereferenced."""
    lib = L.load()
    p = 1 << 20
    #       labels H  W  ld clamp pal P  other image ih iw sr sc sch gray score lds gt ldg ign err ignc a8 e edge f out ldo stream
    good = (p, 8, 8, 8, -1, p, 5, 0, p, 8, 8, 24, 3, 1, 1, p, 8, p, 8, 255, 0xff0000, 0, 128, 1, 0xffffff, 2, p, 12, None)
    assert len(good) == 29
    bad = lambda i, v: lib.catseg_render_labels(*(good[:i] + (v,) + good[i + 1:]))
    err = lambda: lib.catseg_last_error()
    for i in (0, 5, 26):
        assert bad(i, None) == -1 and b"null" in err(), i                          # required pointers
    for i in (1, 2):
        assert bad(i, 0) == -1 and bad(i, 16385) == -1 and b"H and W" in err(), i
    for i in (9, 10):
        assert bad(i, 0) == -1 and bad(i, 16385) == -1 and b"ih and iw" in err(), i
    for i in (3, 16, 18):
        assert bad(i, 7) == -1 and b"stride is smaller than W" in err(), i         # ld, ld_score, ld_gt
    assert bad(27, 11) == -1 and b"3 Wo" in err()                                   # ld_out < 3 * 4
    assert bad(6, 0) == -1 and bad(6, 8193) == -1 and b"P " in err()
    assert bad(22, -1) == -1 and bad(22, 257) == -1 and b"alpha_q8" in err()
    assert bad(23, -1) == -1 and bad(23, 9) == -1 and b"edge_px" in err()
    assert bad(25, 0) == -1 and bad(25, 65) == -1 and b"factor" in err()
    assert bad(7, 1 << 24) == -1 and bad(24, -1) == -1 and bad(20, 1 << 24) == -1 and b"colour" in err()
    assert bad(11, -1) == -1 and b"image stride" in err()
    for i in (0, 15, 17):
        assert bad(i, p + 2) == -1 and b"misaligned" in err(), i
    # what an absent optional input leaves unchecked: its strides, sizes and colours
    no_image = good[:8] + (None, 0, 0, -1, -1, -1) + good[14:]
    no_score = no_image[:15] + (None, 0) + no_image[17:]
    no_gt = no_score[:17] + (None, 0, 255, -1, -1) + no_score[22:]
    for args in (no_image, no_score, no_gt):                                        # they reach the last check
        assert lib.catseg_render_labels(*((p + 2,) + args[1:])) == -1 and b"misaligned" in err()


# ------------------------------------------------------------------ visualizer and config
def test_visualizer_file_names_and_panel_layout(tmp_path, monkeypatch):
    viz = V.PredictionVisualizer(None, str(tmp_path), class_names=["a", "b"])
    assert viz.path_for({"file_name": "/data/Potsdam/img/top_2_13_RGB.tif"}) == str(tmp_path / "viz" / "top_2_13_RGB.png")
    assert viz.path_for({"file_name": "x.y.jpg"}) == str(tmp_path / "viz" / "x.y.png")
    assert viz.path_for({}, 7) == str(tmp_path / "viz" / "000007.png")
    assert viz.evaluate() == {} and hasattr(viz, "reset") and hasattr(viz, "process")
    assert V.panel_names(True, True) == ["image", "overlay", "labels", "gt", "error"]
    assert V.panel_names(False, False) == ["overlay", "labels"] and V.panel_names(True, False)[0] == "image"
    calls = []

    def stub(labels, palette, *, out, factor=1, **kw):                      # each launch paints its own columns
        calls.append(kw)
        out[...] = len(calls)
        return out
    monkeypatch.setattr(ops, "render_labels", stub)
    lab, pal = torch.zeros(5, 7, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.uint8)
    img, gt = torch.zeros(3, 5, 7, dtype=torch.uint8), np.zeros((5, 7), np.int64)
    wide = V.panels({"sem_seg_labels": lab, "sem_seg_score": torch.ones(5, 7)}, pal, image=img, gt=gt, factor=2,
                    edge_px=1, score_alpha=True)
    assert wide.shape == (3, 5 * 4, 3) and wide.dtype == torch.uint8
    assert wide[0, :, 0].tolist() == [k for k in (1, 2, 3, 4, 5) for _ in range(4)]
    assert calls[0]["alpha"] == 0.0 and calls[0]["gray"] is False and calls[0]["image"] is not None
    assert calls[1]["edge_px"] == 1 and calls[1]["score"] is not None and "gt" not in calls[1]
    assert "image" not in calls[2] and "edge_px" not in calls[2]
    assert calls[4]["gt"].dtype == torch.int32 and calls[4]["edge_px"] == 1
    assert V.panels(lab, pal).shape == (5, 14, 3)
    strip = V.legend_strip(["road", "building", "tree"], V.label_colormap(3), [1, 2], 60)
    assert strip.dtype == np.uint8 and strip.shape[1] == 60 and strip.shape[2] == 3 and strip.shape[0] >= 16
    assert (strip.reshape(-1, 3) == (128, 0, 0)).all(1).any() and not (strip.reshape(-1, 3) == (0, 0, 1)).all(1).any()
    assert V.classes_present(torch.tensor([[0, 2, 2], [255, -1, 2]], dtype=torch.int32), 3) == [0, 2]
    V.save_png(str(tmp_path / "a" / "b.png"), np.zeros((2, 60, 3), np.uint8), strip)
    from PIL import Image
    with Image.open(str(tmp_path / "a" / "b.png")) as im:
        assert im.size == (60, 2 + strip.shape[0])


def test_config_defaults_and_render_needs_labels():
    r = tiny_cfg().MODEL.CATSEG_HIP.RENDER
    assert (r.ENABLED, r.ALPHA, r.GRAY, r.EDGE_PX, r.FACTOR, r.SCORE_ALPHA, r.PALETTE) == (False, 0.5, True, 1, 1, False, "")
    with pytest.raises(ValueError, match="RENDER"):
        build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.RENDER.ENABLED": "True"}))
    for key, v in (("EDGE_PX", "9"), ("FACTOR", "0"), ("ALPHA", "1.5")):
        with pytest.raises(ValueError, match="RENDER"):
            build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.OUTPUT": "labels", "MODEL.CATSEG_HIP.RENDER.ENABLED": "True",
                                    f"MODEL.CATSEG_HIP.RENDER.{key}": v}))
    m = build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.OUTPUT": "labels", "MODEL.CATSEG_HIP.RENDER.ENABLED": "True",
                                "MODEL.CATSEG_HIP.RENDER.FACTOR": "8"}))
    assert m.render and m.render_factor == 8 and m.render_edge_px == 1 and m.render_alpha == 0.5
    plain = build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.OUTPUT": "labels"}))
    assert not plain.render
    result = {"sem_seg_labels": torch.zeros(2, 2, dtype=torch.int32), "sem_seg_score": torch.zeros(2, 2)}
    assert plain.add_regions(result, None) is result                        # off: every dict is what it was
