"""ops.render_labels (catseg_render_labels) against the sequential restatement tests/render_ref.py, bit for bit:
shapes round the kernel's 64 x 16 tile, factors that make cells straddle tiles and leave partial cells, edge
widths with label changes on tile borders and in the map's corners, labels outside the palette, both image
layouts and other image sizes, the special scores, a ground truth, strided views of poisoned buffers; then
MODEL.CATSEG_HIP.RENDER on every branch that returns labels, and PredictionVisualizer's PNG."""
import numpy as np
import pytest
import torch

import poison
import render_ref as R
from cat_seg import ops
from cat_seg import visualize as V

from test_boundary_cpu import tiny_cfg
from test_gpu_label_regions import _model, strided_input

pytestmark = pytest.mark.gpu

P = 7
SHAPES = [(1, 1), (1, 70), (70, 1), (17, 23), (16, 64), (17, 65), (150, 203)]
FACTORS = (1, 2, 3, 7, 64)
EDGES = (0, 1, 3, 8)
SCORES = np.array([0.0, 0.5, 1.0, 1.5, -1.0, np.nan, 0.123, 0.999, -0.0, np.inf, -np.inf, 1e-30], np.float32)
COLOURS = dict(other_rgb=(16, 32, 48), error_rgb=(255, 0, 1), ignore_rgb=(5, 6, 7), edge_rgb=(255, 254, 253))
_CASES = {}


def case(H, W):
    """One set of inputs per shape, made once: blobs of labels -1 .. P + 1 and 255 whose borders fall anywhere, with
    changes forced onto the tile borders (x = 63 | 64, y = 14 | 15 | 16) and into the four corners."""
    if (H, W) not in _CASES:
        rng = np.random.default_rng(1000 * H + W)
        coarse = rng.integers(-1, P + 2, (H // 5 + 1, W // 5 + 1))
        lab = np.repeat(np.repeat(coarse, 5, 0), 5, 1)[:H, :W].astype(np.int32)
        lab[rng.random((H, W)) < 0.02] = 255
        inside = (lab >= 0) & (lab < P)                 # the labels outside the palette stay what they are
        lab[:, 64:] = np.where(inside[:, 64:], (lab[:, 64:] + 1) % P, lab[:, 64:])
        lab[15:] = np.where(inside[15:], (lab[15:] + 2) % P, lab[15:])
        lab[14::16, 60:68] = 3
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            lab[y, x] = 5 if lab[y, x] != 5 else 4
        gt = np.where(rng.random((H, W)) < 0.15, 255, np.where(rng.random((H, W)) < 0.2, 1, lab)).astype(np.int32)
        _CASES[(H, W)] = dict(labels=lab, gt=gt, score=rng.choice(SCORES, (H, W)).astype(np.float32),
                              palette=rng.integers(0, 256, (P, 3)).astype(np.uint8),
                              image=rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
    return _CASES[(H, W)]


def run(c, *, image=None, layout="hwc", score=False, gt=False, alpha=0.5, **kw):
    """ops.render_labels and the restatement on the same inputs -> (got, want) as numpy arrays."""
    dev = lambda a: torch.as_tensor(a).cuda()
    img_t = None
    if image is not None:
        img_t = dev(image) if layout == "hwc" else dev(np.ascontiguousarray(image.transpose(2, 0, 1)))
    got = ops.render_labels(dev(c["labels"]), dev(c["palette"]), image=img_t, alpha=alpha,
                            score=dev(c["score"]) if score else None, gt=dev(c["gt"]) if gt else None, **kw)
    ref_kw = {k: v for k, v in kw.items() if k != "gray"}
    want = R.render(c["labels"], c["palette"], image=image, gray_image=kw.get("gray", True),
                    alpha_q8=int(round(256 * alpha)), score=c["score"] if score else None,
                    gt=c["gt"] if gt else None, **ref_kw)
    return got.cpu().numpy(), want


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_factors_and_edges(H, W):
    c = case(H, W)
    for f in FACTORS:
        for e in EDGES:
            got, want = run(c, image=c["image"], score=True, gt=True, factor=f, edge_px=e, **COLOURS)
            assert got.shape == (-(-H // f), -(-W // f), 3) and got.dtype == np.uint8
            assert np.array_equal(got, want), (f, e)


@pytest.mark.parametrize("clamp", [-1, 4])
def test_labels_outside_the_palette_and_the_fold(clamp):
    c = dict(case(17, 65))
    c["labels"] = c["labels"].copy()
    c["labels"][2, :9] = [-1, -7, P, P + 1, 255, 2 ** 31 - 1, -2 ** 31, 0, P - 1]
    for f, e in ((1, 1), (3, 3)):
        got, want = run(c, factor=f, edge_px=e, clamp_pred=clamp, **COLOURS)
        assert np.array_equal(got, want), (f, e)


@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_image_layouts_sizes_and_options(layout):
    c = case(150, 203)
    rng = np.random.default_rng(5)
    for ih, iw in ((150, 203), (37, 53), (301, 407)):
        img = rng.integers(0, 256, (ih, iw, 3)).astype(np.uint8)
        for gray in (True, False):
            got, want = run(c, image=img, layout=layout, gray=gray, factor=1 + (ih == 37), edge_px=1)
            assert np.array_equal(got, want), (ih, iw, gray)
    got, want = run(c, edge_px=1)                                           # no image at all
    assert np.array_equal(got, want)
    sliced = torch.as_tensor(img).cuda()[::2, 1::3]                         # any strides pass without a copy
    got = ops.render_labels(torch.as_tensor(c["labels"]).cuda(), torch.as_tensor(c["palette"]).cuda(), image=sliced)
    assert np.array_equal(got.cpu().numpy(), R.render(c["labels"], c["palette"], image=img[::2, 1::3]))


def test_scores_alphas_and_ground_truth():
    c = dict(case(17, 23))
    c["score"] = np.resize(SCORES, (17, 23)).astype(np.float32)
    for alpha in (0.0, 0.5, 1.0, 0.3):
        for gt in (False, True):
            got, want = run(c, image=c["image"], score=True, gt=gt, alpha=alpha, gray=False, **COLOURS)
            assert np.array_equal(got, want), (alpha, gt)
    got, want = run(c, image=c["image"], gt=True, ignore_label=1, **COLOURS)
    assert np.array_equal(got, want)


def test_strided_views_of_poisoned_buffers_and_determinism():
    H, W, f = 37, 75, 2
    c = case(H, W)
    lbuf, lab = strided_input(c["labels"])
    gbuf, gt = strided_input(c["gt"])
    sbuf, score = poison.padded(torch.as_tensor(c["score"]), 2, 5, device="cuda")
    Ho, Wo = -(-H // f), -(-W // f)
    obuf = poison.filled((Ho + 2, 3 * Wo + 7), torch.uint8, "cuda")
    out = obuf[:Ho, 1:3 * Wo + 1].unflatten(1, (Wo, 3))                  # an odd byte offset and an odd row stride
    pal, img = torch.as_tensor(c["palette"]).cuda(), torch.as_tensor(c["image"]).cuda()
    kw = dict(image=img, score=score, gt=gt, edge_px=3, factor=f, **COLOURS)
    before = lbuf.clone(), gbuf.clone()
    got = ops.render_labels(lab, pal, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    want = R.render(c["labels"], c["palette"], image=c["image"], score=c["score"], gt=c["gt"], edge_px=3, factor=f,
                    **COLOURS)
    assert np.array_equal(out.cpu().numpy(), want)
    slack = poison.holds_fill(obuf).clone()
    slack[:Ho, 1:3 * Wo + 1] = True
    assert bool(slack.all()), "bytes outside the picture were written"
    assert torch.equal(lbuf, before[0]) and torch.equal(gbuf, before[1])
    dense = ops.render_labels(lab.contiguous(), pal, **{**kw, "score": score.contiguous(), "gt": gt.contiguous()})
    again = ops.render_labels(lab, pal, **kw)
    poison.check_bit_identical(dense, again, "dense vs strided")
    poison.check_bit_identical(dense, out.contiguous(), "fresh vs given out")


def test_wrapper_refusals():
    c = case(17, 23)
    lab, pal = torch.as_tensor(c["labels"]).cuda(), torch.as_tensor(c["palette"]).cuda()
    img, sc, gt = (torch.as_tensor(c[k]).cuda() for k in ("image", "score", "gt"))
    bad = [("labels", dict(labels=lab.cpu())), ("labels", dict(labels=lab.float())), ("labels", dict(labels=lab.t())),
           ("palette", dict(palette=pal.cpu())), ("palette", dict(palette=pal.int())), ("palette", dict(palette=pal[:, :2])),
           ("palette", dict(palette=pal[:0])), ("image", dict(image=img.cpu())), ("image", dict(image=img.float())),
           ("image", dict(image=img[..., :2])), ("score", dict(score=sc.double())), ("score", dict(score=sc[:, :5])),
           ("score", dict(score=sc.cpu())), ("gt", dict(gt=gt.long())), ("gt", dict(gt=gt.t().contiguous())),
           ("alpha", dict(alpha=1.5)), ("alpha", dict(alpha=-0.1)), ("edge_px", dict(edge_px=9)),
           ("edge_px", dict(edge_px=-1)), ("factor", dict(factor=0)), ("factor", dict(factor=65)),
           ("factor", dict(factor=2.0)), ("edge_rgb", dict(edge_rgb=(256, 0, 0))), ("other_rgb", dict(other_rgb=-1)),
           ("error_rgb", dict(error_rgb=(1, 2))), ("out", dict(out=torch.empty(17, 23, 3, device="cuda"))),
           ("out", dict(out=torch.empty(17, 22, 3, dtype=torch.uint8, device="cuda"))),
           ("out", dict(out=torch.empty(3, 17, 23, dtype=torch.uint8, device="cuda").permute(1, 2, 0)))]
    for name, kw in bad:
        args = {"labels": lab, "palette": pal, **kw}
        with pytest.raises(ValueError, match=name):
            ops.render_labels(args.pop("labels"), args.pop("palette"), **args)


# ------------------------------------------------------------------ MODEL.CATSEG_HIP.RENDER
RENDER = {"MODEL.CATSEG_HIP.RENDER.ENABLED": "True"}


def _check_render(model, plain, got, image, **options):
    """`got` is `plain` plus "sem_seg_render" = ops.render_labels of the returned map over the input image."""
    assert set(got) == set(plain) | {"sem_seg_render"} and "sem_seg_render" not in plain
    for k in plain:
        if torch.is_tensor(plain[k]):
            poison.check_bit_identical(plain[k], got[k], k)
    opts = dict(gray=True, alpha=0.5, edge_px=1, factor=1)
    opts.update(options)
    pal = V.palette_for(None, int(model.sem_seg_head.predictor.class_tokens("test").shape[0]), device="cuda")
    want = ops.render_labels(got["sem_seg_labels"], pal, image=image.cuda(), **opts)
    assert got["sem_seg_render"].dtype == torch.uint8 and got["sem_seg_render"].is_cuda
    poison.check_bit_identical(got["sem_seg_render"], want, "sem_seg_render")
    return pal, opts


def test_model_render_graph_and_eager():
    gen = torch.Generator().manual_seed(3)
    a, b = [(torch.rand(s, generator=gen) * 255).to(torch.uint8) for s in ((3, 384, 384), (3, 300, 352))]
    inputs = [{"image": a, "height": 200, "width": 300}, {"image": b}]
    plain = _model()(inputs)
    assert all(set(p) == {"sem_seg_labels", "sem_seg_score"} for p in plain)
    outs = {}
    for graph in ("True", "False"):
        m = _model(**{"MODEL.CATSEG_HIP.GRAPH": graph, **RENDER})
        outs[graph] = m(inputs)
        for p, g, x in zip(plain, outs[graph], inputs):
            pal, opts = _check_render(m, p, g, x["image"])
        g = outs[graph][0]                                                   # the 384 x 384 image drawn at 200 x 300
        assert g["sem_seg_render"].shape == (200, 300, 3)
        want = R.render(g["sem_seg_labels"].cpu().numpy(), pal.cpu().numpy(), image=a.permute(1, 2, 0).numpy(), edge_px=1)
        assert np.array_equal(g["sem_seg_render"].cpu().numpy(), want)
    for g, e in zip(outs["True"], outs["False"]):
        poison.check_bit_identical(g["sem_seg_render"], e["sem_seg_render"], "graph vs eager")


def test_model_render_options_float_image_and_sieve():
    """FACTOR, EDGE_PX, GRAY, ALPHA and SCORE_ALPHA reach the kernel; a float image is clamped and truncated; with
    REGIONS.MIN_AREA the picture is drawn from the sieved map."""
    gen = torch.Generator().manual_seed(3)
    b = torch.rand((3, 300, 352), generator=gen) * 300 - 20                 # a float image beyond 0 .. 255
    over = {**RENDER, "MODEL.CATSEG_HIP.RENDER.FACTOR": "8", "MODEL.CATSEG_HIP.RENDER.EDGE_PX": "0",
            "MODEL.CATSEG_HIP.RENDER.GRAY": "False", "MODEL.CATSEG_HIP.RENDER.ALPHA": "0.25",
            "MODEL.CATSEG_HIP.RENDER.SCORE_ALPHA": "True"}
    plain, m = _model()([{"image": b}])[0], _model(**over)
    got = m([{"image": b}])[0]
    _check_render(m, plain, got, b.clamp(0, 255).to(torch.uint8), factor=8, edge_px=0, gray=False, alpha=0.25,
                  score=got["sem_seg_score"])
    assert got["sem_seg_render"].shape == (38, 44, 3)
    regions = {"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True", "MODEL.CATSEG_HIP.REGIONS.MIN_AREA": "6"}
    img = b.clamp(0, 255).to(torch.uint8)
    sieved, m = _model(**regions)([{"image": img}])[0], _model(**regions, **RENDER)
    got = m([{"image": img}])[0]
    assert torch.equal(got["sem_seg_labels"], sieved["sem_seg_labels"])
    pal = V.palette_for(None, int(m.sem_seg_head.predictor.class_tokens("test").shape[0]), device="cuda")
    poison.check_bit_identical(got["sem_seg_render"],
                               ops.render_labels(sieved["sem_seg_labels"], pal, image=img.cuda(), edge_px=1), "sieved")


def test_model_render_tiled_and_sliding():
    tiled = {"MODEL.CATSEG_HIP.TILED.ENABLED": "True", "MODEL.CATSEG_HIP.TILED.TILE": "64",
             "MODEL.CATSEG_HIP.TILED.STRIDE": "32", "MODEL.CATSEG_HIP.TILED.BATCH": "4"}
    img = (torch.rand((3, 96, 96), generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8)
    m = _model(**tiled, **RENDER)
    _check_render(m, _model(**tiled)([{"image": img}])[0], m([{"image": img}])[0], img)
    slide = {"TEST.SLIDING_WINDOW": "True"}
    a = (torch.rand((3, 300, 352), generator=torch.Generator().manual_seed(4)) * 255).to(torch.uint8)
    m = _model(**slide, **RENDER)
    got = m([{"image": a}])[0]
    _check_render(m, _model(**slide)([{"image": a}])[0], got, a)
    assert got["sem_seg_render"].shape == (640, 640, 3)


def test_model_render_through_the_device_tta_merge():
    from cat_seg import SemanticSegmentorWithTTA
    from cat_seg.test_time_augmentation import DatasetMapperTTA
    img = (torch.rand((3, 60, 80), generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8)
    outs = []
    for over in ({}, RENDER):
        cfg = tiny_cfg(**{"MODEL.CATSEG_HIP.TTA_MERGE": "device", "MODEL.CATSEG_HIP.OUTPUT": "labels", **over})
        m = _model(**{"MODEL.CATSEG_HIP.TTA_MERGE": "device", **over})
        w = SemanticSegmentorWithTTA(cfg, m, tta_mapper=DatasetMapperTTA(min_sizes=(48, 64), max_size=4000, flip=True))
        outs.append(w([{"image": img}])[0])
    _check_render(m, outs[0], outs[1], img)
    assert outs[1]["sem_seg_render"].shape == (60, 80, 3)


def test_prediction_visualizer_writes_the_panels(tmp_path):
    from PIL import Image
    c = case(37, 75)
    out = {"sem_seg_labels": torch.as_tensor(np.clip(c["labels"], 0, P - 1)).cuda(),
           "sem_seg_score": torch.as_tensor(c["score"]).cuda()}
    inp = {"file_name": "/data/scenes/area_7.tif", "image": torch.as_tensor(c["image"]).permute(2, 0, 1),
           "sem_seg_gt": c["gt"]}
    names = [f"class{i}" for i in range(P)]
    viz = V.PredictionVisualizer(None, str(tmp_path), palette=c["palette"], class_names=names, edge_px=1, factor=2)
    viz.reset()
    viz.process([inp], [out])
    assert viz.evaluate() == {} and viz.written == [str(tmp_path / "viz" / "area_7.png")]
    want = V.panels(out, torch.as_tensor(c["palette"]).cuda(), image=inp["image"], gt=c["gt"], edge_px=1, factor=2)
    assert want.shape == (19, 5 * 38, 3)
    with Image.open(viz.written[0]) as im:
        assert np.array_equal(np.asarray(im), want.cpu().numpy())
    # the panels are the kernel's pictures side by side, the overlay second
    over = R.render(out["sem_seg_labels"].cpu().numpy(), c["palette"], image=c["image"], edge_px=1, factor=2)
    assert np.array_equal(want[:, 38:76].cpu().numpy(), over)
    # probabilities pass through an argmax on the device; the legend goes under the picture
    probs = torch.nn.functional.one_hot(out["sem_seg_labels"].long(), P).permute(2, 0, 1).float()
    viz = V.PredictionVisualizer(None, str(tmp_path / "p"), palette=c["palette"], class_names=names, gt=False,
                                 legend=True, edge_px=1, factor=2)
    viz.process([{"image": inp["image"]}], [{"sem_seg": probs}])
    with Image.open(str(tmp_path / "p" / "viz" / "000000.png")) as im:
        arr = np.asarray(im)
    assert arr.shape[1] == 3 * 38 and arr.shape[0] > 19
    assert np.array_equal(arr[:19, 38:76], over)
