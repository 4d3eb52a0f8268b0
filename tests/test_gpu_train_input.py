"""catseg_train_augment / catseg_train_crop_select (csrc/train_input.hip) and the device training-input
path built on them against the host composition `cat_seg.data.train_input.reference_apply` (which
tests/test_train_input_cpu.py ties to PIL, torch and the training mapper): every comparison is
torch.equal, on every byte of the image and every label."""
import itertools
import os

import numpy as np
import pytest
import torch

from cat_seg import ops
from cat_seg.data import train_input as TI
from cat_seg.data import transforms as T

pytestmark = pytest.mark.gpu

GUARD = 64


def launch(layout, pix, meta, S, ignore, select=None):
    """The packed host buffers -> (images, targets, crops record) through the kernels.  The outputs sit
    inside larger 0xCD-filled allocations whose surroundings must stay untouched."""
    B = len(layout.descs)
    pix_d, meta_d = torch.from_numpy(pix).cuda(), torch.from_numpy(meta).cuda()
    pad = 4096
    img_all = torch.full((pad + B * 3 * S * S + pad,), 0xCD, dtype=torch.uint8, device="cuda")
    tgt_all = torch.full((pad + B * S * S + pad,), 0xCD, dtype=torch.uint8, device="cuda").repeat_interleave(8).view(torch.int64)
    images = img_all[pad:pad + B * 3 * S * S].view(B, 3, S, S)
    targets = tgt_all[pad:pad + B * S * S].view(B, S, S)
    crops = None
    if select is not None:
        n_labels, max_area = select
        ws = torch.zeros(B * (layout.n_cand + 1), dtype=torch.int32, device="cuda")
        crops = torch.full((B + 2, 4), -7, dtype=torch.int32, device="cuda")[1:B + 1]
        for _ in range(2):                                # the second launch finds the counters zero again
            ops.train_crop_select(pix_d, meta_d, layout.cand_off, B, layout.n_cand, n_labels, ignore, max_area, ws, crops)
        assert int(ws[B * layout.n_cand:].abs().sum()) == 0
    ops.train_augment(pix_d, meta_d, B, images, targets, ignore, crops)
    torch.cuda.synchronize()
    assert np.array_equal(pix_d.cpu().numpy(), pix)       # the source, guard bytes included, is only read
    for whole in (img_all, tgt_all.view(torch.uint8)):
        n = whole.numel()
        edge = pad * (8 if whole is not img_all else 1)
        assert bool((whole[:edge] == 0xCD).all()) and bool((whole[n - edge:] == 0xCD).all())
    return images.cpu(), targets.cpu(), None if crops is None else crops.cpu()


def run(params, images, labels, S, ignore=255, select=None, guard=GUARD):
    layout = TI.plan_batch(params, [l.dtype for l in labels], S, select=select is not None, guard=guard)
    pix = np.full(layout.pixel_bytes, 0xAB, dtype=np.uint8)
    meta = np.zeros(layout.meta_words, dtype=np.int32)
    TI.fill_batch(layout, images, labels, pix, meta)
    return launch(layout, pix, meta, S, ignore, select)


def check(params, images, labels, S, ignore=255, select=None):
    """Device batch == reference_apply per image; returns the device outputs."""
    got_img, got_tgt, crops = run(params, images, labels, S, ignore, select)
    assert got_img.dtype == torch.uint8 and got_tgt.dtype == torch.int64
    for b, (p, im, lb) in enumerate(zip(params, images, labels)):
        ref_img, ref_tgt = TI.reference_apply(p, im, lb, ignore_label=ignore, size_divisibility=S,
                                              max_area=select[1] if select else 1.0)
        assert tuple(ref_img.shape) == (3, S, S)
        bad = (got_img[b] != ref_img).nonzero()
        assert torch.equal(got_img[b], ref_img), (b, p, bad[:5].tolist(), len(bad))
        assert torch.equal(got_tgt[b], ref_tgt), (b, p, (got_tgt[b] != ref_tgt).nonzero()[:5].tolist())
    return got_img, got_tgt, crops


def make(h, w, seed=0, n_classes=5, label_dtype=np.uint8, ignore=255):
    rng = np.random.default_rng(seed + 1000 * h + w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[: h // 4, : w // 4] = 255                         # saturated blocks: the clip of both passes
    img[h // 4: h // 2, : w // 4] = 0
    lab = rng.integers(0, n_classes, (h // 4 + 1, w // 4 + 1)).repeat(4, 0).repeat(4, 1)[:h, :w].astype(label_dtype)
    lab[rng.random((h, w)) < 0.1] = ignore
    return img, lab


def whole(h, w, nh, nw, **kw):
    return TI.TrainParams(h, w, nh, nw, [(0, 0, nh, nw)], **kw)


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("src,dst", [((37, 53), (48, 69)), ((61, 45), (40, 30)), ((100, 64), (31, 20)),
                                     ((24, 24), (24, 24)), ((50, 70), (50, 35))])
def test_resize_only(src, dst):
    """3, 5 and 9 taps (the last over two LDS chunks of source rows), no pass, one pass; the canvas of
    96 leaves pad on both sides and the 69-wide case spans two tiles."""
    img, lab = make(*src)
    check([whole(*src, *dst)], [img], [lab], 96)


# ------------------------------------------------------------------------------------------------ crop / flip / pad
CROPS = {"origin": ((37, 53), (48, 69), (0, 0, 30, 37)),
         "far_corner": ((37, 53), (48, 69), (48 - 30, 69 - 37, 30, 37)),
         "whole_image": ((29, 31), (36, 38), (0, 0, 36, 38)),
         "small": ((37, 53), (48, 69), (5, 7, 20, 21))}


@pytest.mark.parametrize("S", [40, 38])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case", list(CROPS))
def test_crop_flip_pad(case, flip, S):
    """S = 40: the 4-pixel stores; S = 38: the scalar store path.  Odd crop widths (37, 21) under the flip."""
    src, dst, crop = CROPS[case]
    img, lab = make(*src, seed=3)
    check([TI.TrainParams(*src, *dst, [crop], flip=flip)], [img], [lab], S)


def test_flip_across_tiles():
    """A flipped 69-wide crop spans two 64-wide tiles: each tile's LDS columns come from the mirrored side."""
    img, lab = make(37, 53, seed=4)
    check([TI.TrainParams(37, 53, 48, 69, [(0, 0, 48, 69)], flip=True)], [img], [lab], 96)
    check([TI.TrainParams(37, 53, 48, 69, [(3, 2, 40, 66)], flip=True)], [img], [lab], 72)


# ------------------------------------------------------------------------------------------------ colour
def colour_image():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    img[0:4] = np.arange(256, dtype=np.uint8).reshape(4, 64)[:, :, None]            # every grey level (d == 0)
    img[4] = 0                                                                       # pure black (v == 0)
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]], np.uint8)
    img[5, :60] = np.tile(prim, (10, 1))                                             # primaries, secondaries: ties
    hsv = np.stack([np.arange(180).repeat(2)[:320] % 180, np.full(320, 255), np.full(320, 200)], -1).astype(np.uint8)
    img[6:11] = T._hsv_to_rgb_u8(hsv).reshape(5, 64, 3)                               # a hue ramp
    img[11, :32] = [250, 250, 3]                                                     # clipping under +beta / alpha 1.5
    img[11, 32:] = [3, 250, 250]
    return img


C = T.ColorParams
COLOURS = {"bright+": C(brightness=True, beta=32.0), "bright-": C(brightness=True, beta=-32.0),
           "contrast_lo": C(contrast=True, contrast_alpha=0.5), "contrast_hi": C(contrast=True, contrast_alpha=1.5),
           "sat_lo": C(saturation=True, saturation_alpha=0.5), "sat_hi": C(saturation=True, saturation_alpha=1.5),
           "hue+": C(hue=True, hue_delta=18), "hue-": C(hue=True, hue_delta=-18),
           "all_order1": C(True, 13.37, 1, True, 1.2345678, True, 0.87654321, True, -11),
           "all_order0": C(True, -21.123456, 0, True, 0.7654321, True, 1.3333333, True, 7)}


@pytest.mark.parametrize("name", list(COLOURS))
def test_colour(name):
    img = colour_image()
    lab = np.zeros((64, 64), np.uint8)
    check([whole(64, 64, 64, 64, color=COLOURS[name])], [img], [lab], 64)


# ------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("dtype,n_classes,ignore", [(np.uint8, 150, 255), (np.int32, 848, 65535)])
def test_labels(dtype, n_classes, ignore):
    img, lab = make(45, 61, seed=5, n_classes=n_classes, label_dtype=dtype, ignore=ignore)
    if dtype == np.int32:
        lab[7, 9] = 847
    _, tgt, _ = check([TI.TrainParams(45, 61, 58, 79, [(2, 5, 50, 70)], flip=True)], [img], [lab], 80, ignore=ignore)
    assert int(tgt[0, 60, 75]) == ignore and int(tgt.max()) == ignore       # the pad is the ignore label


# ------------------------------------------------------------------------------------------------ batch
def _three():
    shapes = [((37, 53), (48, 69)), ((100, 64), (31, 20)), ((64, 64), (64, 64))]
    data = [make(*s, seed=6 + i, label_dtype=(np.int32 if i == 1 else np.uint8)) for i, (s, _) in enumerate(shapes)]
    params = [TI.TrainParams(37, 53, 48, 69, [(1, 2, 40, 60)], flip=True, color=COLOURS["all_order1"]),
              TI.TrainParams(100, 64, 31, 20, [(0, 0, 31, 20)], flip=False, color=COLOURS["sat_hi"]),
              TI.TrainParams(64, 64, 64, 64, [(0, 0, 64, 64)], flip=True, color=None)]
    return params, [d[0] for d in data], [d[1] for d in data]


def test_batch_equals_single_launches():
    params, images, labels = _three()
    img3, tgt3, _ = check(params, images, labels, 64)
    for b in range(3):
        img1, tgt1, _ = run(params[b:b + 1], images[b:b + 1], labels[b:b + 1], 64)
        assert torch.equal(img1[0], img3[b]) and torch.equal(tgt1[0], tgt3[b])


def test_poisoned_source_and_outputs():
    """64 guard bytes of 0xAB before, between and after the source planes, outputs pre-filled with 0xCD
    inside larger allocations (`launch` checks the guards and the surroundings): every output element is
    written and equals the yardstick."""
    params, images, labels = _three()
    layout = TI.plan_batch(params, [l.dtype for l in labels], 64, select=False, guard=GUARD)
    d = layout.descs
    assert int(d["img_off"][0]) >= GUARD
    for b in range(3):
        assert int(d["lab_off"][b]) - (int(d["img_off"][b]) + int(d["h"][b]) * int(d["w"][b]) * 3) >= GUARD
    assert layout.pixel_bytes - (int(d["lab_off"][2]) + 64 * 64) >= GUARD
    check(params, images, labels, 64)
    check(params, images, labels, 66)                     # the scalar store path


# ------------------------------------------------------------------------------------------------ crop selection
def _select_map(dtype, ignore, classes):
    """40 x 40: window A one class (fails), B one class exactly at 0.75 of the counted pixels (fails: the
    comparison is strict), C only the ignore label (fails), D two classes half / half (passes)."""
    c1, c2, c3, c4, c5 = classes
    sem = np.full((40, 40), ignore, dtype=dtype)
    sem[:20, :20] = c1
    sem[:20, 20:] = c2
    sem[0:5, 20:40] = c3
    sem[20:, 20:30] = c4
    sem[20:, 30:] = c5
    return sem


WIN = {"A": (0, 0, 20, 20), "B": (0, 20, 20, 20), "C": (20, 0, 20, 20), "D": (20, 20, 20, 20)}
SELECT = {"fifth_passes": ("ABCADAAAAA", 4), "first_passes": ("DAAAAAAAAA", 0), "none_passes": ("ABCABCABCB", 9),
          "only_ignore_then_pass": ("CCCCCCCDAA", 7), "threshold_is_strict": ("BBDAAAAAAA", 2)}


@pytest.mark.parametrize("n_labels", [256, 4096])
@pytest.mark.parametrize("case", list(SELECT))
def test_crop_select(case, n_labels):
    letters, expect = SELECT[case]
    if n_labels == 256:
        sem, ignore = _select_map(np.uint8, 255, (1, 2, 3, 4, 200)), 255
    else:
        sem, ignore = _select_map(np.int32, 65535, (1, 847, 3, 4095, 5)), 65535
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    cands = [WIN[c] for c in letters]
    assert TI.select_candidate(sem, cands, 0.75, ignore) == expect
    p = TI.TrainParams(40, 40, 40, 40, cands, flip=True, color=COLOURS["hue+"])
    _, _, crops = check([p], [img], [sem], 40, ignore=ignore, select=(n_labels, 0.75))
    assert crops[0].tolist() == list(cands[expect])


def test_crop_select_resized_batch():
    """Candidates in a nearest-resized label map (read through the index tables), three images per launch,
    random windows: the records equal the host rule, the augment launch that reads them equals the yardstick."""
    rng = np.random.default_rng(12)
    params, images, labels, expect = [], [], [], []
    for i, ((h, w), (nh, nw)) in enumerate([((40, 52), (60, 78)), ((90, 70), (45, 35)), ((33, 33), (33, 33))]):
        img, lab = make(h, w, seed=20 + i, n_classes=3)
        lab[rng.random((h, w)) < 0.3] = 255
        cands = []
        for _ in range(TI.N_CANDIDATES):
            ch, cw = int(rng.integers(4, min(nh, 32) + 1)), int(rng.integers(4, min(nw, 32) + 1))
            cands.append((int(rng.integers(nh - ch + 1)), int(rng.integers(nw - cw + 1)), ch, cw))
        if i == 0:
            cands[0] = cands[1] = (0, 0, 3, 3)            # a 4 x 4 label block: one class, or only ignore
        sem = T.ResizeTransform(h, w, nh, nw).apply_segmentation(lab.astype("double")) if (h, w) != (nh, nw) else lab
        expect.append(cands[TI.select_candidate(sem, cands, 0.5, 255)])
        params.append(TI.TrainParams(h, w, nh, nw, cands, flip=bool(i % 2)))
        images.append(img)
        labels.append(lab)
    _, _, crops = check(params, images, labels, 32, select=(256, 0.5))
    assert crops.tolist() == [list(e) for e in expect]


def test_wrapper_rejects_too_many_labels():
    params, images, labels = _three()
    with pytest.raises(ValueError, match="4096"):
        run(params, images, labels, 64, select=(4097, 0.75))


# ------------------------------------------------------------------------------------------------ end to end
def _png_dataset(tmp, shapes, n_classes):
    from PIL import Image
    from cat_seg.data import load_sem_seg
    img_dir, gt_dir = os.path.join(tmp, "img"), os.path.join(tmp, "gt")
    os.makedirs(img_dir)
    os.makedirs(gt_dir)
    for i, (h, w) in enumerate(shapes):
        img, lab = make(h, w, seed=30 + i, n_classes=n_classes)
        Image.fromarray(img).save(os.path.join(img_dir, f"{i:03d}.png"))
        Image.fromarray(lab).save(os.path.join(gt_dir, f"{i:03d}.png"))
    return load_sem_seg(gt_dir, img_dir, gt_ext="png", image_ext="png")


def _device_cfg(**over):
    from test_boundary_cpu import tiny_cfg
    cfg = tiny_cfg(**{"MODEL.CATSEG_HIP.TRAIN_INPUT": "device", "SOLVER.IMS_PER_BATCH": "2"})
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", "(384,)", "INPUT.CROP.ENABLED", "True", "INPUT.CROP.TYPE", "absolute",
                         "INPUT.CROP.SIZE", "(384, 384)", "INPUT.COLOR_AUG_SSD", "True", "INPUT.SIZE_DIVISIBILITY", "384"])
    for k, v in over.items():
        cfg.merge_from_list([k, v])
    return cfg


def test_device_loader_end_to_end(tmp_path):
    """PNGs -> build_train_loader(TRAIN_INPUT "device") -> batches equal to reference_apply of the same drawn
    parameters; the same seed gives the same batches; the training branch takes a device batch."""
    pytest.importorskip("PIL")
    from cat_seg import build_model
    from cat_seg.data import build_train_loader
    from cat_seg.data.dataset_mappers import read_image
    from conftest import GOLDEN
    gd = dict(np.load(os.path.join(GOLDEN, "e2e_tiny_pad.npz")))
    T_ = len(gd["tokens"])
    dicts = _png_dataset(str(tmp_path), [(300, 500), (420, 390), (384, 384)], T_)
    cfg = _device_cfg()
    loader = build_train_loader(dicts, cfg=cfg, num_workers=0, seed=5)
    seen = []
    for batch in itertools.islice(iter(loader), 2):
        assert len(batch) == 2
        for d, p in zip(batch, loader.post.last_params):
            assert set(d) == {"image", "sem_seg", "file_name", "height", "width", "ori_size"}
            assert d["image"].is_cuda and d["image"].dtype == torch.uint8 and tuple(d["image"].shape) == (3, 384, 384)
            assert d["sem_seg"].is_cuda and d["sem_seg"].dtype == torch.int64 and tuple(d["sem_seg"].shape) == (384, 384)
            image = read_image(d["file_name"], "RGB")
            sem = read_image(next(x for x in dicts if x["file_name"] == d["file_name"])["sem_seg_file_name"], None)
            ref_img, ref_sem = TI.reference_apply(p, image, sem, ignore_label=255, size_divisibility=384)
            assert torch.equal(d["image"].cpu(), ref_img) and torch.equal(d["sem_seg"].cpu(), ref_sem)
            assert d["ori_size"] == p.candidates[0][2:]
        seen.append([(d["file_name"], d["image"].cpu(), d["sem_seg"].cpu()) for d in batch])
    again = build_train_loader(dicts, cfg=cfg, num_workers=0, seed=5)
    for first, batch in zip(seen, itertools.islice(iter(again), 2)):
        for (name, im, sem), d in zip(first, batch):
            assert name == d["file_name"] and torch.equal(im, d["image"].cpu()) and torch.equal(sem, d["sem_seg"].cpu())
    model = build_model(cfg).cuda()
    model.sem_seg_head.predictor.set_class_tokens(gd["tokens"])
    model.arch = model.arch.replace(pad_len=int(gd["pad_len"]))
    model._engine = None
    model.train()
    loss = model(batch)["loss_sem_seg"]
    assert loss.dim() == 0 and bool(torch.isfinite(loss))


def test_device_loader_with_the_area_constraint(tmp_path):
    """SINGLE_CATEGORY_MAX_AREA < 1: ten candidates per image, the selection on the device; the batch
    equals reference_apply, which applies the host rule to the same candidates."""
    pytest.importorskip("PIL")
    from cat_seg.data.device_input import DeviceTrainAugment
    from cat_seg.data import RawTrainMapper
    dicts = _png_dataset(str(tmp_path), [(120, 150), (96, 200)], 4)
    cfg = _device_cfg(**{"INPUT.MIN_SIZE_TRAIN": "(96,)", "INPUT.CROP.SIZE": "(64, 64)", "INPUT.SIZE_DIVISIBILITY": "64",
                         "INPUT.CROP.SINGLE_CATEGORY_MAX_AREA": "0.3"})
    aug = DeviceTrainAugment(cfg, "cuda", seed=2)
    raws = [RawTrainMapper(cfg)(d) for d in dicts]
    batch = aug(raws)
    assert all(len(p.candidates) == TI.N_CANDIDATES for p in aug.last_params)
    for d, r, p in zip(batch, raws, aug.last_params):
        ref_img, ref_sem = TI.reference_apply(p, r["image_raw"].numpy(), r["sem_seg_raw"].numpy(), ignore_label=255,
                                              size_divisibility=64, max_area=0.3)
        assert torch.equal(d["image"].cpu(), ref_img) and torch.equal(d["sem_seg"].cpu(), ref_sem)


def test_no_host_sync(tmp_path):
    """One warm call of DeviceTrainAugment under torch's sync debug mode: staging, both copies and the
    launches never wait for the device."""
    pytest.importorskip("PIL")
    from cat_seg.data.device_input import DeviceTrainAugment
    from cat_seg.data import RawTrainMapper
    dicts = _png_dataset(str(tmp_path), [(120, 150), (96, 200)], 4)
    cfg = _device_cfg(**{"INPUT.MIN_SIZE_TRAIN": "(96,)", "INPUT.CROP.SIZE": "(64, 64)", "INPUT.SIZE_DIVISIBILITY": "64",
                         "INPUT.CROP.SINGLE_CATEGORY_MAX_AREA": "0.3"})
    aug = DeviceTrainAugment(cfg, "cuda", seed=2)
    raws = [RawTrainMapper(cfg)(d) for d in dicts]
    for _ in range(3):                                    # both slots allocated and used once
        aug(raws)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                # this build of torch has no such mode on ROCm
        pytest.skip(f"torch.cuda.set_sync_debug_mode unsupported: {e}")
    try:
        batch = aug(raws)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(batch[0]["image"].shape) == (3, 64, 64)
