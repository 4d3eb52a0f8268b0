"""Host side of the device training-input path (cat_seg/data/train_input.py, build.py): the tables the
kernels read restate PIL and torch exactly, the pinned colour draw equals the random one, the host
reference equals the training mapper, the candidate rule, the sampler and the host loader."""
import itertools
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from cat_seg.data import TrainingSampler, build_train_loader, load_sem_seg
from cat_seg.data import train_input as TI
from cat_seg.data import transforms as T
from cat_seg.data.dataset_mappers import MaskFormerSemanticDatasetMapper, read_image

from test_boundary_cpu import tiny_cfg

# (h, w) -> (new_h, new_w): up with 3 taps, down with 5, one axis unchanged, up by ~2.9, down by 3.2 (9 taps), unchanged
SIZE_PAIRS = [((37, 53), (48, 69)), ((61, 45), (40, 30)), ((50, 70), (50, 35)), ((33, 47), (96, 137)),
              ((100, 64), (31, 20)), ((24, 24), (24, 24))]


@pytest.mark.parametrize("src,dst", SIZE_PAIRS)
def test_resample_tables_equal_pil_bilinear(src, dst):
    rng = np.random.default_rng(src[0] * 1000 + dst[1])
    img = rng.integers(0, 256, src + (3,), dtype=np.uint8)
    img[:4, :4] = 255
    img[4:8, :4] = 0                                    # hard edges: the clip and the rounding
    ref = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BILINEAR))
    got = TI.resize_bilinear_u8(img, dst[0], dst[1])
    assert got.dtype == np.uint8 and np.array_equal(got, ref)
    for n_in, n_out in zip(src, dst):
        t = TI.resample_tables(n_in, n_out)
        assert t.bounds.dtype == np.int32 and t.coefs.dtype == np.int32 and t.bounds.shape == (n_out, 2)
        assert (t.bounds[:, 0] >= 0).all() and (t.bounds[:, 0] + t.bounds[:, 1] <= n_in).all()
        assert (t.bounds[:, 1] >= 1).all() and (t.bounds[:, 1] <= t.coefs.shape[1]).all()
        assert (np.diff(t.bounds[:, 0]) >= 0).all() and (np.diff(t.bounds.sum(1)) >= 0).all()   # the tile's row range
        assert TI.resample_tables(n_in, n_out) is t     # cached
        # the sums of a pass fit int32
        assert 255 * int(t.coefs.astype(np.int64).sum(1).max()) + (1 << 21) < 2 ** 31


@pytest.mark.parametrize("n_in,n_out", [(53, 69), (45, 30), (64, 20), (24, 24)])
def test_nearest_index_equals_interpolate(n_in, n_out):
    ref = F.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None, None], (1, n_out), mode="nearest")[0, 0, 0]
    got = TI.nearest_index(n_in, n_out)
    assert got.dtype == np.int32 and np.array_equal(got, ref.numpy().astype(np.int32))


def test_color_draw_equals_apply_image():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    aug = T.ColorAugSSD()
    seen = set()
    for s in range(48):
        random.seed(s)
        ref = aug.apply_image(img)
        state = random.getstate()
        random.seed(s)
        p = aug.draw()
        assert random.getstate() == state                # the same draws consumed
        assert np.array_equal(aug.apply_params(img, p), ref), (s, p)
        seen.add((p.brightness, p.order, p.contrast, p.saturation, p.hue))
    assert len(seen) > 16                                # both orders, every flag on and off


def _write_pngs(tmp, shapes, n_classes=5, seed=0):
    img_dir, gt_dir = os.path.join(tmp, "img"), os.path.join(tmp, "gt")
    os.makedirs(img_dir)
    os.makedirs(gt_dir)
    rng = np.random.default_rng(seed)
    for i, (h, w) in enumerate(shapes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(img_dir, f"{i:03d}.png"))
        lab = rng.integers(0, n_classes, (h // 8 + 1, w // 8 + 1), dtype=np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        lab[:3] = 255
        Image.fromarray(lab).save(os.path.join(gt_dir, f"{i:03d}.png"))
    return load_sem_seg(gt_dir, img_dir, gt_ext="png", image_ext="png")


def reference_cfg(**over):
    """The reference's training input configuration (configs/vitb_384.yaml)."""
    cfg = tiny_cfg()
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", "(384,)", "INPUT.CROP.ENABLED", "True", "INPUT.CROP.TYPE", "absolute",
                         "INPUT.CROP.SIZE", "(384, 384)", "INPUT.COLOR_AUG_SSD", "True", "INPUT.SIZE_DIVISIBILITY", "384"])
    for k, v in over.items():
        cfg.merge_from_list([k, v])
    return cfg


def test_reference_apply_equals_the_mapper_step_by_step(tmp_path):
    """MaskFormerSemanticDatasetMapper's own transforms, one after the other, recording what each drew;
    reference_apply with those parameters gives the mapper's image and labels."""
    dicts = _write_pngs(str(tmp_path), [(300, 500), (500, 420), (384, 384)])
    cfg = reference_cfg()
    mapper = MaskFormerSemanticDatasetMapper(cfg, True)
    flips = 0
    for k, d in enumerate(dicts * 2):
        image = read_image(d["file_name"], "RGB")
        sem = read_image(d["sem_seg_file_name"], None)
        h, w = image.shape[:2]
        random.seed(k)
        np.random.seed(k)
        img, lab = image, sem.astype("double")
        params = TI.TrainParams(h, w, h, w, [], False, None)
        for aug in mapper.tfm_gens:
            if isinstance(aug, T.ColorAugSSD):
                state = random.getstate()
                params.color = aug.draw()
                random.setstate(state)
            t = aug.get_transform(img, lab)
            img, lab = t.apply_image(img), t.apply_segmentation(lab)
            if isinstance(t, T.ResizeTransform):
                params.nh, params.nw = t.new_h, t.new_w
            elif isinstance(t, T.CropTransform):
                params.candidates = [(t.y0, t.x0, t.h, t.w)]
            elif isinstance(t, T.HFlipTransform):
                params.flip = True
                flips += 1
        random.seed(k)
        np.random.seed(k)
        out = mapper(d)                                   # the mapper itself, same streams
        got_img, got_sem = TI.reference_apply(params, image, sem, ignore_label=mapper.ignore_label, size_divisibility=384)
        assert got_img.dtype == torch.uint8 and got_sem.dtype == torch.int64
        assert torch.equal(got_img, out["image"]) and torch.equal(got_sem, out["sem_seg"])
        assert tuple(out["ori_size"]) == params.candidates[0][2:]
    assert 0 < flips < 6


def test_candidate_rule():
    sem = np.full((40, 40), 255.0)
    sem[:20, :20] = 1                                     # window A: one class only            -> fails
    sem[:20, 20:] = 2
    sem[0:5, 20:40] = 3                                   # window B: 300 of class 2, 100 of 3  -> 0.75 exactly
    sem[20:, 20:30] = 4
    sem[20:, 30:] = 5                                     # window D: half / half               -> passes
    A, Bw, Cw, D = (0, 0, 20, 20), (0, 20, 20, 20), (20, 0, 20, 20), (20, 20, 20, 20)
    assert not TI.candidate_passes(sem[:20, :20], 0.75, 255)
    assert not TI.candidate_passes(sem[:20, 20:], 0.75, 255)          # max == sum * max_area: strict
    assert TI.candidate_passes(sem[:20, 20:], 0.76, 255)
    assert not TI.candidate_passes(sem[20:, :20], 0.75, 255)          # only the ignore label
    assert TI.candidate_passes(sem[20:, 20:], 0.75, 255)
    assert TI.select_candidate(sem, [D, A], 0.75, 255) == 0           # the first passes
    assert TI.select_candidate(sem, [A, Bw, Cw, D, A], 0.75, 255) == 3
    assert TI.select_candidate(sem, [A, Bw, Cw], 0.75, 255) == 2      # all fail: the last
    # the same rule as RandomCropCategoryArea (its loop leaves the last draw when none passes)
    p = TI.TrainParams(40, 40, 40, 40, [A, Bw, Cw, D, A])
    img = np.zeros((40, 40, 3), np.uint8)
    _, lab = TI.reference_apply(p, img, sem.astype(np.uint8), max_area=0.75)
    assert torch.equal(lab, torch.from_numpy(sem[20:, 20:].astype(np.int64)))


def test_draw_train_params():
    s = TI.TrainAugSettings(min_sizes=(384,), crop_size=(384, 384), max_area=0.75, color_aug=True)
    a = TI.draw_train_params(s, 300, 500, TI.image_rng(3, 0, 7, 1))
    b = TI.draw_train_params(s, 300, 500, TI.image_rng(3, 0, 7, 1))
    c = TI.draw_train_params(s, 300, 500, TI.image_rng(3, 0, 7, 2))
    assert a == b and a != c
    assert (a.nh, a.nw) == T.resize_output_shape(300, 500, 384, 1333) and len(a.candidates) == TI.N_CANDIDATES
    for y0, x0, ch, cw in a.candidates:
        assert (ch, cw) == (384, 384) and 0 <= y0 <= a.nh - ch and 0 <= x0 <= a.nw - cw
    one = TI.draw_train_params(TI.TrainAugSettings(min_sizes=(0,), crop_enabled=False), 30, 50, TI.image_rng(0, 0, 0, 0))
    assert (one.nh, one.nw) == (30, 50) and one.candidates == [(0, 0, 30, 50)] and one.color is None


def test_plan_batch_validates():
    p = TI.TrainParams(30, 50, 60, 100, [(0, 0, 60, 100)])
    with pytest.raises(ValueError, match="exceeds"):
        TI.plan_batch([p], [np.uint8], 96, select=False)
    with pytest.raises(ValueError, match="leaves"):
        TI.plan_batch([TI.TrainParams(30, 50, 60, 100, [(10, 0, 60, 100)])], [np.uint8], 128, select=False)
    lay = TI.plan_batch([p, p], [np.uint8, np.int32], 128, select=False, guard=64)
    assert lay.descs["lab_off"][1] % 4 == 0 and lay.descs["img_off"][0] >= 64
    assert lay.descs["xb_off"][0] == lay.descs["xb_off"][1]              # tables shared between images


def test_training_sampler():
    a = list(itertools.islice(iter(TrainingSampler(10, True, 5, 0, 2)), 20))
    b = list(itertools.islice(iter(TrainingSampler(10, True, 5, 1, 2)), 20))
    for e in range(4):                                    # the two ranks partition every epoch
        assert sorted(a[5 * e:5 * e + 5] + b[5 * e:5 * e + 5]) == list(range(10))
    assert a == list(itertools.islice(iter(TrainingSampler(10, True, 5, 0, 2)), 20))
    assert a != list(itertools.islice(iter(TrainingSampler(10, True, 6, 0, 2)), 20))
    assert list(itertools.islice(iter(TrainingSampler(3, False, 0, 0, 1)), 7)) == [0, 1, 2, 0, 1, 2, 0]


def test_build_train_loader_host(tmp_path):
    dicts = _write_pngs(str(tmp_path), [(300, 500), (400, 390), (384, 384)])
    cfg = reference_cfg(**{"SOLVER.IMS_PER_BATCH": "2"})
    assert cfg.MODEL.CATSEG_HIP.TRAIN_INPUT == "host"
    loader = build_train_loader(dicts, cfg=cfg, num_workers=0, seed=1)
    batches = list(itertools.islice(iter(loader), 3))     # more than one epoch of 3 images
    for batch in batches:
        assert isinstance(batch, list) and len(batch) == 2
        for d in batch:
            assert {"image", "sem_seg", "file_name", "height", "width", "ori_size", "instances"} <= set(d)
            assert tuple(d["image"].shape) == (3, 384, 384) and d["image"].dtype == torch.uint8
            assert tuple(d["sem_seg"].shape) == (384, 384) and d["sem_seg"].dtype == torch.int64


def test_unknown_train_input_is_an_error(tmp_path):
    dicts = _write_pngs(str(tmp_path), [(64, 64)])
    with pytest.raises(ValueError, match="TRAIN_INPUT"):
        build_train_loader(dicts, cfg=reference_cfg(**{"MODEL.CATSEG_HIP.TRAIN_INPUT": "gpu"}), num_workers=0)


def test_raw_train_mapper(tmp_path):
    dicts = _write_pngs(str(tmp_path), [(30, 50)])
    out = TI.RawTrainMapper(reference_cfg())(dicts[0])
    assert set(out) == {"file_name", "height", "width", "image_raw", "sem_seg_raw"}
    assert tuple(out["image_raw"].shape) == (30, 50, 3) and out["image_raw"].dtype == torch.uint8
    assert tuple(out["sem_seg_raw"].shape) == (30, 50) and out["sem_seg_raw"].dtype == torch.uint8
    # a 16-bit label file widens to int32
    path = os.path.join(str(tmp_path), "gt", "000.png")
    Image.fromarray(np.full((30, 50), 847, dtype=np.uint16)).save(path)
    wide = TI.RawTrainMapper(reference_cfg())(dicts[0])["sem_seg_raw"]
    assert wide.dtype == torch.int32 and int(wide[0, 0]) == 847


def test_device_augment_rejects_what_the_host_mapper_cannot_do():
    """Construction and call-time errors are raised before anything touches the GPU."""
    from cat_seg.data.device_input import DeviceTrainAugment
    with pytest.raises(ValueError, match="SIZE_DIVISIBILITY"):
        DeviceTrainAugment(reference_cfg(**{"INPUT.SIZE_DIVISIBILITY": "-1"}), "cuda")
    with pytest.raises(ValueError, match="CROP.TYPE"):
        DeviceTrainAugment(reference_cfg(**{"INPUT.CROP.TYPE": "centre"}), "cuda")
    with pytest.raises(ValueError, match="4096"):
        DeviceTrainAugment(reference_cfg(**{"INPUT.CROP.SINGLE_CATEGORY_MAX_AREA": "0.75"}), "cuda", n_labels=5000)
    DeviceTrainAugment(reference_cfg(), "cuda", n_labels=5000)             # no constraint: nothing is counted
    # the crop (here the whole resized image: cropping off) exceeds the canvas: the host mapper's negative pad
    aug = DeviceTrainAugment(reference_cfg(**{"INPUT.CROP.ENABLED": "False"}), "cuda")
    raw = {"image_raw": torch.zeros(300, 500, 3, dtype=torch.uint8), "sem_seg_raw": torch.zeros(300, 500, dtype=torch.uint8)}
    with pytest.raises(ValueError, match="exceeds"):
        aug([raw])
