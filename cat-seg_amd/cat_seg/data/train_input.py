"""Host side of the device training-input path (MODEL.CATSEG_HIP.TRAIN_INPUT "device"): the random
parameters of the reference's training mapper drawn ahead of the pixels, the tables the kernels read,
the batch packed for them, and the host composition they must equal.

The yardstick is the existing host path: `transforms.py` as `MaskFormerSemanticDatasetMapper.__call__`
composes it (mask_former_semantic_dataset_mapper.py:62-147): ResizeShortestEdge, RandomCropCategoryArea,
ColorAugSSD, RandomFlip, pad to SIZE_DIVISIBILITY.  With the draws pinned every step is a pure function of
the pixels; `reference_apply` is that function, and csrc/train_input.hip computes it per output pixel.

  resample_tables   PIL's bilinear resize of uint8 restated: per axis the bounds and the int32
                    coefficients (22 fraction bits) of Resample.c
  nearest_index     the source index per output index of F.interpolate(mode="nearest")
  draw_train_params the geometric and colour parameters of one image, from its own numpy Generator
  reference_apply   the host composition with those parameters
  plan_batch /      images, labels, descriptors, tables and candidates laid out, validated and written into
  fill_batch        the two buffers the kernels take
  RawTrainMapper    the worker-side mapper: decode only
"""
from __future__ import annotations

import copy
import functools
import math
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import transforms as T
from .._lib import TrainImageDesc

PRECISION_BITS = 22          # PIL Resample.c: 32 - 8 - 2
N_CANDIDATES = 10            # RandomCrop_CategoryAreaConstraint's draws
MAX_LABELS = 4096            # LDS histogram bins of catseg_train_crop_select
CROP_TYPES = ("absolute", "relative", "relative_range", "absolute_range")


class ResampleTable(NamedTuple):
    bounds: np.ndarray       # (out, 2) int32: first source index, tap count
    coefs: np.ndarray        # (out, ksize) int32, zero past the tap count


@functools.lru_cache(maxsize=256)
def resample_tables(in_size: int, out_size: int) -> ResampleTable:
    """The bounds and fixed-point coefficients of one axis of PIL's `Image.resize(..., BILINEAR)` on
    uint8 (Resample.c precompute_coeffs + normalize_coeffs_8bpc): a pass computes
    clip8((sum(px * k) + 2^21) >> 22).  An axis whose size does not change has no pass in PIL; its table
    here is the identity (one tap of 2^22), which that formula maps to the pixel itself.  Cached per
    (in, out); the arrays are read-only."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size), np.ones(out_size, dtype=np.int64)], 1).astype(np.int32)
        coefs = np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
    else:
        scale = in_size / out_size
        filterscale = max(scale, 1.0)
        support = 1.0 * filterscale                      # the triangle filter's support is 1
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / filterscale
        bounds = np.zeros((out_size, 2), dtype=np.int32)
        coefs = np.zeros((out_size, ksize), dtype=np.int32)
        for i in range(out_size):
            center = (i + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), in_size) - xmin
            wgt = 1.0 - np.abs((np.arange(xmax) + xmin - center + 0.5) * ss)
            wgt = np.where(wgt > 0.0, wgt, 0.0)
            total = 0.0
            for v in wgt.tolist():                       # float64, left to right as the C loop (np.sum pairs)
                total += v
            if total != 0.0:
                wgt = wgt / total
            bounds[i] = (xmin, xmax)
            coefs[i, :xmax] = (0.5 + wgt * (1 << PRECISION_BITS)).astype(np.int64)
    bounds.setflags(write=False)
    coefs.setflags(write=False)
    return ResampleTable(bounds, coefs)


def resample_axis_u8(a: np.ndarray, table: ResampleTable, axis: int) -> np.ndarray:
    """One pass of the resize over `axis` of a uint8 array, as the kernel and PIL compute it."""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((len(table.bounds),) + a.shape[1:], dtype=np.uint8)
    for i, (lo, n) in enumerate(table.bounds):
        k = table.coefs[i, :n].astype(np.int64).reshape((n,) + (1,) * (a.ndim - 1))
        s = (a[lo:lo + n] * k).sum(0) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(s >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_bilinear_u8(img: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    """PIL's two-pass resize from the tables: horizontal first, rounded to uint8, then vertical."""
    h, w = img.shape[:2]
    if w != new_w:
        img = resample_axis_u8(img, resample_tables(w, new_w), 1)
    if h != new_h:
        img = resample_axis_u8(img, resample_tables(h, new_h), 0)
    return img


@functools.lru_cache(maxsize=256)
def nearest_index(in_size: int, out_size: int) -> np.ndarray:
    """Source index per output index of `F.interpolate(mode="nearest")`:
    min(int(floor(dst * float32(in / out))), in - 1), the scale and the product in float32."""
    scale = np.float32(in_size) / np.float32(out_size)
    idx = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    idx = np.minimum(idx, in_size - 1).astype(np.int32)
    idx.setflags(write=False)
    return idx


# ------------------------------------------------------------------------------------------------ parameters
@dataclass(frozen=True)
class TrainAugSettings:
    """What the training mapper reads from the config (MaskFormerSemanticDatasetMapper.__init__)."""
    min_sizes: Tuple[int, ...] = (384,)
    max_size: int = 1333
    sampling: str = "choice"
    crop_enabled: bool = True
    crop_type: str = "absolute"
    crop_size: Tuple[float, float] = (384, 384)
    max_area: float = 1.0
    color_aug: bool = False
    flip_prob: float = 0.5
    size_divisibility: int = 384
    ignore_label: int = 255

    @classmethod
    def from_cfg(cls, cfg) -> "TrainAugSettings":
        from .dataset_mappers import _cfg_get
        inp = cfg.INPUT
        try:
            from .catalog import MetadataCatalog
            ignore = MetadataCatalog.get(cfg.DATASETS.TRAIN[0]).ignore_label
        except (AttributeError, IndexError, KeyError):
            ignore = cfg.MODEL.SEM_SEG_HEAD.IGNORE_VALUE
        return cls(min_sizes=tuple(int(s) for s in inp.MIN_SIZE_TRAIN), max_size=int(_cfg_get(inp, "MAX_SIZE_TRAIN", 1333)),
                   sampling=str(_cfg_get(inp, "MIN_SIZE_TRAIN_SAMPLING", "choice")), crop_enabled=bool(inp.CROP.ENABLED),
                   crop_type=str(inp.CROP.TYPE), crop_size=tuple(inp.CROP.SIZE),
                   max_area=float(inp.CROP.SINGLE_CATEGORY_MAX_AREA), color_aug=bool(_cfg_get(inp, "COLOR_AUG_SSD", False)),
                   size_divisibility=int(inp.SIZE_DIVISIBILITY), ignore_label=int(ignore))

    @property
    def constrained(self) -> bool:
        return self.crop_enabled and self.max_area < 1.0


@dataclass
class TrainParams:
    """The parameters of one image: source and resized size, the crop candidates (y0, x0, ch, cw) in the
    resized image (one, or N_CANDIDATES with the area constraint on), flip and the colour record."""
    h: int
    w: int
    nh: int
    nw: int
    candidates: List[Tuple[int, int, int, int]]
    flip: bool = False
    color: Optional[T.ColorParams] = None


class _GeneratorRandom:
    """randrange / uniform / randint of `random` on a numpy Generator (ColorAugSSD.draw)."""

    def __init__(self, rng: np.random.Generator):
        self.rng = rng

    def randrange(self, n):
        return int(self.rng.integers(n))

    def uniform(self, a, b):
        return a + (b - a) * float(self.rng.random())

    def randint(self, a, b):
        return int(self.rng.integers(a, b + 1))


def _crop_size_for(s: TrainAugSettings, h: int, w: int, rng: np.random.Generator) -> Tuple[int, int]:
    """RandomCropCategoryArea.crop_size_for on `rng`."""
    ch, cw = s.crop_size
    if s.crop_type == "relative":
        return int(h * ch + 0.5), int(w * cw + 0.5)
    if s.crop_type == "relative_range":
        rh, rw = np.asarray(s.crop_size, dtype=np.float32)
        rh, rw = rh + rng.random() * (1 - rh), rw + rng.random() * (1 - rw)
        return int(h * rh + 0.5), int(w * rw + 0.5)
    if s.crop_type == "absolute":
        return min(int(ch), h), min(int(cw), w)
    if s.crop_type == "absolute_range":
        lo, hi = int(ch), int(cw)
        return int(rng.integers(min(h, lo), min(h, hi) + 1)), int(rng.integers(min(w, lo), min(w, hi) + 1))
    raise ValueError(f"Unknown crop type {s.crop_type}")


def draw_train_params(settings: TrainAugSettings, h: int, w: int, rng: np.random.Generator) -> TrainParams:
    """Every random choice of the training mapper for one h x w image, drawn from `rng` in the mapper's
    order (resize choice, crop candidates, colour, flip) before a pixel is touched.

    `rng` is the image's own Generator (the loader seeds it from (seed, rank, batch index, index in the
    batch)), so a batch is reproducible whatever the worker count.  With the area constraint on this draws
    all N_CANDIDATES crop candidates, where the host mapper stops drawing at the first one that passes: the
    two paths consume randomness differently and do not produce the same stream of crops.  That is
    intended; the distribution of the chosen crop is the same."""
    if settings.sampling == "range":
        size = int(rng.integers(settings.min_sizes[0], settings.min_sizes[-1] + 1))
    else:
        size = int(settings.min_sizes[int(rng.integers(len(settings.min_sizes)))])
    nh, nw = (h, w) if size == 0 else T.resize_output_shape(h, w, size, settings.max_size)
    if settings.crop_enabled:
        cands = []
        for _ in range(N_CANDIDATES if settings.constrained else 1):
            ch, cw = _crop_size_for(settings, nh, nw, rng)
            y0 = int(rng.integers(nh - ch + 1))
            x0 = int(rng.integers(nw - cw + 1))
            cands.append((y0, x0, ch, cw))
    else:
        cands = [(0, 0, nh, nw)]
    color = T.ColorAugSSD().draw(_GeneratorRandom(rng)) if settings.color_aug else None
    flip = bool(rng.random() < settings.flip_prob)
    return TrainParams(h, w, nh, nw, cands, flip, color)


def image_rng(seed: int, rank: int, batch_index: int, index: int) -> np.random.Generator:
    return np.random.default_rng([int(seed), int(rank), int(batch_index), int(index)])


# ------------------------------------------------------------------------------------------------ host reference
def candidate_passes(window: np.ndarray, max_area: float, ignored: Optional[int]) -> bool:
    """RandomCropCategoryArea's test of one window of the label map (float64 comparison, strict)."""
    labels, cnt = np.unique(window, return_counts=True)
    if ignored is not None:
        cnt = cnt[labels != ignored]
    return bool(len(cnt) > 1 and np.max(cnt) < np.sum(cnt) * max_area)


def select_candidate(sem: np.ndarray, candidates: Sequence[Tuple[int, int, int, int]], max_area: float,
                     ignored: Optional[int]) -> int:
    """Index of the first candidate that passes in the (resized) label map `sem`, else the last."""
    for i, (y0, x0, ch, cw) in enumerate(candidates):
        if candidate_passes(sem[y0:y0 + ch, x0:x0 + cw], max_area, ignored):
            return i
    return len(candidates) - 1


def reference_apply(params: TrainParams, image: np.ndarray, label: np.ndarray, *, ignore_label: int = 255,
                    size_divisibility: int = -1, max_area: float = 1.0):
    """The host composition of the existing transforms with the parameters pinned: what
    MaskFormerSemanticDatasetMapper.__call__ computes once its draws are `params`.  `image` HWC uint8,
    `label` HW of any integer type.  Returns (CHW uint8 tensor, HW int64 tensor), padded right and bottom
    to `size_divisibility` when that is positive.  With more than one candidate the crop is the first that
    passes the area rule in the resized label map, else the last."""
    image = np.asarray(image)
    sem = np.asarray(label).astype("double")
    p = params
    assert image.shape[:2] == (p.h, p.w) and sem.shape == (p.h, p.w), (image.shape, sem.shape, p.h, p.w)
    if (p.nh, p.nw) != (p.h, p.w):
        tf = T.ResizeTransform(p.h, p.w, p.nh, p.nw)
        image, sem = tf.apply_image(image), tf.apply_segmentation(sem)
    if len(p.candidates) == 1:
        y0, x0, ch, cw = p.candidates[0]
    else:
        y0, x0, ch, cw = p.candidates[select_candidate(sem, p.candidates, max_area, ignore_label)]
    tf = T.CropTransform(x0, y0, cw, ch)
    image, sem = tf.apply_image(image), tf.apply_segmentation(sem)
    if p.color is not None:
        image = T.ColorAugSSD().apply_params(image, p.color)
    if p.flip:
        tf = T.HFlipTransform(image.shape[1])
        image, sem = tf.apply_image(image), tf.apply_segmentation(sem)
    image = torch.as_tensor(np.ascontiguousarray(image.transpose(2, 0, 1)))
    sem = torch.as_tensor(sem.astype("long"))
    if size_divisibility > 0:
        h, w = image.shape[-2:]
        pad = [0, size_divisibility - w, 0, size_divisibility - h]
        image = torch.nn.functional.pad(image, pad, value=128).contiguous()
        sem = torch.nn.functional.pad(sem, pad, value=ignore_label).contiguous()
    return image, sem.long()


# ------------------------------------------------------------------------------------------------ packing
# include/catseg_hip_train.h CatsegTrainImageDesc
DESC_DTYPE = np.dtype(TrainImageDesc)
assert DESC_DTYPE.itemsize == 128        # the header's own promise
DESC_WORDS = DESC_DTYPE.itemsize // 4
PLANE_ALIGN = 64


def _align(n: int, a: int = PLANE_ALIGN) -> int:
    return -(-n // a) * a


class BatchLayout(NamedTuple):
    """Where everything of one packed batch lies.  `pixels` bytes: per image the HWC plane and the label
    plane at img_off / lab_off, `guard` bytes before, between and after the planes.  `meta` int32 words:
    the descriptors [B][DESC_WORDS] at 0, the candidates [B][n_cand][4] at cand_off, then the tables."""
    pixel_bytes: int
    meta_words: int
    cand_off: int
    n_cand: int
    descs: np.ndarray                  # (B,) DESC_DTYPE
    cands: np.ndarray                  # (B, n_cand, 4) int32
    tables: List[Tuple[int, np.ndarray]]


def plan_batch(params: Sequence[TrainParams], label_dtypes: Sequence[np.dtype], S: int, *, select: bool,
               guard: int = 0) -> BatchLayout:
    """Lay a batch out and validate it: every index the kernels form from the descriptors stays inside the
    buffers.  `select`: the crop comes from catseg_train_crop_select (crop_sel = image index), else from the
    first candidate.  Raises ValueError when a crop exceeds the canvas S."""
    B = len(params)
    n_cand = max(len(p.candidates) for p in params) if select else 1
    descs = np.zeros(B, dtype=DESC_DTYPE)
    cands = np.zeros((B, n_cand, 4), dtype=np.int32)
    tables: List[Tuple[int, np.ndarray]] = []
    placed = {}
    word = B * DESC_WORDS
    cand_off = word
    word += cands.size

    def place(key, make):
        nonlocal word
        if key not in placed:
            arr = np.ascontiguousarray(make(), dtype=np.int32).reshape(-1)
            placed[key] = word
            tables.append((word, arr))
            word += arr.size
        return placed[key]

    byte = _align(guard) if guard else 0
    for b, (p, ldt) in enumerate(zip(params, label_dtypes)):
        lab_bytes = np.dtype(ldt).itemsize
        if lab_bytes not in (1, 4):
            raise ValueError(f"label planes are uint8 or int32, got {ldt}")
        if min(p.h, p.w, p.nh, p.nw) <= 0:
            raise ValueError(f"empty image {(p.h, p.w)} -> {(p.nh, p.nw)}")
        d = descs[b]
        d["img_off"] = byte
        byte = _align(byte + p.h * p.w * 3 + guard)
        d["lab_off"] = byte
        byte = _align(byte + p.h * p.w * lab_bytes + guard)
        d["h"], d["w"], d["nh"], d["nw"] = p.h, p.w, p.nh, p.nw
        tx, ty = resample_tables(p.w, p.nw), resample_tables(p.h, p.nh)
        d["xb_off"] = place(("b", p.w, p.nw), lambda: tx.bounds)
        d["xk_off"] = place(("k", p.w, p.nw), lambda: tx.coefs)
        d["kx"] = tx.coefs.shape[1]
        d["yb_off"] = place(("b", p.h, p.nh), lambda: ty.bounds)
        d["yk_off"] = place(("k", p.h, p.nh), lambda: ty.coefs)
        d["ky"] = ty.coefs.shape[1]
        d["nx_off"] = place(("n", p.w, p.nw), lambda: nearest_index(p.w, p.nw))
        d["ny_off"] = place(("n", p.h, p.nh), lambda: nearest_index(p.h, p.nh))
        wins = list(p.candidates) if select else [p.candidates[0]]
        if select and len(wins) != n_cand:
            raise ValueError("every image of a batch has the same number of crop candidates")
        for (y0, x0, ch, cw) in wins:
            if not (ch >= 1 and cw >= 1 and y0 >= 0 and x0 >= 0 and y0 + ch <= p.nh and x0 + cw <= p.nw):
                raise ValueError(f"crop {(y0, x0, ch, cw)} leaves the resized image {(p.nh, p.nw)}")
            if ch > S or cw > S:
                raise ValueError(f"crop {ch} x {cw} exceeds INPUT.SIZE_DIVISIBILITY {S}: the host mapper fails "
                                 "there on a negative pad")
        cands[b] = np.asarray(wins, dtype=np.int32)
        d["crop"] = cands[b, 0]
        d["crop_sel"] = b if select else -1
        d["flip"], d["lab_bytes"] = int(p.flip), lab_bytes
        c = p.color
        if c is not None:
            d["bright"], d["order"], d["contrast"], d["sat"], d["hue"] = c.brightness, c.order, c.contrast, c.saturation, c.hue
            d["hue_delta"], d["beta"], d["c_alpha"], d["s_alpha"] = c.hue_delta, c.beta, c.contrast_alpha, c.saturation_alpha
    return BatchLayout(byte, word, cand_off, n_cand, descs, cands, tables)


def fill_batch(layout: BatchLayout, images: Sequence[np.ndarray], labels: Sequence[np.ndarray], pixels: np.ndarray,
               meta: np.ndarray) -> None:
    """Write a planned batch into `pixels` (uint8, >= pixel_bytes) and `meta` (int32, >= meta_words)."""
    B = len(layout.descs)
    for b in range(B):
        d = layout.descs[b]
        h, w = int(d["h"]), int(d["w"])
        img, lab = np.asarray(images[b]), np.asarray(labels[b])
        if img.shape != (h, w, 3) or img.dtype != np.uint8 or lab.shape != (h, w) or lab.dtype.itemsize != int(d["lab_bytes"]):
            raise ValueError(f"image {b}: expected HWC uint8 {(h, w, 3)} and a label plane {(h, w)}, got "
                             f"{img.shape} {img.dtype} / {lab.shape} {lab.dtype}")
        o = int(d["img_off"])
        pixels[o:o + h * w * 3].reshape(h, w, 3)[...] = img
        o = int(d["lab_off"])
        pixels[o:o + lab.nbytes].view(lab.dtype).reshape(h, w)[...] = lab
    meta[:B * DESC_WORDS] = layout.descs.view(np.int32)
    meta[layout.cand_off:layout.cand_off + layout.cands.size] = layout.cands.reshape(-1)
    for off, arr in layout.tables:
        meta[off:off + arr.size] = arr


# ------------------------------------------------------------------------------------------------ worker side
class RawTrainMapper:
    """The worker-side mapper of the device path: decode the image and its label file, nothing else.
    Returns {"file_name", "height", "width", "image_raw": HWC uint8 tensor, "sem_seg_raw": HW uint8 or int32
    tensor} (16-bit label files widen to int32 here); resize, crop, colour, flip and pad run on the device
    (cat_seg.data.device_input.DeviceTrainAugment)."""

    def __init__(self, cfg=None, *, image_format: str = "RGB"):
        self.img_format = cfg.INPUT.FORMAT if cfg is not None else image_format

    def __call__(self, dataset_dict: dict) -> dict:
        from .dataset_mappers import check_image_size, read_image
        d = copy.deepcopy(dataset_dict)
        image = read_image(d["file_name"], self.img_format)
        check_image_size(d, image)
        if "sem_seg_file_name" not in d:
            raise ValueError(f"Cannot find 'sem_seg_file_name' for semantic segmentation dataset {d['file_name']}.")
        sem = read_image(d.pop("sem_seg_file_name"), None)
        if sem.ndim == 3:
            sem = sem[:, :, 0]
        if sem.dtype != np.uint8:
            sem = sem.astype(np.int32)
        if "annotations" in d:
            raise ValueError("Semantic segmentation dataset should not have 'annotations'.")
        d["image_raw"] = torch.from_numpy(np.array(image))          # a writable copy of PIL's buffer
        d["sem_seg_raw"] = torch.from_numpy(np.array(sem))
        return d
