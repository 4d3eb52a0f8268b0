"""The device half of MODEL.CATSEG_HIP.TRAIN_INPUT "device": a batch of decoded images (RawTrainMapper)
-> the model's training inputs, augmented by csrc/train_input.hip.

Per batch: the parameters of every image are drawn on the host (train_input.draw_train_params), the
source pixels and the descriptors / tables / candidates go through two pinned staging buffers and two
non-blocking H2D copies, then at most two launches run on the current stream (catseg_train_crop_select
only with the category-area constraint on, catseg_train_augment).  Nothing comes back to the host.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from . import train_input as TI


class DeviceTrainAugment:
    """`__call__(list of RawTrainMapper dicts)` -> the list of dicts CATSeg's training branch takes:
    {"image": (3, S, S) uint8 device view, "sem_seg": (S, S) int64 device view, "file_name", "height",
    "width", "ori_size"}, S = INPUT.SIZE_DIVISIBILITY; the views of one batch share two fresh tensors.
    "instances" (the host mapper's per-class masks) is not produced: the training branch never reads it.
    "ori_size" is the crop's extent (the candidates' common extent under the area constraint, where the
    chosen window itself stays on the device); None if the candidates differ in extent.

    Image i of the `batch_index`-th call draws from its own Generator seeded with (seed, rank,
    batch_index, i): the stream of batches depends on the seed alone.  The staging buffers live in two slots
    guarded by events, as CATSeg._stage_canvas does: the host runs at most two batches ahead of the copies."""

    def __init__(self, cfg=None, device="cuda", seed: int = 0, *, rank: int = 0,
                 settings: Optional[TI.TrainAugSettings] = None, n_labels: Optional[int] = None):
        s = settings if settings is not None else TI.TrainAugSettings.from_cfg(cfg)
        if s.size_divisibility <= 0:
            raise ValueError(f"DeviceTrainAugment needs INPUT.SIZE_DIVISIBILITY > 0 (the side of the padded canvas), "
                             f"got {s.size_divisibility}")
        if s.crop_enabled and s.crop_type not in TI.CROP_TYPES:
            raise ValueError(f"INPUT.CROP.TYPE {s.crop_type!r}: expected one of {TI.CROP_TYPES}")
        if n_labels is None:
            n_labels = 256
            if cfg is not None and s.ignore_label >= 256:
                n_labels = int(cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES)
        if s.constrained and n_labels > TI.MAX_LABELS:
            raise ValueError(f"the category-area constraint counts at most {TI.MAX_LABELS} labels on the device, "
                             f"got {n_labels}")
        self.settings, self.n_labels = s, int(n_labels)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DeviceTrainAugment runs on the GPU: pass a cuda device")
        self.seed, self.rank, self.batch_index = int(seed), int(rank), 0
        self._slots = [{"pix_host": None, "pix_dev": None, "meta_host": None, "meta_dev": None, "done": None}
                       for _ in range(2)]
        self._next = 0
        self._select_ws = {}
        self.last_params: List[TI.TrainParams] = []

    # -------------------------------------------------------------------------------------------- staging
    def _buffer(self, slot, name, n, dtype):
        host = slot[name + "_host"]
        if host is None or host.numel() < n:
            cap = max(n, 0 if host is None else 2 * host.numel())
            slot[name + "_host"] = torch.empty(cap, dtype=dtype, pin_memory=True)
            slot[name + "_dev"] = torch.empty(cap, dtype=dtype, device=self.device)
        return slot[name + "_host"], slot[name + "_dev"]

    def draw(self, raws: Sequence[dict]) -> List[TI.TrainParams]:
        """The parameters of the next batch (advances the batch counter)."""
        k = self.batch_index
        self.batch_index += 1
        return [TI.draw_train_params(self.settings, int(r["image_raw"].shape[0]), int(r["image_raw"].shape[1]),
                                     TI.image_rng(self.seed, self.rank, k, i)) for i, r in enumerate(raws)]

    def apply(self, raws: Sequence[dict], params: Sequence[TI.TrainParams]):
        """Stage and launch one batch with the given parameters: (images (B, 3, S, S) uint8, targets
        (B, S, S) int64) on the device."""
        s = self.settings
        S, B = s.size_divisibility, len(raws)
        images = [np.asarray(r["image_raw"]) for r in raws]
        labels = [np.asarray(r["sem_seg_raw"]) for r in raws]
        select = s.constrained
        layout = TI.plan_batch(params, [l.dtype for l in labels], S, select=select)
        slot = self._slots[self._next]
        self._next ^= 1
        if slot["done"] is not None and not slot["done"].query():
            slot["done"].synchronize()          # this slot's previous copies have read the pinned buffers
        pix_host, pix_dev = self._buffer(slot, "pix", layout.pixel_bytes, torch.uint8)
        meta_host, meta_dev = self._buffer(slot, "meta", layout.meta_words, torch.int32)
        TI.fill_batch(layout, images, labels, pix_host.numpy(), meta_host.numpy())
        with torch.cuda.device(self.device):
            pix_dev[:layout.pixel_bytes].copy_(pix_host[:layout.pixel_bytes], non_blocking=True)
            meta_dev[:layout.meta_words].copy_(meta_host[:layout.meta_words], non_blocking=True)
            out = torch.empty(B, 3, S, S, dtype=torch.uint8, device=self.device)
            tgt = torch.empty(B, S, S, dtype=torch.int64, device=self.device)
            crops = None
            if select:
                # one zeroed workspace per (B, n_cand): the kernel leaves its counters zero, its flags not
                ws = self._select_ws.get((B, layout.n_cand))
                if ws is None:
                    ws = self._select_ws[(B, layout.n_cand)] = torch.zeros(B * (layout.n_cand + 1), dtype=torch.int32,
                                                                           device=self.device)
                crops = torch.empty(B, 4, dtype=torch.int32, device=self.device)
                ops.train_crop_select(pix_dev, meta_dev, layout.cand_off, B, layout.n_cand, self.n_labels,
                                      s.ignore_label, s.max_area, ws, crops)
            ops.train_augment(pix_dev, meta_dev, B, out, tgt, s.ignore_label, crops)
            slot["done"] = torch.cuda.Event()
            slot["done"].record(torch.cuda.current_stream(self.device))
        return out, tgt

    def __call__(self, raws: Sequence[dict]) -> List[dict]:
        params = self.draw(raws)
        self.last_params = params
        out, tgt = self.apply(raws, params)
        batch = []
        for i, (r, p) in enumerate(zip(raws, params)):
            d = {k: v for k, v in r.items() if k not in ("image_raw", "sem_seg_raw")}
            extents = {(c[2], c[3]) for c in p.candidates}
            d["ori_size"] = next(iter(extents)) if len(extents) == 1 else None
            d["image"], d["sem_seg"] = out[i], tgt[i]
            batch.append(d)
        return batch
