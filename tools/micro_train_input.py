"""Training input per batch: the host composition against the device path.

Per source size, a batch of --batch decoded images -> 384 short edge / 384 x 384 crop / canvas 384 with the
colour augmentation on (the reference's training input), legs alternating within one process:

  host     cat_seg.data.train_input.reference_apply per image in this process (PIL / numpy; no decode)
  device   DeviceTrainAugment.apply: staging into the pinned buffers, both H2D copies and the launch, from
           HIP events around the call (the host's packing runs between them) and from a host clock around call + sync
  kernel   catseg_train_augment alone on staged buffers, HIP events around --inner launches

and the kernel's achieved bandwidth over its algorithmic bytes: the source pixels and labels the chosen
crops need plus the outputs.  Median and range over --reps.  Needs a GPU (no fallback).  One JSON document,
printed and written to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT]

from cat_seg import ops  # noqa: E402
from cat_seg._lib import require_gpu  # noqa: E402
from cat_seg.data import train_input as TI  # noqa: E402
from cat_seg.data.device_input import DeviceTrainAugment  # noqa: E402


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def algorithmic_bytes(params, label_bytes, S):
    """Source bytes the crops need (the rows and columns the two passes of the crop's pixels read, and the
    crop's labels) + the output bytes (3 uint8 planes and one int64 plane per canvas pixel)."""
    src = 0
    for p, lb in zip(params, label_bytes):
        y0, x0, ch, cw = p.candidates[0]
        ty, tx = TI.resample_tables(p.h, p.nh), TI.resample_tables(p.w, p.nw)
        rows = int(ty.bounds[y0 + ch - 1].sum() - ty.bounds[y0, 0])
        cols = int(tx.bounds[x0 + cw - 1].sum() - tx.bounds[x0, 0])
        src += rows * cols * 3 + ch * cw * lb
    return src, len(params) * S * S * 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 683, 2048, 3072], help="H W pairs")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="kernel launches per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_input", "micro.json"))
    a = ap.parse_args()
    require_gpu()
    S = 384
    settings = TI.TrainAugSettings(min_sizes=(S,), crop_size=(S, S), color_aug=True, size_divisibility=S)
    out = {"metric": "training input per batch", "unit": "ms", "batch": a.batch, "canvas": S, "device": torch.cuda.get_device_name(0),
           "sizes": []}
    for h, w in zip(a.sizes[::2], a.sizes[1::2]):
        rng = np.random.default_rng(h)
        raws = [{"image_raw": torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
                 "sem_seg_raw": torch.from_numpy(rng.integers(0, 171, (h // 32 + 1, w // 32 + 1), dtype=np.uint8)
                                                 .repeat(32, 0).repeat(32, 1)[:h, :w].copy())} for _ in range(a.batch)]
        aug = DeviceTrainAugment(None, "cuda", seed=0, settings=settings)
        params = aug.draw(raws)
        # correctness at the timed size first: faster and different is not faster
        img, tgt = aug.apply(raws, params)
        for b, (r, p) in enumerate(zip(raws, params)):
            ri, rt = TI.reference_apply(p, r["image_raw"].numpy(), r["sem_seg_raw"].numpy(), size_divisibility=S)
            assert torch.equal(img[b].cpu(), ri) and torch.equal(tgt[b].cpu(), rt), f"device != host at {h} x {w}"
        # staged buffers for the kernel-alone leg
        layout = TI.plan_batch(params, [np.uint8] * a.batch, S, select=False)
        pix, meta = np.zeros(layout.pixel_bytes, np.uint8), np.zeros(layout.meta_words, np.int32)
        TI.fill_batch(layout, [r["image_raw"].numpy() for r in raws], [r["sem_seg_raw"].numpy() for r in raws], pix, meta)
        pix_d, meta_d = torch.from_numpy(pix).cuda(), torch.from_numpy(meta).cuda()
        o_img = torch.empty(a.batch, 3, S, S, dtype=torch.uint8, device="cuda")
        o_tgt = torch.empty(a.batch, S, S, dtype=torch.int64, device="cuda")
        for _ in range(3):
            aug.apply(raws, params)
            ops.train_augment(pix_d, meta_d, a.batch, o_img, o_tgt, 255)
        torch.cuda.synchronize()
        host, dev_ev, dev_wall, kern = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for r, p in zip(raws, params):
                TI.reference_apply(p, r["image_raw"].numpy(), r["sem_seg_raw"].numpy(), size_divisibility=S)
            host.append((time.perf_counter() - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            aug.apply(raws, params)
            e1.record()
            torch.cuda.synchronize()
            dev_wall.append((time.perf_counter() - t0) * 1e3)
            dev_ev.append(e0.elapsed_time(e1))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                ops.train_augment(pix_d, meta_d, a.batch, o_img, o_tgt, 255)
            e1.record()
            torch.cuda.synchronize()
            kern.append(e0.elapsed_time(e1) / a.inner)
        src_b, out_b = algorithmic_bytes(params, [1] * a.batch, S)
        k = statistics.median(kern)
        out["sizes"].append({
            "source": [h, w], "resized": [params[0].nh, params[0].nw], "h2d_bytes": layout.pixel_bytes + 4 * layout.meta_words,
            "host_ms": stats(host), "device_events_ms": stats(dev_ev), "device_wall_ms": stats(dev_wall),
            "kernel_ms": stats(kern), "algorithmic_bytes": {"source": src_b, "outputs": out_b},
            "kernel_GBps_over_algorithmic_bytes": round((src_b + out_b) / (k * 1e6), 2),
            "host_over_device": round(statistics.median(host) / statistics.median(dev_wall), 2)})
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
