"""Training-step throughput of the MI355X path (not the headline metric).

One step = the reference Trainer's iteration (train_net.py:298-311 via detectron2 SimpleTrainer):
CATSeg training forward (fp32 CLIP with CLIP_FINETUNE "attention" by default -- --clip-finetune and
--prompt-length select the other modes and visual prompt tuning --, the aggregation head) -> BCE loss
-> backward through the HIP kernels -> AdamW with full-model clipping (train_net.py:228-253),
on the reference training config (configs/vitb_384.yaml: ViT-B/16 @384, COCO-Stuff's 171 classes,
POOLING [2,2], IMS_PER_BATCH 4, BASE_LR 2e-4, CLIP_GRADIENTS full_model 0.01), synthetic images and
labels, random-init weights.  --classes N takes the first N ade847 prompts; N > 256 (pad_len) runs the
per-image top-k class selection of model.py:691-725 (cat_seg.training).  --input host / device trains from a PNG
dataset written to a temporary directory (--source-size H W) through cat_seg.data.build_train_loader instead of
the synthetic tensors: the reference's mapper in the workers, or decode in the workers and the fused
augmentation kernel (MODEL.CATSEG_HIP.TRAIN_INPUT).  Prints one JSON line; --profile adds the per-kernel HIP-event times of one
step (ops.PROFILE).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT]

from cat_seg import add_cat_seg_config, build_model, get_cfg, ops  # noqa: E402
from cat_seg.arch import PRESETS  # noqa: E402
from cat_seg.optim import build_optimizer  # noqa: E402


def write_png_dataset(root, n, size, classes):
    """n random RGB PNGs of `size` with blocky label PNGs (8-bit up to 255 classes, else 16-bit; 255 = ignore)."""
    from PIL import Image
    from cat_seg.data import load_sem_seg
    h, w = size
    img_dir, gt_dir = os.path.join(root, "img"), os.path.join(root, "gt")
    os.makedirs(img_dir)
    os.makedirs(gt_dir)
    rng = np.random.default_rng(0)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(img_dir, f"{i:04d}.png"))
        lab = rng.integers(0, classes, (h // 32 + 1, w // 32 + 1)).repeat(32, 0).repeat(32, 1)[:h, :w]
        lab[lab == 255] = 254
        lab[:8] = 255
        Image.fromarray(lab.astype(np.uint8 if classes <= 255 else np.uint16)).save(os.path.join(gt_dir, f"{i:04d}.png"))
    return load_sem_seg(gt_dir, img_dir, gt_ext="png", image_ext="png")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip", default="ViT-B/16", choices=["ViT-B/16", "ViT-L/14@336px"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--classes", type=int, default=171)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clip-finetune", "--finetune", dest="finetune", default="attention",
                    choices=["attention", "prompt", "full", "none"],
                    help="MODEL.SEM_SEG_HEAD.CLIP_FINETUNE (cat_seg_model.py:57-75)")
    ap.add_argument("--prompt-length", type=int, default=0,
                    help="visual prompt tokens per vision block (PROMPT_LENGTH; PROMPT_DEPTH = the layer count)")
    ap.add_argument("--attention-type", default="linear", choices=["linear", "full"],
                    help="MODEL.SEM_SEG_HEAD.ATTENTION_TYPE of the class aggregation (model.py:331-334)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--image", type=int, default=384,
                    help="training crop (the reference's INPUT.CROP.SIZE (384, 384) for B/16 and L/14; the "
                         "CLIP encoder sees it resized to its resolution, cat_seg_model.py:136-146)")
    ap.add_argument("--input", default="synthetic", choices=["synthetic", "host", "device"],
                    help="where a step's batch comes from: the same synthetic tensors every step | build_train_loader "
                         "over a PNG dataset written to a temporary directory, augmented by the host mapper in the "
                         "workers (MODEL.CATSEG_HIP.TRAIN_INPUT host) | decoded in the workers and augmented by "
                         "catseg_train_augment (device)")
    ap.add_argument("--source-size", type=int, nargs=2, default=[512, 683], metavar=("H", "W"),
                    help="size of the PNG dataset's images (--input host / device)")
    ap.add_argument("--workers", type=int, default=4, help="loader workers (--input host / device)")
    ap.add_argument("--dataset-images", type=int, default=16, help="images in the PNG dataset")
    a = ap.parse_args()

    cfg = get_cfg()
    add_cat_seg_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "cat-seg_amd", "configs", "vitb_384.yaml"))
    cfg.merge_from_list(["MODEL.SEM_SEG_HEAD.CLIP_PRETRAINED", a.clip, "MODEL.SEM_SEG_HEAD.POOLING_SIZES", "[2,2]",
                         "MODEL.SEM_SEG_HEAD.CLIP_FINETUNE", a.finetune, "MODEL.CATSEG_HIP.DTYPE", "f32",
                         "MODEL.SEM_SEG_HEAD.ATTENTION_TYPE", a.attention_type,
                         "SOLVER.BASE_LR", "0.0002", "SOLVER.CLIP_GRADIENTS.ENABLED", "True",
                         "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model", "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", "0.01"])
    if a.clip != "ViT-B/16":
        cfg.merge_from_list(["MODEL.SEM_SEG_HEAD.TEXT_GUIDANCE_DIM", "768",
                             "MODEL.SEM_SEG_HEAD.APPEARANCE_GUIDANCE_DIM", "768"])
    if a.prompt_length > 0:
        layers = PRESETS[a.clip].vision_layers
        cfg.merge_from_list(["MODEL.SEM_SEG_HEAD.PROMPT_DEPTH", str(layers),
                             "MODEL.SEM_SEG_HEAD.PROMPT_LENGTH", str(a.prompt_length)])
    model = build_model(cfg).cuda().train()
    assert model.arch.prompt_depth in (0, model.arch.vision_layers)
    toks = np.load(os.path.join(ROOT, "tests", "golden", "class_tokens.npz"))["ade847"][:a.classes]
    model.sem_seg_head.predictor.set_class_tokens(torch.from_numpy(toks.astype(np.int64)))
    opt = build_optimizer(cfg, model)
    S = a.image
    gen = torch.Generator().manual_seed(0)
    batch = [{"image": torch.randint(0, 256, (3, S, S), generator=gen, dtype=torch.uint8),
              "sem_seg": torch.randint(0, a.classes, (S, S), generator=gen)} for _ in range(a.batch)]
    for b in batch:
        b["sem_seg"][:8] = 255
    batches, tmp = None, None
    if a.input != "synthetic":
        # the reference's training input (configs/config.yaml:49-60 at this crop) over PNGs of --source-size
        import tempfile
        from cat_seg.data import build_train_loader
        tmp = tempfile.TemporaryDirectory()
        cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", f"({S},)", "INPUT.CROP.ENABLED", "True", "INPUT.CROP.TYPE", "absolute",
                             "INPUT.CROP.SIZE", f"({S}, {S})", "INPUT.COLOR_AUG_SSD", "True",
                             "INPUT.SIZE_DIVISIBILITY", str(S), "MODEL.CATSEG_HIP.TRAIN_INPUT", a.input,
                             "SOLVER.IMS_PER_BATCH", str(a.batch)])
        dicts = write_png_dataset(tmp.name, a.dataset_images, a.source_size, a.classes)
        batches = iter(build_train_loader(dicts, cfg=cfg, num_workers=a.workers, seed=0))

    def step():
        opt.zero_grad(set_to_none=True)
        loss = model(next(batches) if batches is not None else batch)["loss_sem_seg"]
        loss.backward()
        opt.step()
        return loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    out = {"metric": "training images/sec (forward + backward + AdamW step)", "value": a.batch / dt,
           "unit": "images/sec", "ms_per_step": dt * 1e3, "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
           "dtype": "f32", "input": a.input,
           "data": ("synthetic images / labels" if a.input == "synthetic" else
                    f"{a.dataset_images} random PNGs of {a.source_size[0]} x {a.source_size[1]}, {a.workers} workers, "
                    f"augmentation on the {a.input}") + ", random-init weights",
           "loss": float(loss.detach()), "grad_norm": float(opt.last_grad_norm[0]),
           "peak_mem_gb": torch.cuda.max_memory_allocated() / 2 ** 30,
           "config": {"clip": a.clip, "resolution": S, "clip_resolution": model.clip_resolution[0], "classes": a.classes, "batch": a.batch, "pooling": [2, 2],
                      "clip_finetune": a.finetune, "prompt_length": a.prompt_length, "attention_type": a.attention_type, "optimizer": "AdamW (HIP) + full-model clip 0.01"}}
    if a.profile:
        ops.PROFILE = []
        step()
        torch.cuda.synchronize()
        fam, shp = {}, {}
        for r in ops.PROFILE:
            ms = r["start"].elapsed_time(r["end"])
            f = fam.setdefault(r["kernel"], [0.0, 0, 0.0])
            f[0] += ms
            f[1] += 1
            f[2] += r["flops"]
            if r.get("shape") is not None:
                g = shp.setdefault((r["kernel"],) + tuple(r["shape"]), [0.0, 0, 0.0])
                g[0] += ms
                g[1] += 1
                g[2] += r["flops"]
        ops.PROFILE = None
        # the GEMM launches by shape (M, N, K[, A / B contiguous dimension]): where the GEMM time goes
        out["gemm_shapes"] = [{"kernel": k[0], "shape": list(k[1:]), "ms": round(v[0], 3), "launches": v[1],
                               "tflops": round(v[2] / (v[0] * 1e9), 1) if v[0] > 0 else None}
                              for k, v in sorted(shp.items(), key=lambda kv: -kv[1][0])[:40]]
        tot = sum(v[0] for v in fam.values())
        out["kernels_ms"] = {k: {"ms": round(v[0], 3), "launches": v[1],
                                 "tflops": round(v[2] / (v[0] * 1e9), 1) if v[0] > 0 and v[2] else None}
                             for k, v in sorted(fam.items(), key=lambda kv: -kv[1][0])}
        out["kernels_total_ms"] = round(tot, 2)
    if tmp is not None:
        batches = None                  # the loader's workers end with its iterator
        tmp.cleanup()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
