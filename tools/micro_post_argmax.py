"""Time the label-map route against the probability route it replaces, warm, in one process, alternating, medians:

  new     catseg_postprocess_argmax      (+ one catseg_semseg_confusion_labels over the batch for the eval form)
  parent  catseg_postprocess / catseg_resize_bilinear into a preallocated (B, T, H, W) output, followed by
          catseg_semseg_confusion per image (eval) or out.argmax(1) (serving)

at the headline shape, two real eval shapes (batch 1, odd output width) and the sliding form.  Bytes are what
each route must move (logit crop read + outputs written, the parent's volume written and read back); GB/s is
bytes over the median time.  Checks the labels against the parent's argmax (equal where the parent runs
banded, W % 4 == 0; else the share of differing pixels is printed).
usage: python tools/micro_post_argmax.py [--json OUT.json] [--rounds 7] [--iters 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT]
import torch  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops  # noqa: E402

SHAPES = [  # name, B, T, h, w, crop, H, W, sigmoid
    ("headline 8x150 96^2 -> 336^2", 8, 150, 96, 96, None, 336, 336, True),
    ("eval 1x150 96^2 crop 96x72 -> 512x683", 1, 150, 96, 96, (96, 72), 512, 683, True),
    ("eval 1x847 96^2 -> 512x683", 1, 847, 96, 96, None, 512, 683, True),
    ("sliding 1x150 640^2 -> 480x640 (no sigmoid)", 1, 150, 640, 640, None, 480, 640, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    L.require_gpu()
    torch.manual_seed(0)
    results = []
    for name, B, T, h, w, crop, H, W, sig in SHAPES:
        ch, cw = crop or (h, w)
        lg = (3 * torch.randn(B, T, h, w, device="cuda")) if sig else torch.rand(B, T, h, w, device="cuda")
        vol = torch.empty(B, T, H, W, device="cuda")
        labels = torch.empty(B, H, W, dtype=torch.int32, device="cuda")
        score = torch.empty(B, H, W, device="cuda")
        gt = torch.randint(0, T, (B, H, W), device="cuda", dtype=torch.int32)
        conf = torch.zeros((T + 1) ** 2, dtype=torch.int64, device="cuda")
        bad = torch.zeros(1, dtype=torch.int64, device="cuda")
        parent_post = ops.postprocess if sig else ops.resize_bilinear

        def new():
            ops.postprocess_argmax(lg, labels, score, crop=crop, sigmoid=sig)

        def new_eval():             # the binning is per pixel: a batch of label maps is one (B*H, W) map
            new()
            ops.semseg_confusion_labels(labels.view(B * H, W), gt.view(B * H, W), conf, bad, num_classes=T)

        def parent():
            parent_post(lg, vol, crop=crop)

        def parent_eval():
            parent()
            for b in range(B):
                ops.semseg_confusion(vol[b], gt[b], conf, bad, num_classes=T)

        def parent_serving():
            parent()
            return vol.argmax(1)

        fns = [("new", new), ("parent_post", parent), ("new_eval", new_eval), ("parent_eval", parent_eval),
               ("parent_serving", parent_serving)]
        for _, f in fns:            # warm every route at this shape
            f()
        torch.cuda.synchronize()
        ts = {n: [] for n, _ in fns}
        for _ in range(a.rounds):   # alternating
            for n, f in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    f()
                e1.record()
                torch.cuda.synchronize()
                ts[n].append(e0.elapsed_time(e1) / a.iters * 1e3)
        med = {n: sorted(v)[len(v) // 2] for n, v in ts.items()}
        src = 4 * B * T * ch * cw
        byt = {"new": src + 8 * B * H * W,
               "parent_post": src + 4 * B * T * H * W,
               "new_eval": src + 8 * B * H * W + 8 * B * H * W,
               "parent_eval": src + 8 * B * T * H * W + 4 * B * H * W,
               "parent_serving": src + 8 * B * T * H * W + 8 * B * H * W}
        new()
        ref = parent_serving()
        differ = (ref != labels.long()).float().mean().item()
        if W % 4 == 0 and differ and "sliding" not in name:
            raise SystemExit(f"{name}: labels differ from the banded parent at {differ:.2e} of the pixels")
        r = {"shape": name, "B": B, "T": T, "hw": [h, w], "crop": [ch, cw], "HW": [H, W], "sigmoid": sig,
             "us": {n: round(med[n], 2) for n in med}, "us_min": {n: round(min(ts[n]), 2) for n in ts},
             "bytes": byt, "GBps": {n: round(byt[n] / med[n] / 1e3, 1) for n in med},
             "bytes_saved_vs_parent_post": round(1 - byt["new"] / byt["parent_post"], 4),
             "ratio_new_over_parent_post": round(med["new"] / med["parent_post"], 3),
             "ratio_new_eval_over_parent_post": round(med["new_eval"] / med["parent_post"], 3),
             "labels_differ_share": differ}
        results.append(r)
        print(f"{name}\n   " + "  ".join(f"{n} {med[n]:.1f} us ({r['GBps'][n]:.0f} GB/s)" for n in med) +
              f"\n   new / parent_post {r['ratio_new_over_parent_post']:.3f}, new_eval / parent_post "
              f"{r['ratio_new_eval_over_parent_post']:.3f}, bytes saved {100 * r['bytes_saved_vs_parent_post']:.1f} %, "
              f"labels differ at {differ:.2e}", flush=True)
        del vol
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/micro_post_argmax.py", "rounds": a.rounds, "iters": a.iters, "median_of": "rounds",
                       "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
