"""Time catseg_postprocess_topk (K = 2 and K = 4, with the mass) against (a) catseg_postprocess_argmax at the
same shape, which is what the extra ranks cost, and (b) the composition it replaces: catseg_postprocess into a
(B, T, H, W) volume, then torch.topk(K, dim=1) and sum(1) on the device.  One process, warm, the legs alternating
over the rounds; median and range per leg.  Bytes are what a route must move (the logit crop read + the maps
written; the composition writes the volume and reads it back twice); GB/s is bytes over the median time.  "live" is
what a route holds in device memory besides the logits: its outputs, and for the composition the volume too.
Checks the fused maps against the composition's (equal where catseg_postprocess runs banded, W % 4 == 0).
usage: python tools/micro_post_topk.py [--json OUT.json] [--rounds 3] [--iters 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT]
import torch  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops  # noqa: E402

SHAPES = [  # name, B, T, h, w, H, W
    ("headline 8x150 96^2 -> 336^2", 8, 150, 96, 96, 336, 336),
    ("scene 1x150 96^2 -> 2048x3072", 1, 150, 96, 96, 2048, 3072),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    L.require_gpu()
    torch.manual_seed(0)
    results = []
    for name, B, T, h, w, H, W in SHAPES:
        lg = 3 * torch.randn(B, T, h, w, device="cuda")
        vol = torch.empty(B, T, H, W, device="cuda")
        labels = torch.empty(B, H, W, dtype=torch.int32, device="cuda")
        score = torch.empty(B, H, W, device="cuda")

        def argmax():
            ops.postprocess_argmax(lg, labels, score)

        def fused(K):
            return lambda: ops.postprocess_topk(lg, K, out_hw=(H, W))

        def composed(K):
            def run():
                ops.postprocess(lg, vol)
                top = torch.topk(vol, K, dim=1)
                return top.values, top.indices, vol.sum(1)
            return run

        fns = [("argmax", argmax)]
        for K in (2, 4):
            fns += [(f"topk{K}", fused(K)), (f"composed{K}", composed(K))]
        for _, f in fns:            # warm every leg at this shape
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
        src, px = 4 * B * T * h * w, 4 * B * H * W
        byt, live = {"argmax": src + 2 * px}, {"argmax": 2 * px}
        for K in (2, 4):
            byt[f"topk{K}"] = src + (2 * K + 1) * px
            live[f"topk{K}"] = (2 * K + 1) * px
            # the volume written, read by topk and by sum; torch.topk returns int64 indices
            byt[f"composed{K}"] = src + 3 * T * px + (3 * K + 1) * px
            live[f"composed{K}"] = T * px + (3 * K + 1) * px
        checks = {}
        for K in (2, 4):
            got = fused(K)()
            vals, idx, mass = composed(K)()
            checks[f"K{K}"] = {
                "labels_differ_share": (idx != got["topk_labels"].long()).float().mean().item(),
                "max_abs_score_diff": (vals - got["topk_score"]).abs().max().item(),
                "max_rel_mass_diff": ((mass - got["mass"]).abs() / mass).max().item()}
            if W % 4 == 0 and checks[f"K{K}"]["max_abs_score_diff"]:
                raise SystemExit(f"{name}: K = {K} scores differ from the sort of the banded volume")
            del got, vals, idx, mass
        r = {"shape": name, "B": B, "T": T, "hw": [h, w], "HW": [H, W],
             "us": {n: round(med[n], 2) for n in med},
             "us_range": {n: [round(min(ts[n]), 2), round(max(ts[n]), 2)] for n in ts},
             "bytes": byt, "live_bytes": live, "GBps": {n: round(byt[n] / med[n] / 1e3, 1) for n in med},
             "ratio_topk_over_argmax": {f"K{K}": round(med[f"topk{K}"] / med["argmax"], 3) for K in (2, 4)},
             "ratio_topk_over_composed": {f"K{K}": round(med[f"topk{K}"] / med[f"composed{K}"], 4) for K in (2, 4)},
             "fused_wins_beyond_the_spread": {f"K{K}": max(ts[f"topk{K}"]) < min(ts[f"composed{K}"]) for K in (2, 4)},
             "checks": checks}
        results.append(r)
        print(f"{name}\n   " + "  ".join(f"{n} {med[n]:.1f} us [{min(ts[n]):.1f}, {max(ts[n]):.1f}] "
                                        f"({r['GBps'][n]:.0f} GB/s)" for n in med) +
              f"\n   topk / argmax {r['ratio_topk_over_argmax']}, topk / composed {r['ratio_topk_over_composed']}, "
              f"checks {checks}", flush=True)
        del vol
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/micro_post_topk.py", "rounds": a.rounds, "iters": a.iters, "median_of": "rounds",
                       "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
