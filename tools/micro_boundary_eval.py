"""Time the boundary counters of one prediction / ground-truth pair on the device against the host composition they
replace, warm, in one process, legs alternating, copies included:

  host_boundary    both maps copied to the host, then the published per-class method: per present label and per
                   width w, scipy.ndimage.binary_erosion (3 x 3 ones, iterations=w, border_value=0) of the
                   ground-truth mask and of the predicted mask, mask minus erosion as the band, and the counts
                   (inter, gt_band, pred_band per class, band_conf from the union of the ground-truth bands).  scipy
                   stands in for OpenCV's erode, which the published code calls and which is not a dependency here
  device_boundary  ops.boundary_confusion (two distance maps + the counters) and the copy of the counters to the host
  distance_pred / distance_gt / counters   the device parts alone, timed with events; the distance pass also as
                   GB/s against its bytes: the map read by both passes (8 B per pixel), the int16 row distances
                   written and read back (4 B) and the int16 result (2 B)
  distance_uniform the distance pass on a uniform map of the same size with the same cap: its worst case, every
                   column scan away from the border runs to the cap

for the two maps of the neighbouring tools (tools/micro_label_regions.py): smooth blobs + 2 % speckle as the
prediction and its sieved map (ops.sieve_labels, min_area 16) as the ground truth, 512 x 683 with 12 labels and
2048 x 3072 with 30 labels; widths 0.02 x the image diagonal and 3 px.  Seeded, reads no file.  The device leg is
wall-clocked around a synchronize, enough repetitions to fill --fill seconds (at least one), --rounds times,
alternating with the host leg (once per round), so the run-to-run spread is visible.  The two paths' counters are
compared for equality.  Not measured: a full evaluation loop, and OpenCV as the baseline.
usage: python tools/micro_boundary_eval.py [--json profiles/boundary/micro.json] [--rounds 3] [--fill 0.3]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops  # noqa: E402
from micro_label_regions import MIN_AREA, SHAPES, blobs  # noqa: E402

ONES = np.ones((3, 3), bool)


def host_counters(P, G, widths, N):
    """The flat counters of catseg_boundary_confusion by per-class erosion (no ignore label, no fold)."""
    n1 = N + 1
    per = n1 * n1 + 3 * N
    out = np.zeros(len(widths) * per, np.int64)
    pair = n1 * P.astype(np.int64) + G
    labels = np.union1d(np.unique(P), np.unique(G))
    for k, w in enumerate(widths):
        c = out[k * per:(k + 1) * per]
        gband = np.zeros(G.shape, bool)
        for v in labels:
            mg, mp = G == v, P == v
            bg = mg & ~ndimage.binary_erosion(mg, ONES, iterations=w, border_value=0)
            bp = mp & ~ndimage.binary_erosion(mp, ONES, iterations=w, border_value=0)
            gband |= bg
            c[n1 * n1 + v] = (bg & bp).sum()
            c[n1 * n1 + N + v] = bg.sum()
            c[n1 * n1 + 2 * N + v] = bp.sum()
        c[:n1 * n1] = np.bincount(pair[gband], minlength=n1 * n1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fill", type=float, default=0.3)
    a = ap.parse_args()
    L.require_gpu()
    out = {"tool": "tools/micro_boundary_eval.py", "rounds": a.rounds, "shapes": []}
    for H, W, n_labels in SHAPES:
        pred = blobs(H, W, n_labels, seed=H).cuda()
        gt = ops.sieve_labels(pred, MIN_AREA)
        widths = [max(1, int(round(0.02 * math.sqrt(H * H + W * W)))), 3]
        K, cap = len(widths), max(widths) + 1
        total = K * ((n_labels + 1) ** 2 + 3 * n_labels)
        counters = torch.zeros(total, dtype=torch.int64, device="cuda")

        def f_host():
            return host_counters(pred.cpu().numpy(), gt.cpu().numpy(), widths, n_labels)

        def f_device():
            counters.zero_()
            ops.boundary_confusion(pred, gt, widths, counters, num_classes=n_labels)
            return counters.cpu()

        d_pred, d_gt = ops.boundary_distance(pred, cap), ops.boundary_distance(gt, cap)
        uniform = torch.zeros_like(pred)            # the distance pass's worst case: every column scan runs to the cap
        d_uni = ops.boundary_distance(uniform, cap)
        warr = (C.c_int * K)(*widths)

        def f_counters():
            L.call("catseg_boundary_confusion", pred.data_ptr(), gt.data_ptr(), d_pred.data_ptr(), d_gt.data_ptr(), H,
                   W, n_labels, 255, -1, warr, K, counters.data_ptr(), torch.cuda.current_stream().cuda_stream)

        def wall(f):
            def run(iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    f()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / iters * 1e3        # ms per call
            return run

        def events(f):
            def run(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    f()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / iters
            return run

        got = f_device().numpy()
        t0 = time.perf_counter()
        equal = bool(np.array_equal(f_host(), got))                       # also the host leg's first run
        first_host = (time.perf_counter() - t0) * 1e3
        legs = [("device_boundary", wall(f_device)),
                ("distance_pred", events(lambda: ops.boundary_distance(pred, cap, out=d_pred))),
                ("distance_gt", events(lambda: ops.boundary_distance(gt, cap, out=d_gt))),
                ("distance_uniform", events(lambda: ops.boundary_distance(uniform, cap, out=d_uni))),
                ("counters", events(f_counters))]
        iters = {k: max(1, int(a.fill * 1e3 / f(1))) for k, f in legs}     # warm, size the repetitions
        ts = {k: [] for k, _ in legs}
        ts["host_boundary"] = [first_host]
        for r in range(a.rounds):                                          # alternating
            for k, f in legs:
                ts[k].append(f(iters[k]))
            if r + 1 < a.rounds:
                ts["host_boundary"].append(wall(f_host)(1))
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        dist_bytes = 14 * H * W
        rec = {"HW": [H, W], "labels": n_labels, "widths": widths, "cap": cap, "counters": total,
               "counters_equal_to_host": equal, "in_band_pixels": [int(x) for x in got.reshape(K, -1)[:, :(n_labels + 1) ** 2].sum(1)],
               "iters": iters, "ms": {k: [round(v, 4) for v in ts[k]] for k in ts},
               "ms_median": {k: round(med[k], 4) for k in med},
               "distance_bytes": dist_bytes,
               "distance_GBps": {k: round(dist_bytes / (med[k] * 1e-3) / 1e9, 1) for k in ("distance_pred", "distance_gt", "distance_uniform")},
               "mean_distance": {"pred": round(float(d_pred.float().mean()), 2), "gt": round(float(d_gt.float().mean()), 2),
                                 "uniform": round(float(d_uni.float().mean()), 2)},
               "speedup": round(med["host_boundary"] / med["device_boundary"], 1),
               # the gap must exceed the spread of the runs of this same call
               "device_faster_beyond_spread": bool(max(ts["device_boundary"]) < min(ts["host_boundary"])),
               "host_faster_beyond_spread": bool(max(ts["host_boundary"]) < min(ts["device_boundary"]))}
        out["shapes"].append(rec)
        for k in ts:
            print(f"{H} x {W}  {k:16s} median {med[k]:11.4f} ms  (min {min(ts[k]):.4f}, max {max(ts[k]):.4f})", flush=True)
        print(f"{H} x {W}  widths {widths}; counters equal {equal}; host / device {rec['speedup']}x; "
              f"distance {rec['distance_GBps']} GB/s", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
