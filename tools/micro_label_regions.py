"""Time the connected regions + table (and the sieve) of one label map made on the device against the host
composition they replace, warm, in one process, legs alternating, copies included:

  host_regions     the map and its score copied to the host, scipy.ndimage.label once per present label,
                   find_objects for the boxes, bincounts for areas and score sums
  device_regions   ops.label_regions with score (labelling + scan, the 4-byte read of R, the write pass) and the
                   copy of the table to the host; the region ids stay on the device, where the next step reads them
  host_sieve       the copy, the restated sieve (tests/regions_ref.py sieve), then host_regions on its result
  device_sieve     ops.sieve_labels + ops.label_regions + the copy of the table
  count / write / sieve   the device parts alone (ops.label_regions_count, ops.label_regions_write into a preallocated
                   table, ops.sieve_labels), timed with events

for smooth blob maps with 2 % single-pixel speckle of 512 x 683 with 12 labels and 2048 x 3072 with 30 labels (the
shapes of tools/micro_label_runs.py).  Seeded, reads no file.  The host and device legs are wall-clocked around a
synchronize, enough repetitions to fill --fill seconds (at least one), --rounds times, alternating, so the run-to-run
spread is visible.  The bytes of `count` are the algorithmic ones of the labelling: the map read, parent written and
read again (12 bytes per pixel).
usage: python tools/micro_label_regions.py [--json profiles/regions/micro.json] [--rounds 5] [--fill 0.3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402
import regions_ref  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops  # noqa: E402

SHAPES = [(512, 683, 12), (2048, 3072, 30)]
CELL = 48
MIN_AREA = 16
STRUCT8 = ndimage.generate_binary_structure(2, 2)


def blobs(H, W, n_labels, seed, speckle=0.02):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, n_labels, (H // CELL + 2, W // CELL + 2), generator=g)
    yy = torch.arange(H)[:, None] + (8 * torch.sin(torch.arange(W) / 17.0))[None, :]
    xx = torch.arange(W)[None, :] + (8 * torch.cos(torch.arange(H) / 13.0))[:, None]
    m = coarse[(yy / CELL).long().clamp(0), (xx / CELL).long().clamp(0)].to(torch.int32)
    sp = torch.rand(H, W, generator=g) < speckle
    m[sp] = torch.randint(0, n_labels, (int(sp.sum()),), generator=g).to(torch.int32)
    return m


def host_regions(m, score):
    """scipy per present label: (number of regions, areas, boxes, score sums), in scipy's per-label order"""
    q = np.rint(score * np.float32(65536.0)).astype(np.int64).ravel()
    areas, boxes, sums = [], [], []
    for v in np.unique(m):
        lab, k = ndimage.label(m == v, structure=STRUCT8)
        boxes += ndimage.find_objects(lab)
        flat = lab.ravel()
        areas.append(np.bincount(flat, minlength=k + 1)[1:])
        sums.append(np.bincount(flat, weights=q, minlength=k + 1)[1:])
    return sum(len(a) for a in areas), np.concatenate(areas), boxes, np.concatenate(sums)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fill", type=float, default=0.3)
    a = ap.parse_args()
    L.require_gpu()
    out = {"tool": "tools/micro_label_regions.py", "rounds": a.rounds, "cell": CELL, "min_area": MIN_AREA,
           "connectivity": 8, "shapes": []}
    for H, W, n_labels in SHAPES:
        labels = blobs(H, W, n_labels, seed=H).cuda()
        score = torch.rand(H, W, generator=torch.Generator().manual_seed(1)).cuda()

        def to_host(table):
            return {k: v.cpu() for k, v in table.items()}

        def f_host_regions():
            return host_regions(labels.cpu().numpy(), score.cpu().numpy())

        def f_device_regions():
            ids, table = ops.label_regions(labels, score=score)
            return ids, to_host(table)

        def f_host_sieve():
            m = regions_ref.sieve(labels.cpu().numpy(), MIN_AREA, 8)
            return m, host_regions(m, score.cpu().numpy())

        def f_device_sieve():
            m = ops.sieve_labels(labels, MIN_AREA)
            ids, table = ops.label_regions(m, score=score)
            return m, to_host(table)

        def wall(f):
            def run(iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    f()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / iters * 1e6        # us per call
            return run

        def events(f):
            def run(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    f()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / iters * 1e3
            return run

        # equality of the two paths, against the full restatement
        ids, table = f_device_regions()
        exp_ids, exp = regions_ref.regions(labels.cpu().numpy(), 8, -1, score.cpu().numpy())
        same = bool(np.array_equal(ids.cpu().numpy(), exp_ids) and
                    all(np.array_equal(table[k].numpy(), exp[k]) for k in exp))
        n_host, areas, _, sums = f_host_regions()
        R = int(table["area"].numel())
        same = same and n_host == R and sorted(areas.tolist()) == sorted(exp["area"].tolist()) and \
            int(sums.sum()) == int(exp["score_q16"].sum())
        sieved, stable = f_device_sieve()
        same_sieve = bool(np.array_equal(sieved.cpu().numpy(), regions_ref.sieve(labels.cpu().numpy(), MIN_AREA, 8)))
        R_sieved = int(stable["area"].numel())

        ws = ops.label_regions_count(labels)
        pre = {"label": torch.empty(R, dtype=torch.int32, device="cuda"), "area": torch.empty(R, dtype=torch.int32, device="cuda"),
               "bbox": torch.empty(R, 4, dtype=torch.int32, device="cuda"), "first": torch.empty(R, dtype=torch.int32, device="cuda"),
               "score_q16": torch.empty(R, dtype=torch.int64, device="cuda")}
        pre_ids, pre_out = torch.empty_like(labels), torch.empty_like(labels)
        legs = [("host_regions", wall(f_host_regions)), ("device_regions", wall(f_device_regions)),
                ("host_sieve", wall(f_host_sieve)), ("device_sieve", wall(f_device_sieve)),
                ("count", events(lambda: ops.label_regions_count(labels))),
                ("write", events(lambda: ops.label_regions_write(labels, ws, pre_ids, pre, score=score))),
                ("sieve", events(lambda: ops.sieve_labels(labels, MIN_AREA, out=pre_out)))]
        iters = {k: max(1, int(a.fill * 1e6 / f(1))) for k, f in legs}               # warm, size the repetitions
        ts = {k: [] for k, _ in legs}
        for _ in range(a.rounds):                                                     # alternating
            for k, f in legs:
                ts[k].append(f(iters[k]))
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        nbytes = 12 * H * W
        rec = {"HW": [H, W], "labels": n_labels, "regions": R, "regions_after_sieve": R_sieved,
               "equal_to_restatement": same, "sieve_equal_to_restatement": same_sieve, "iters": iters,
               "us": {k: [round(v, 1) for v in ts[k]] for k in ts},
               "us_median": {k: round(med[k], 1) for k in med},
               "count_bytes": nbytes, "count_GBps": round(nbytes / med["count"] / 1e3, 1),
               "speedup_regions": round(med["host_regions"] / med["device_regions"], 2),
               "speedup_sieve": round(med["host_sieve"] / med["device_sieve"], 2),
               # the gap must exceed the spread of the runs of this same call
               "regions_faster_beyond_spread": bool(max(ts["device_regions"]) < min(ts["host_regions"])),
               "sieve_faster_beyond_spread": bool(max(ts["device_sieve"]) < min(ts["host_sieve"]))}
        out["shapes"].append(rec)
        for k in ts:
            print(f"{H} x {W}  {k:15s} median {med[k]:11.1f} us  (min {min(ts[k]):.1f}, max {max(ts[k]):.1f}, "
                  f"{iters[k]} calls x {a.rounds})", flush=True)
        print(f"{H} x {W}  {R} regions ({R_sieved} after the sieve); host / device: regions {rec['speedup_regions']}x, "
              f"sieve + regions {rec['speedup_sieve']}x; equal: {same}, {same_sieve}; labelling + scan "
              f"{rec['count_GBps']} GB/s of {nbytes / 1e6:.2f} MB", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
