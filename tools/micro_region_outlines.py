"""Time the outlines of the regions of one label map made on the device against the host composition they replace,
warm, in one process, legs alternating, copies included:

  host_outlines    the region ids copied to the host (a file for the tracer: the write is timed apart and left out)
                   plus the sequential tracer of tools/region_outlines_host.cpp built at -O2, its own wall clock
                   per trace; the fairest host stand-in there is without gdal / rasterio
  device_outlines  ops.region_outlines (count + scan, the 4-byte read of K, link + ranking + scans, the 4-byte read
                   of NR, the write pass) and the copy of the rings to the host
  count / rank / write   the device parts alone into preallocated buffers, timed with events over many calls, and
                   once each with their bytes (the wrappers' ops.PROFILE records: "parts"); the kernels inside
                   them are listed by a kernel trace of one call, profiles/outlines/kernels.txt

for the region ids (ops.label_regions, connectivity 8) of smooth blob maps with 2 % single-pixel speckle of 512 x 683
with 12 labels and 2048 x 3072 with 30 labels (the maps of tools/micro_label_regions.py).  Seeded, reads no file but
the one it writes for the tracer.  The device legs are wall-clocked around a synchronize, enough repetitions to fill
--fill seconds (at least one), --rounds times, alternating with the host leg, so the run-to-run spread is visible.
usage: python tools/micro_region_outlines.py [--json profiles/outlines/micro.json] [--rounds 5] [--fill 0.3]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cat-seg_amd"), ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops  # noqa: E402
from micro_label_regions import SHAPES, blobs  # noqa: E402


def build_tracer(tmp):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        raise SystemExit("micro_region_outlines: no host C++ compiler for the baseline")
    exe = os.path.join(tmp, "region_outlines_host")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "cat-seg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "region_outlines_host.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fill", type=float, default=0.3)
    a = ap.parse_args()
    L.require_gpu()
    tmp = tempfile.mkdtemp(prefix="outlines_")
    exe = build_tracer(tmp)
    out = {"tool": "tools/micro_region_outlines.py", "rounds": a.rounds, "connectivity": 8, "shapes": []}
    for H, W, n_labels in SHAPES:
        labels = blobs(H, W, n_labels, seed=H).cuda()
        ids, _ = ops.label_regions(labels)
        path = os.path.join(tmp, f"ids_{H}x{W}.i32")

        def f_copy():
            return ids.cpu().numpy()

        def host_trace(reps):
            r = subprocess.run([exe, "--trace", path, str(H), str(W), "8", str(reps)], check=True,
                               capture_output=True, text=True)
            return json.loads(r.stdout)

        def f_device():
            return {k: v.cpu() for k, v in ops.region_outlines(ids).items()}

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

        f_copy().tofile(path)
        got = f_device()
        K, NR = int(got["vertices"].shape[0]), int(got["ring_value"].numel())
        first = host_trace(1)
        # the two paths agree on the counts here; tests/test_gpu_region_outlines.py holds every vertex to the restatement
        same_counts = first["K"] == K and first["NR"] == NR
        area = np.zeros(int(ids.max().item()) + 1, np.int64)
        np.add.at(area, got["ring_value"].numpy(), got["ring_area2"].numpy())
        same_area = bool(np.array_equal(area, 2 * np.bincount(f_copy().ravel(), minlength=len(area))))

        ws = ops.region_outlines_count(ids)
        rws = ops.region_outlines_rank(ids, ws, K)
        pre = {"ring_offset": torch.empty(NR + 1, dtype=torch.int32, device="cuda"),
               "ring_value": torch.empty(NR, dtype=torch.int32, device="cuda"),
               "ring_area2": torch.empty(NR, dtype=torch.int64, device="cuda"),
               "vertices": torch.empty(K, 2, dtype=torch.int32, device="cuda")}
        legs = [("copy_to_host", wall(f_copy)), ("device_outlines", wall(f_device)),
                ("count", events(lambda: ops.region_outlines_count(ids))),
                ("rank", events(lambda: ops.region_outlines_rank(ids, ws, K))),
                ("write", events(lambda: ops.region_outlines_write(ids, rws, K, pre)))]
        iters = {k: max(1, int(a.fill * 1e6 / f(1))) for k, f in legs}               # warm, size the repetitions
        ts = {k: [] for k, _ in legs}
        ts["host_trace"] = []
        for _ in range(a.rounds):                                                     # alternating
            for k, f in legs:
                ts[k].append(f(iters[k]))
            ts["host_trace"].append(host_trace(1)["ms"][0] * 1e3)
        ts["host_outlines"] = [c + t for c, t in zip(ts["copy_to_host"], ts["host_trace"])]
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}

        # every launch of one pass alone: the wrappers' own records
        ops.PROFILE = []
        ws2 = ops.region_outlines_count(ids)
        rws2 = ops.region_outlines_rank(ids, ws2, K)
        ops.region_outlines_write(ids, rws2, K, pre)
        torch.cuda.synchronize()
        parts = {r["kernel"]: {"us": round(r["start"].elapsed_time(r["end"]) * 1e3, 1), "bytes": r["bytes"]}
                 for r in ops.PROFILE}
        ops.PROFILE = None

        rec = {"HW": [H, W], "labels": n_labels, "regions": int(ids.max().item()) + 1, "K": K, "NR": NR,
               "jump_rounds": int(np.ceil(np.log2(max(K, 1)))),
               "counts_equal_to_host_tracer": same_counts, "areas_equal_to_pixel_counts": same_area, "iters": iters,
               "workspace_bytes": {"map": ws.numel() * 4, "ring": rws.numel() * 4},
               "result_bytes": 8 * K + 16 * NR + 4,
               "us": {k: [round(v, 1) for v in ts[k]] for k in ts},
               "us_median": {k: round(med[k], 1) for k in med}, "parts": parts,
               "speedup": round(med["host_outlines"] / med["device_outlines"], 2),
               # the gap must exceed the spread of the runs of this same call
               "device_faster_beyond_spread": bool(max(ts["device_outlines"]) < min(ts["host_outlines"])),
               "host_faster_beyond_spread": bool(max(ts["host_outlines"]) < min(ts["device_outlines"]))}
        out["shapes"].append(rec)
        for k in ts:
            print(f"{H} x {W}  {k:16s} median {med[k]:11.1f} us  (min {min(ts[k]):.1f}, max {max(ts[k]):.1f})", flush=True)
        print(f"{H} x {W}  K {K} corners, NR {NR} rings, {rec['regions']} regions; host / device {rec['speedup']}x; "
              f"counts equal {same_counts}, areas equal {same_area}; parts {parts}", flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
