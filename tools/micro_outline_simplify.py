"""Time the simplification of the outlines of one region map on the device against the host composition it replaces,
warm, in one process, legs alternating, copies included:

  host_simplify    the region ids and the rings copied to the host (a file for the tool: the write is timed apart
                   and left out) plus the sequential pipeline of tools/outline_simplify_host.cpp built at -O2 (the
                   logic header run by one thread: junction bitmaps, nodes, arcs, Douglas-Peucker, compaction), its
                   own wall clock per run
  device_simplify  ops.simplify_outlines (junctions + count + scan, the 4-byte read of N, nodes + arcs + Douglas-
                   Peucker + scan, the 4-byte read of K', the write pass) and the copy of the simplified rings to
                   the host
  count / run / write   the device parts alone into preallocated buffers, timed with events over many calls, and
                   once each with their bytes (the wrappers' ops.PROFILE records: "parts")

for the region ids (ops.label_regions, connectivity 8) and outlines (ops.region_outlines) of the two maps of
tools/micro_region_outlines.py: 512 x 683 with 12 labels and 2048 x 3072 with 30 labels, at tolerance 1.0.  Reports
K -> K', N, and the histogram of arc lengths (arcs of at least 2 edges by the highest set bit of their length), which
decides where a workgroup takes over from a wave.  Seeded, reads no file but the one it writes for the tool.  The
device legs are wall-clocked around a synchronize, enough repetitions to fill --fill seconds (at least one), --rounds
times, alternating with the host leg, so the run-to-run spread is visible.
usage: python tools/micro_outline_simplify.py [--json profiles/simplify/micro.json] [--rounds 5] [--fill 0.3]"""
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

TOLERANCE = 1.0


def build_tool(tmp):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        raise SystemExit("micro_outline_simplify: no host C++ compiler for the baseline")
    exe = os.path.join(tmp, "outline_simplify_host")
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "cat-seg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "outline_simplify_host.cpp"), "-o", exe], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fill", type=float, default=0.3)
    a = ap.parse_args()
    L.require_gpu()
    tmp = tempfile.mkdtemp(prefix="simplify_")
    exe = build_tool(tmp)
    out = {"tool": "tools/micro_outline_simplify.py", "rounds": a.rounds, "connectivity": 8, "tolerance": TOLERANCE,
           "shapes": []}
    for H, W, n_labels in SHAPES:
        labels = blobs(H, W, n_labels, seed=H).cuda()
        ids, _ = ops.label_regions(labels)
        outl = ops.region_outlines(ids)
        K, NR = int(outl["vertices"].shape[0]), int(outl["ring_value"].numel())
        path = os.path.join(tmp, f"rings_{H}x{W}.i32")

        def f_copy():
            return ids.cpu().numpy(), outl["ring_offset"].cpu().numpy(), outl["vertices"].cpu().numpy()

        def host_tool(reps):
            r = subprocess.run([exe, "--simplify", path, str(H), str(W), str(NR), str(K), str(TOLERANCE), str(reps)],
                               check=True, capture_output=True, text=True)
            return json.loads(r.stdout)

        def f_device():
            return {k: v.cpu() for k, v in ops.simplify_outlines(ids, outl, TOLERANCE).items()}

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

        with open(path, "wb") as f:
            for part in f_copy():
                f.write(np.ascontiguousarray(part, np.int32).tobytes())
        got = f_device()
        K2 = int(got["vertices"].shape[0])
        first = host_tool(1)
        ws = ops.simplify_outlines_count(ids, outl)
        N = int(ws[0].item())
        # the two paths agree on the counts here; tests/test_gpu_outline_simplify.py holds every vertex to the restatement
        same_counts = first["N"] == N and first["K2"] == K2

        nws = ops.simplify_outlines_run(ids, outl, ws, N, TOLERANCE)
        pre = {"ring_offset": torch.empty(NR + 1, dtype=torch.int32, device="cuda"),
               "ring_value": torch.empty(NR, dtype=torch.int32, device="cuda"),
               "ring_area2": torch.empty(NR, dtype=torch.int64, device="cuda"),
               "ring_hole": torch.empty(NR, dtype=torch.uint8, device="cuda"),
               "vertices": torch.empty(K2, 2, dtype=torch.int32, device="cuda")}
        legs = [("copy_to_host", wall(f_copy)), ("device_simplify", wall(f_device)),
                ("count", events(lambda: ops.simplify_outlines_count(ids, outl))),
                ("run", events(lambda: ops.simplify_outlines_run(ids, outl, ws, N, TOLERANCE))),
                ("write", events(lambda: ops.simplify_outlines_write(ids, outl, nws, N, pre)))]
        iters = {k: max(1, int(a.fill * 1e6 / f(1))) for k, f in legs}               # warm, size the repetitions
        ts = {k: [] for k, _ in legs}
        ts["host_tool"] = []
        for _ in range(a.rounds):                                                     # alternating
            for k, f in legs:
                ts[k].append(f(iters[k]))
            ts["host_tool"].append(host_tool(1)["ms"][0] * 1e3)
        ts["host_simplify"] = [c + t for c, t in zip(ts["copy_to_host"], ts["host_tool"])]
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}

        # every part alone, once: the wrappers' own records
        ops.PROFILE = []
        ws2 = ops.simplify_outlines_count(ids, outl)
        nws2 = ops.simplify_outlines_run(ids, outl, ws2, N, TOLERANCE)
        ops.simplify_outlines_write(ids, outl, nws2, N, pre)
        torch.cuda.synchronize()
        parts = {r["kernel"]: {"us": round(r["start"].elapsed_time(r["end"]) * 1e3, 1), "bytes": r["bytes"]}
                 for r in ops.PROFILE}
        ops.PROFILE = None

        hist = {f"{1 << b}..{(2 << b) - 1}": n for b, n in enumerate(first["hist"]) if n}
        rec = {"HW": [H, W], "labels": n_labels, "regions": int(ids.max().item()) + 1, "NR": NR, "K": K, "N": N,
               "K2": K2, "arcs_of_2_or_more_edges": first["arcs"], "arc_length_histogram": hist,
               "arcs_at_or_above_workgroup_threshold": sum(n for b, n in enumerate(first["hist"]) if (1 << b) >= 512),
               "counts_equal_to_host_tool": same_counts, "iters": iters,
               "workspace_bytes": {"map": ws.numel() * 4, "node": nws.numel() * 4},
               "result_bytes": 8 * K2 + 17 * NR + 4,
               "us": {k: [round(v, 1) for v in ts[k]] for k in ts},
               "us_median": {k: round(med[k], 1) for k in med}, "parts": parts,
               "speedup": round(med["host_simplify"] / med["device_simplify"], 2),
               # the gap must exceed the spread of the runs of this same call
               "device_faster_beyond_spread": bool(max(ts["device_simplify"]) < min(ts["host_simplify"])),
               "host_faster_beyond_spread": bool(max(ts["host_simplify"]) < min(ts["device_simplify"]))}
        out["shapes"].append(rec)
        for k in ts:
            print(f"{H} x {W}  {k:16s} median {med[k]:11.1f} us  (min {min(ts[k]):.1f}, max {max(ts[k]):.1f})", flush=True)
        print(f"{H} x {W}  K {K} -> N {N} -> K' {K2}, NR {NR} rings; arcs {first['arcs']}, lengths {hist}; "
              f"host / device {rec['speedup']}x; counts equal {same_counts}; parts {parts}", flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
