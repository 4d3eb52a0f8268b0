"""Evaluation harness: detectron2's `DatasetEvaluator` surface for semantic segmentation
(SURVEY §8f rank 3), with the per-image confusion-matrix update on the device.

Mirrors the evaluators the reference registers (train_net.py:89-149):
  * `SemSegEvaluator`       — detectron2 v0.6 `SemSegEvaluator` (the copy the reference keeps
                              as `SemSegGzeroEvaluator`, plain_train_net.py:48-200, without
                              the seen/unseen split);
  * `SemSegGzeroEvaluator`  — + seen / unseen IoU and their harmonic mean over
                              `val_extra_classes` (plain_train_net.py:170-197);
  * `VOCbEvaluator`         — VOC with background: predictions >= 20 fold to 20
                              (train_net.py:43-67).
`process()` bins every pixel with `catseg_semseg_confusion` (argmax over the class planes +
int64 bincount, exact), or, for the `"sem_seg_labels"` outputs of MODEL.CATSEG_HIP.OUTPUT "labels",
with `catseg_semseg_confusion_labels` from the argmax map the model already made; `evaluate()` sums the matrices over ranks (torch.distributed, as
detectron2's `all_gather`, plain_train_net.py:136-146) and forms the metrics on the host
from the small (N+1)^2 matrix.  With an `output_dir`, `process()` also keeps the COCO-stuff
RLE records of every prediction (`encode_json_sem_seg`, plain_train_net.py:125,207-228; the RLE
is pycocotools' `mask.encode`, restated in `coco_rle_encode` since pycocotools is absent) and
`evaluate()` gathers them over ranks and writes `sem_seg_predictions.json`
(plain_train_net.py:139-152).  With `rle="device"` (the default) the records come from the
column-major label runs of the argmax map, made on the device (`ops.label_runs`,
catseg_label_runs_*): only the runs cross to the host, where `rle_records_from_runs` reads every
label's RLE off them; `rle="host"` copies the map and encodes one mask per label as the reference
does.  Both give the same records and the same file.

With `boundary=[...]` the evaluators also report boundary-aware metrics (Boundary IoU, trimap and
eroded-boundary mIoU / pACC / mF1 per width; no counterpart in the reference): `process()` bins their
counters on the device from the argmax map and the ground truth (`ops.boundary_confusion`:
catseg_boundary_distance of both maps + catseg_boundary_confusion) and `evaluate()` forms
`boundary_metrics` from the reduced counters.  Without it nothing changes.

With `confidence={...}` they also report calibration (ECE, MCE, pACC@k, a reliability table and the coverage /
selective-pACC curve; no counterpart in the reference): `process()` bins the counters on the device
(`ops.confidence_bins`) from the top-k maps of a MODEL.CATSEG_HIP.CONFIDENCE "labels" output, or of a probability
volume after one `ops.postprocess_topk`, and `evaluate()` forms `confidence_metrics`.  Without it nothing changes.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import ops


def _metadata(dataset_name):
    """MetadataCatalog entry (detectron2's when importable, else cat_seg.data's stand-in, where
    the reference's dataset names are registered on import); None without a name."""
    from .data.catalog import MetadataCatalog
    return MetadataCatalog.get(dataset_name) if dataset_name else None


def _catalog_gt_loader(dataset_name):
    """detectron2 SemSegEvaluator's ground truth: the label file registered for the input's
    "file_name" (input_file_to_gt_file), read as stored (8-bit PNG or 16-bit TIFF)."""
    from PIL import Image
    from .data.catalog import DatasetCatalog
    table = {d["file_name"]: d["sem_seg_file_name"] for d in DatasetCatalog.get(dataset_name)}

    def load(inp):
        with Image.open(table[inp["file_name"]]) as im:
            return np.array(im, dtype=np.int64)
    return load


def coco_rle_encode(mask: np.ndarray) -> dict:
    """pycocotools `mask.encode` of one H x W binary mask (the call in plain_train_net.py:223), as
    {"size": [H, W], "counts": str}: run lengths over the column-major pixels, alternating and
    starting with a run of zeros (0 when pixel (0, 0) is set) -- maskApi.c rleEncode -- written
    with maskApi.c rleToString's compression: from the third count on, each count minus the count
    two before, in 5-bit groups low first, 0x20 = more groups follow, 0x10 of the last group = the
    sign, each group + 48 as one ASCII character.  pycocotools is not installed here: the string is
    checked against hand-derived vectors of that published algorithm and an independent decoder
    (tests/test_eval_cpu.py), not against pycocotools itself."""
    mask = np.asarray(mask)
    h, w = mask.shape
    return {"size": [int(h), int(w)], "counts": rle_counts_to_string(rle_mask_counts(mask))}


def rle_mask_counts(mask: np.ndarray) -> list:
    """maskApi.c rleEncode of one H x W binary mask: the run lengths over its column-major pixels,
    alternating and starting with a run of zeros (0 when pixel (0, 0) is set)."""
    flat = np.asarray(mask, dtype=bool).ravel(order="F")
    if flat.size == 0:
        return [0]
    edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    runs = np.diff(np.concatenate(([0], edges, [flat.size])))
    return ([0] if flat[0] else []) + runs.tolist()


def rle_counts_to_string(counts) -> str:
    """maskApi.c rleToString of a list of run lengths (the compression described in coco_rle_encode)."""
    # vectorised: x_i = c_i - c_{i-2} (i > 2), n_i = the fewest 5-bit groups whose
    # two's complement holds x_i (the loop "until the rest is the last group's sign extension")
    c = np.asarray(counts, dtype=np.int64)
    x = c.copy()
    if c.size > 3:
        x[3:] -= c[1:-2]
    n = np.ones_like(x)
    for k in range(1, 7):
        lim = 1 << (5 * k - 1)
        n += (x >= lim) | (x < -lim)
    ks = np.arange(int(n.max()))
    groups = (x[:, None] >> (5 * ks)[None, :]) & 0x1F
    more = ks[None, :] < (n[:, None] - 1)
    chars = groups + 48 + np.where(more, 0x20, 0)
    return chars[ks[None, :] < n[:, None]].astype(np.uint8).tobytes().decode("ascii")


def rle_records_from_runs(run_start, run_label, H: int, W: int) -> list:
    """Every per-label COCO RLE of one H x W label map from its column-major label runs (ops.label_runs:
    run_start ascending positions p = x * H + y, run_label the label of each run, runs maximal): a list of
    (label, {"size": [H, W], "counts": str}) in ascending label order, each equal to
    coco_rle_encode(map == label).  Run i is the interval [start_i, start_{i+1}) (the last ends at H * W); a
    label's counts are the gaps and lengths of its intervals in order, s_0, e_0 - s_0, s_1 - e_0, ... (a
    leading 0 by itself when s_0 == 0), plus the rest H * W - e_last when that is positive."""
    n = int(H) * int(W)
    start = np.asarray(run_start, dtype=np.int64).ravel()
    label = np.asarray(run_label).ravel()
    if start.size != label.size or start.size == 0 or start[0] != 0:
        raise ValueError("rle_records_from_runs: need one label per run and a first run at position 0")
    end = np.concatenate((start[1:], [n]))
    order = np.argsort(label, kind="stable")
    lab = label[order]
    # interleaved interval borders s_0, e_0, s_1, e_1, ... of all labels, label by label
    pts = np.empty(2 * order.size, dtype=np.int64)
    pts[0::2] = start[order]
    pts[1::2] = end[order]
    first = np.concatenate(([0], np.flatnonzero(lab[1:] != lab[:-1]) + 1, [lab.size]))
    size = [int(H), int(W)]
    records = []
    for a, b in zip(first[:-1].tolist(), first[1:].tolist()):
        p = pts[2 * a:2 * b]
        counts = np.empty(p.size + 1, dtype=np.int64)
        counts[0] = p[0]
        counts[1:-1] = p[1:] - p[:-1]
        counts[-1] = n - p[-1]
        records.append((int(lab[a]), {"size": size[:], "counts": rle_counts_to_string(
            counts if counts[-1] > 0 else counts[:-1])}))
    return records


_OBJ_GROUP = []


def _object_group():
    """A gloo process group over all ranks for object collectives (created once, collectively);
    None (the default group) when the default backend is gloo already."""
    if dist.get_backend() == "gloo":
        return None
    if not _OBJ_GROUP:
        _OBJ_GROUP.append(dist.new_group(backend="gloo"))
    return _OBJ_GROUP[0]


def reduce_confusion(conf: torch.Tensor) -> torch.Tensor:
    """Sum the per-rank confusion matrices (plain_train_net.py:136-146); returns a CPU int64 tensor."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        t = conf.clone() if dist.get_backend() == "nccl" else conf.cpu().clone()
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        conf = t
    return conf.cpu()


def semseg_metrics(conf: np.ndarray, class_names: Sequence[str], val_extra_classes: Sequence[str] = ()) -> dict:
    """The metrics of SemSegGzeroEvaluator.evaluate (plain_train_net.py:153-197) from an
    (N+1) x (N+1) confusion matrix indexed [pred][gt] (row N / column N: ignored pixels)."""
    conf = np.asarray(conf, dtype=np.int64)
    n = len(class_names)
    if conf.shape != (n + 1, n + 1):
        raise ValueError(f"confusion matrix {conf.shape} does not match {n} classes")
    core = conf[:-1, :-1].astype(np.float64)
    tp = np.diagonal(conf)[:-1].astype(np.float64)
    pos_gt = core.sum(axis=0)
    pos_pred = core.sum(axis=1)
    gt_seen = pos_gt > 0
    acc = np.where(gt_seen, tp / np.where(gt_seen, pos_gt, 1.0), np.nan)
    union = pos_gt + pos_pred - tp
    iou = np.where(gt_seen, tp / np.where(gt_seen, union, 1.0), np.nan)
    weights = pos_gt / pos_gt.sum()
    res = {"mIoU": 100 * iou[gt_seen].sum() / ((pos_gt + pos_pred) > 0).sum(),
           "fwIoU": 100 * (iou[gt_seen] * weights[gt_seen]).sum()}
    res.update({f"IoU-{c}": 100 * iou[i] for i, c in enumerate(class_names)})
    res["mACC"] = 100 * acc[gt_seen].sum() / gt_seen.sum()
    res["pACC"] = 100 * tp.sum() / pos_gt.sum()
    res.update({f"ACC-{c}": 100 * acc[i] for i, c in enumerate(class_names)})
    if len(val_extra_classes):
        extra = np.array([c in val_extra_classes for c in class_names])
        unseen = (100 * iou[extra]).sum() / len(val_extra_classes)
        seen = (100 * iou[~extra]).sum() / (n - len(val_extra_classes))
        res["seen_IoU"], res["unseen_IoU"] = seen, unseen
        res["harmonic mean"] = 2 * seen * unseen / (seen + unseen)
    return res


def boundary_specs(boundary) -> list:
    """The `boundary=` argument of the evaluators as a list of (kind, value, tag): ("px", n) is an absolute
    width of n pixels, tag "{n}px"; ("ratio", r) the per-image width max(1, round(r * image diagonal)), tag
    "{r:g}d".  Up to 8 specs; a bad one raises ValueError."""
    specs = []
    if isinstance(boundary, (str, bytes)) or not hasattr(boundary, "__iter__"):
        raise ValueError(f"boundary must be a sequence of ('px', n) / ('ratio', r) specs, got {boundary!r}")
    for spec in boundary:
        if not isinstance(spec, (tuple, list)) or len(spec) != 2 or spec[0] not in ("px", "ratio"):
            raise ValueError(f"boundary spec {spec!r}: expected ('px', n) or ('ratio', r)")
        kind, v = spec
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"boundary spec {spec!r}: the width must be a number")
        if kind == "px":
            if int(v) != v or not 1 <= int(v) <= 16383:
                raise ValueError(f"boundary spec {spec!r}: a pixel width is an integer in 1 .. 16383")
            specs.append(("px", int(v), f"{int(v)}px"))
        else:
            if not (v > 0 and v < 1):        # also refuses NaN
                raise ValueError(f"boundary spec {spec!r}: a ratio of the image diagonal lies in (0, 1)")
            specs.append(("ratio", float(v), f"{float(v):g}d"))
    if not 1 <= len(specs) <= 8:
        raise ValueError(f"boundary: 1 .. 8 specs, got {len(specs)}")
    tags = [s[2] for s in specs]
    if len(set(tags)) != len(tags):
        raise ValueError(f"boundary: two specs share a tag: {tags}")
    return specs


def boundary_widths(specs, H: int, W: int) -> list:
    """The widths in pixels of `boundary_specs` for an H x W image (a ratio: max(1, round(r * sqrt(H^2 + W^2))),
    at most 16383)."""
    return [v if kind == "px" else min(16383, max(1, int(round(v * float(np.sqrt(float(H) ** 2 + float(W) ** 2))))))
            for kind, v, _ in specs]


def boundary_metrics(conf, counters, class_names: Sequence[str], tags: Sequence[str]) -> dict:
    """The boundary-aware metrics from the (N+1) x (N+1) confusion matrix and the reduced counters of
    catseg_boundary_confusion (K ((N+1)^2 + 3N) integers; per width band_conf, inter, gt_band, pred_band), one
    width per tag t:
      BIoU@t-<class> = 100 inter / (gt_band + pred_band - inter), NaN where gt_band == 0; mBIoU@t their mean
      over the classes with gt_band > 0 (Boundary IoU, the counts accumulated over the dataset);
      trimap-mIoU@t, trimap-pACC@t = semseg_metrics of band_conf (the pixels within the width of a ground-truth
      class boundary); eroded-mIoU@t, eroded-pACC@t = semseg_metrics of conf - band_conf (those pixels left
      out), eroded-mF1@t = the mean over the classes seen in that matrix's ground truth of
      100 * 2 tp / (pos_gt + pos_pred).
    An empty band or an empty eroded map gives NaN, without a warning."""
    conf = np.asarray(conf, dtype=np.int64)
    n, n1 = len(class_names), len(class_names) + 1
    per = n1 * n1 + 3 * n
    counters = np.asarray(counters, dtype=np.int64).reshape(-1)
    if conf.shape != (n1, n1) or counters.size != len(tags) * per:
        raise ValueError(f"boundary_metrics: conf {conf.shape} / {counters.size} counters do not match {n} classes "
                         f"and {len(tags)} widths")
    nan = float("nan")
    res = {}

    def mean(v, seen):
        return float(v[seen].mean()) if seen.any() else nan

    for k, t in enumerate(tags):
        c = counters[k * per:(k + 1) * per]
        band = c[:n1 * n1].reshape(n1, n1)
        inter, gt_band, pred_band = (c[n1 * n1 + i * n:n1 * n1 + (i + 1) * n].astype(np.float64) for i in range(3))
        seen = gt_band > 0
        biou = np.where(seen, 100 * inter / np.where(seen, gt_band + pred_band - inter, 1.0), nan)
        res[f"mBIoU@{t}"] = mean(biou, seen)
        res.update({f"BIoU@{t}-{name}": float(biou[i]) for i, name in enumerate(class_names)})
        for prefix, m in (("trimap", band), ("eroded", conf - band)):
            if m[:-1, :-1].sum() > 0:
                sm = semseg_metrics(m, class_names)
                res[f"{prefix}-mIoU@{t}"], res[f"{prefix}-pACC@{t}"] = float(sm["mIoU"]), float(sm["pACC"])
            else:
                res[f"{prefix}-mIoU@{t}"] = res[f"{prefix}-pACC@{t}"] = nan
        core = (conf - band)[:-1, :-1].astype(np.float64)
        tp, pos_gt, pos_pred = np.diagonal(core), core.sum(axis=0), core.sum(axis=1)
        gseen = pos_gt > 0
        res[f"eroded-mF1@{t}"] = mean(np.where(gseen, 100 * 2 * tp / np.where(gseen, pos_gt + pos_pred, 1.0), nan), gseen)
    return res


def confidence_spec(confidence) -> dict:
    """The `confidence=` argument of the evaluators, checked and completed: {"bins": 1 .. 256 (15), "kind": "score"
    (the confidence of a pixel is the score of its rank-0 class) | "normalized" (that score / the mass of the class
    scores), "topk": 1 .. 4 (2), the ranks of pACC@k}."""
    if not isinstance(confidence, dict) or set(confidence) - {"bins", "kind", "topk"}:
        raise ValueError(f"confidence must be a dict with the keys bins, kind and topk, got {confidence!r}")
    spec = {"bins": int(confidence.get("bins", 15)), "kind": confidence.get("kind", "score"),
            "topk": int(confidence.get("topk", 2))}
    if not 1 <= spec["bins"] <= 256:
        raise ValueError(f"confidence: bins must lie in 1 .. 256, got {confidence.get('bins')!r}")
    if spec["kind"] not in ("score", "normalized"):
        raise ValueError(f"confidence: kind must be 'score' or 'normalized', got {spec['kind']!r}")
    if not 1 <= spec["topk"] <= 4:
        raise ValueError(f"confidence: topk must lie in 1 .. 4, got {confidence.get('topk')!r}")
    return spec


def confidence_metrics(counters, n_bins: int, K: int) -> dict:
    """The calibration metrics from the reduced counters of catseg_confidence_bins (3 n_bins + K + 2 integers:
    count, correct, conf_q24 per bin, hit per rank, valid, nan), every ratio in percent:
      ECE = sum over the bins of n_b / N |acc_b - conf_b|, MCE = the largest |acc_b - conf_b| of a bin with pixels
      (acc_b = correct_b / n_b, conf_b = the mean confidence conf_q24_b / 2^24 / n_b, N = sum n_b);
      pACC@k for k = 1 .. K = hit[k - 1] / valid: the share of pixels whose ground truth is among ranks 0 .. k-1;
      reliability = {"count", "accuracy", "confidence"}: per bin n_b, acc_b and conf_b (nan for an empty bin);
      coverage, selective-pACC = per bin b, the share of the pixels in bins >= b and the accuracy among them: what
      remains when everything below confidence b / n_bins is rejected (nan where nothing remains);
      nan-confidence = the number of pixels with a NaN confidence (they enter nothing else)."""
    c = np.asarray(counters, dtype=np.int64).reshape(-1)
    if c.size != 3 * n_bins + K + 2:
        raise ValueError(f"confidence_metrics: {c.size} counters do not match {n_bins} bins and K = {K}")
    count, correct, q24 = (c[i * n_bins:(i + 1) * n_bins].astype(np.float64) for i in range(3))
    hit, valid, nans = c[3 * n_bins:3 * n_bins + K].astype(np.float64), float(c[-2]), int(c[-1])
    total = count.sum()
    some = count > 0
    safe = np.where(some, count, 1.0)
    acc = np.where(some, correct / safe, np.nan)
    conf = np.where(some, q24 / 16777216.0 / safe, np.nan)
    gap = np.where(some, np.abs(correct / safe - q24 / 16777216.0 / safe), 0.0)
    res = {"ECE": 100 * float((count * gap).sum() / total) if total else float("nan"),
           "MCE": 100 * float(gap.max()) if total else float("nan")}
    for k in range(K):
        res[f"pACC@{k + 1}"] = 100 * hit[k] / valid if valid else float("nan")
    kept = count[::-1].cumsum()[::-1]
    kept_correct = correct[::-1].cumsum()[::-1]
    res["reliability"] = {"count": count.astype(np.int64).tolist(), "accuracy": (100 * acc).tolist(),
                          "confidence": (100 * conf).tolist()}
    res["coverage"] = (100 * kept / total).tolist() if total else [float("nan")] * n_bins
    res["selective-pACC"] = np.where(kept > 0, 100 * kept_correct / np.where(kept > 0, kept, 1.0), np.nan).tolist()
    res["nan-confidence"] = nans
    return res


class SemSegEvaluator:
    """reset() / process(inputs, outputs) / evaluate() -> {"sem_seg": metrics}.

    `confidence`: None, or a dict (`confidence_spec`) that turns the calibration metrics on: ECE, MCE, pACC@k, the
    reliability table and the coverage / selective-pACC curve (`confidence_metrics`), their counters binned on the
    device (ops.confidence_bins) from the top-k maps of a MODEL.CATSEG_HIP.CONFIDENCE "labels" output, or from
    one identity-size ops.postprocess_topk of a "sem_seg" probability output, and added to the "sem_seg" dict.

    `boundary`: None, or up to 8 width specs (`boundary_specs`) that turn the boundary-aware metrics on:
    Boundary IoU, trimap and eroded-boundary mIoU / pACC / mF1 per width (`boundary_metrics`), their counters
    binned on the device from the same maps (ops.boundary_confusion) and added to the "sem_seg" dict.

    Ground truth per input: `input["sem_seg_gt"]` (H x W labels, tensor or array), else
    `gt_loader(input)` (e.g. reading `input["file_name"]`'s `sem_seg_file_name` as the
    reference does).  `class_names` / `ignore_label` come from detectron2's MetadataCatalog
    when it is importable, else from the arguments."""

    clamp_pred = -1

    def __init__(self, dataset_name: Optional[str] = None, distributed: bool = True, output_dir=None, *,
                 class_names: Optional[Sequence[str]] = None, ignore_label: Optional[int] = None,
                 gt_loader: Optional[Callable] = None, device=None, rle: str = "device", boundary=None,
                 confidence=None):
        if rle not in ("device", "host"):
            raise ValueError(f"SemSegEvaluator: rle must be 'device' or 'host', got {rle!r}")
        self._rle = rle
        self._boundary = boundary_specs(boundary) if boundary is not None else None
        self._confidence = confidence_spec(confidence) if confidence is not None else None
        meta = _metadata(dataset_name)
        if class_names is None:
            class_names = meta.get("stuff_classes") if meta is not None else None
            if class_names is None:
                raise ValueError(f"SemSegEvaluator: no class names (dataset {dataset_name!r} has no 'stuff_classes' "
                                 "metadata and class_names= was not given)")
        self._class_names = list(class_names)
        self._num_classes = len(self._class_names)
        self._ignore_label = ignore_label if ignore_label is not None else (
            meta.get("ignore_label", 255) if meta is not None else 255)
        self._distributed = distributed
        self._output_dir = output_dir
        self._dataset_name = dataset_name
        self._gt_loader = gt_loader
        self._device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # contiguous training ids -> dataset category ids for the RLE records (plain_train_net.py:84-90)
        c2d = meta.get("stuff_dataset_id_to_contiguous_id") if meta is not None else None
        self._contiguous_id_to_dataset_id = {v: k for k, v in c2d.items()} if c2d else None
        self.reset()

    def reset(self):
        n1 = self._num_classes + 1
        self._conf = torch.zeros(n1 * n1, dtype=torch.int64, device=self._device)
        self._invalid = torch.zeros(1, dtype=torch.int64, device=self._device)
        self._predictions = []
        if self._boundary is not None:
            n = self._num_classes
            self._bcounters = torch.zeros(len(self._boundary) * (n1 * n1 + 3 * n), dtype=torch.int64,
                                          device=self._device)
        if self._confidence is not None:
            self._ccounters = torch.zeros(3 * self._confidence["bins"] + self._confidence["topk"] + 2,
                                          dtype=torch.int64, device=self._device)

    def _confidence_update(self, topk_labels, topk_score, mass, gt):
        """The calibration counters of one image from its top-k maps ((K, H, W), K >= topk) and, for the
        normalised kind, its mass."""
        K = self._confidence["topk"]
        if topk_labels.dim() != 3 or topk_labels.shape[0] < K or tuple(topk_labels.shape[1:]) != tuple(gt.shape):
            raise ValueError(f"confidence: top-k maps {tuple(topk_labels.shape)} do not hold {K} ranks of a "
                             f"{tuple(gt.shape)} image")
        conf = topk_score[0]
        if self._confidence["kind"] == "normalized":
            conf = conf / mass
        ops.confidence_bins(topk_labels[:K].to(self._device, torch.int32).contiguous(),
                            conf.to(self._device, torch.float32).contiguous(), gt, self._ccounters,
                            num_classes=self._num_classes, ignore_label=self._ignore_label,
                            clamp_pred=self.clamp_pred, n_bins=self._confidence["bins"])

    @property
    def boundary_tags(self) -> list:
        """The width tags of `boundary=`, in order (empty without it)."""
        return [s[2] for s in self._boundary] if self._boundary is not None else []

    def _boundary_update(self, labels, gt):
        """The boundary counters of one image from its int32 prediction map (the fold is applied on the device)."""
        H, W = labels.shape
        ops.boundary_confusion(labels, gt, boundary_widths(self._boundary, H, W), self._bcounters,
                               num_classes=self._num_classes, ignore_label=self._ignore_label,
                               clamp_pred=self.clamp_pred)

    def _gt(self, inp) -> torch.Tensor:
        gt = inp.get("sem_seg_gt")
        if gt is None:
            if self._gt_loader is None and self._dataset_name and "file_name" in inp:
                self._gt_loader = _catalog_gt_loader(self._dataset_name)
            if self._gt_loader is None:
                raise KeyError("input has no 'sem_seg_gt' and no gt_loader / registered dataset was given")
            gt = self._gt_loader(inp)
        gt = torch.as_tensor(np.asarray(gt) if not torch.is_tensor(gt) else gt)
        return gt.to(self._device, torch.int32).contiguous()

    def process(self, inputs, outputs):
        with torch.cuda.device(self._device):      # the kernel runs on this device's current stream
            self._process(inputs, outputs)

    def _process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            if isinstance(out, dict) and "sem_seg_labels" in out:
                self._process_labels(inp, out["sem_seg_labels"])
                if self._confidence is not None:
                    missing = [k for k in ("sem_seg_topk_labels", "sem_seg_topk_score", "sem_seg_mass") if k not in out]
                    if missing:
                        raise ValueError(f"SemSegEvaluator(confidence=...): the 'labels' output has no {missing}: "
                                         "build the model with MODEL.CATSEG_HIP.CONFIDENCE.ENABLED")
                    self._confidence_update(out["sem_seg_topk_labels"], out["sem_seg_topk_score"],
                                            out["sem_seg_mass"], self._gt(inp))
                continue
            probs = out["sem_seg"] if isinstance(out, dict) else out
            probs = probs.to(self._device, torch.float32).contiguous()
            gt = self._gt(inp)
            if tuple(gt.shape) != tuple(probs.shape[1:]):
                raise ValueError(f"gt {tuple(gt.shape)} vs prediction {tuple(probs.shape[1:])}")
            ops.semseg_confusion(probs, gt, self._conf, self._invalid, num_classes=self._num_classes,
                                 ignore_label=self._ignore_label, clamp_pred=self.clamp_pred)
            device_rle = bool(self._output_dir) and self._rle == "device"
            # the argmax map: for the boundary counters and for the label runs of the records
            labels = probs.argmax(dim=0).to(torch.int32) if device_rle or self._boundary is not None else None
            if self._boundary is not None:
                self._boundary_update(labels, gt)
            if self._confidence is not None:
                # the top-k maps of the volume itself: one identity-size launch, no sigmoid
                maps = ops.postprocess_topk(probs[None], self._confidence["topk"], sigmoid=False,
                                            out_hw=tuple(probs.shape[1:]))
                self._confidence_update(maps["topk_labels"][0], maps["topk_score"][0], maps["mass"][0], gt)
            if device_rle:
                # the records are written only with an output_dir (the reference builds them for every
                # image); only the label runs of the argmax map are brought to the host
                self._records_from_device(labels, inp.get("file_name"))
            elif self._output_dir:
                pred = probs.argmax(dim=0)
                if self.clamp_pred >= 0:
                    pred = pred.clamp(max=self.clamp_pred)
                self._predictions.extend(self.encode_json_sem_seg(pred.cpu().numpy(), inp.get("file_name")))

    def _process_labels(self, inp, labels):
        """An output of MODEL.CATSEG_HIP.OUTPUT "labels": the argmax map is binned as it is
        (catseg_semseg_confusion_labels), and is what the RLE records are built from."""
        labels = labels.to(self._device, torch.int32).contiguous()
        gt = self._gt(inp)
        if labels.dim() != 2 or tuple(gt.shape) != tuple(labels.shape):
            raise ValueError(f"gt {tuple(gt.shape)} vs label map {tuple(labels.shape)}")
        ops.semseg_confusion_labels(labels, gt, self._conf, self._invalid, num_classes=self._num_classes,
                                    ignore_label=self._ignore_label, clamp_pred=self.clamp_pred)
        if self._boundary is not None:
            self._boundary_update(labels, gt)
        if self._output_dir and self._rle == "device":
            self._records_from_device(labels, inp.get("file_name"))
        elif self._output_dir:
            pred = labels.to(torch.int64)
            if self.clamp_pred >= 0:
                pred = pred.clamp(max=self.clamp_pred)
            self._predictions.extend(self.encode_json_sem_seg(pred.cpu().numpy(), inp.get("file_name")))

    def _records_from_device(self, labels, input_file_name):
        """rle="device": the label runs of an int32 device label map (ops.label_runs, the clamp_pred fold
        applied there) cross to the host, and the records are assembled from them."""
        H, W = labels.shape
        run_start, run_label = ops.label_runs(labels, clamp_pred=self.clamp_pred)
        self._predictions.extend(self.encode_json_label_runs(run_start.cpu().numpy(), run_label.cpu().numpy(),
                                                             H, W, input_file_name))

    def _dataset_id(self, label) -> int:
        if self._contiguous_id_to_dataset_id is None:
            return int(label)
        if int(label) not in self._contiguous_id_to_dataset_id:
            raise AssertionError(f"Label {label} is not in the metadata info for {self._dataset_name}")
        return self._contiguous_id_to_dataset_id[int(label)]

    def encode_json_label_runs(self, run_start, run_label, H, W, input_file_name) -> list:
        """encode_json_sem_seg from the column-major label runs of the argmax map (numpy arrays, as
        ops.label_runs makes them on the device) instead of the map: the same records in the same order."""
        return [{"file_name": input_file_name, "category_id": self._dataset_id(label), "segmentation": rle}
                for label, rle in rle_records_from_runs(run_start, run_label, H, W)]

    def encode_json_sem_seg(self, sem_seg: np.ndarray, input_file_name) -> list:
        """COCO-stuff records of one argmax map (plain_train_net.py:207-228): one per label present,
        {"file_name", "category_id", "segmentation": RLE}, labels mapped to dataset ids when the
        metadata has stuff_dataset_id_to_contiguous_id."""
        records = []
        for label in np.unique(sem_seg):
            records.append({"file_name": input_file_name, "category_id": self._dataset_id(label),
                            "segmentation": coco_rle_encode(sem_seg == label)})
        return records

    def predictions(self) -> list:
        """The RLE records of every processed image, gathered over ranks in rank order
        (plain_train_net.py:139-140)."""
        if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            parts = [None] * dist.get_world_size()
            # Python objects go through a gloo group (as detectron2's comm.all_gather does), never
            # pickled into device buffers of the RCCL group
            dist.all_gather_object(parts, self._predictions, group=_object_group())
            return [r for part in parts for r in part]
        return list(self._predictions)

    def confusion_matrix(self) -> np.ndarray:
        n1 = self._num_classes + 1
        conf = reduce_confusion(self._conf) if self._distributed else self._conf.cpu()
        return conf.numpy().reshape(n1, n1)

    def _metrics(self, conf):
        return semseg_metrics(conf, self._class_names)

    def evaluate(self):
        invalid = int(reduce_confusion(self._invalid)[0]) if self._distributed else int(self._invalid.item())
        if invalid:
            # the reference's bincount would outgrow the matrix and its reshape would fail
            raise ValueError(f"{invalid} ground-truth labels outside [0, {self._num_classes}) and != ignore_label")
        conf = self.confusion_matrix()
        bcounters = None
        if self._boundary is not None:
            bcounters = (reduce_confusion(self._bcounters) if self._distributed else self._bcounters.cpu()).numpy()
        ccounters = None
        if self._confidence is not None:
            ccounters = (reduce_confusion(self._ccounters) if self._distributed else self._ccounters.cpu()).numpy()
        preds = self.predictions() if self._output_dir else None
        if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
            return None
        if self._output_dir:
            import json
            import os
            os.makedirs(self._output_dir, exist_ok=True)
            with open(os.path.join(self._output_dir, "sem_seg_predictions.json"), "w") as f:
                f.write(json.dumps(preds))
        res = self._metrics(conf)
        if bcounters is not None:
            res.update(boundary_metrics(conf, bcounters, self._class_names, [s[2] for s in self._boundary]))
        if ccounters is not None:
            res.update(confidence_metrics(ccounters, self._confidence["bins"], self._confidence["topk"]))
        if self._output_dir:
            torch.save(res, os.path.join(self._output_dir, "sem_seg_evaluation.pth"))
        return OrderedDict({"sem_seg": res})


class SemSegGzeroEvaluator(SemSegEvaluator):
    """+ seen / unseen IoU and harmonic mean over `val_extra_classes` (plain_train_net.py:48-200)."""

    def __init__(self, *args, val_extra_classes: Optional[Sequence[str]] = None, **kw):
        super().__init__(*args, **kw)
        if val_extra_classes is None:
            meta = _metadata(args[0] if args else kw.get("dataset_name"))
            val_extra_classes = meta.get("val_extra_classes", ()) if meta is not None else ()
        self._val_extra_classes = list(val_extra_classes)

    def _metrics(self, conf):
        return semseg_metrics(conf, self._class_names, self._val_extra_classes)


class VOCbEvaluator(SemSegEvaluator):
    """VOC with background: predictions >= 20 fold to class 20 (train_net.py:55-58)."""

    clamp_pred = 20
