"""Looking at predictions: palettes, the reference figure's panels, a legend and PNG files, round
`ops.render_labels` (the reference's cat_seg/utils/visualizer OVRSSS_Visualizer.save_visual and viz.py: imgviz
label2rgb over the grey image at alpha 0.5, a prediction panel, a ground-truth panel).

Every pixel is coloured on the device by one kernel per panel, each writing its own columns of one wide picture,
and one copy brings that picture to the host, where PIL writes the PNG and, when asked, draws a legend strip under
it.  The map, the score and the image never go to the host.  DESIGN.md section 4, "Rendering".
"""
from __future__ import annotations

import contextlib
import os
from collections import OrderedDict
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops


def label_colormap(n: int = 256) -> np.ndarray:
    """The PASCAL VOC colour map, (n, 3) uint8: the bits of the label dealt to r, g, b from the top bit down
    ((0,0,0), (128,0,0), (0,128,0), (128,128,0), ...), what imgviz.label_colormap gives."""
    i = np.arange(int(n), dtype=np.int64)
    cmap = np.zeros((int(n), 3), np.int64)
    for j in range(8):
        for c in range(3):
            cmap[:, c] |= ((i >> (3 * j + c)) & 1) << (7 - j)
    return cmap.astype(np.uint8)


def _default_device():
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def palette_for(dataset, n: Optional[int] = None, device=None) -> torch.Tensor:
    """The palette of a dataset as an (n, 3) uint8 tensor on `device` (the GPU when there is one): the catalog's
    stuff_colors where it has them (a name, or a Metadata object), the colour map for the classes beyond them or
    for a dataset without colours (None, "" or an unknown name included).  n defaults to the number of colours
    (or of stuff_classes); at most 8192."""
    meta = dataset
    if dataset is None or isinstance(dataset, str):
        from .data.catalog import MetadataCatalog
        meta = MetadataCatalog.get(dataset) if dataset and dataset in MetadataCatalog.list() else None
    colors = list(meta.get("stuff_colors", None) or []) if meta is not None else []
    if n is None:
        n = len(colors) or len((meta.get("stuff_classes", None) if meta is not None else None) or []) or 256
    if not 1 <= int(n) <= 8192:
        raise ValueError(f"palette_for: n must lie in 1 .. 8192, got {n!r}")
    pal = label_colormap(int(n))
    k = min(len(colors), int(n))
    if k:
        pal[:k] = np.asarray(colors[:k], dtype=np.uint8).reshape(k, 3)
    return torch.from_numpy(pal).to(device if device is not None else _default_device())


def _maps(result):
    """(labels, score) of an OUTPUT "labels" result dict, of a {"sem_seg": probabilities} dict (argmax on the
    device) or of a bare label map."""
    if torch.is_tensor(result):
        return result, None
    if "sem_seg_labels" in result:
        return result["sem_seg_labels"], result.get("sem_seg_score")
    score, labels = result["sem_seg"].max(dim=0)
    return labels.to(torch.int32), score.to(torch.float32).contiguous()


def _device_image(image, device):
    """A (3, h, w) or (h, w, 3) image as uint8 on `device`; a float image is clamped to 0 .. 255 and truncated."""
    if image is None:
        return None
    image = torch.as_tensor(image).to(device)
    return image if image.dtype == torch.uint8 else image.clamp(0, 255).to(torch.uint8)


def render_result(result, palette, image=None, gt=None, *, score_alpha=False, **options) -> torch.Tensor:
    """ops.render_labels of a result dict ("sem_seg_labels" / "sem_seg_score", or "sem_seg"): the overlay over
    `image`, with `gt` the error map.  score_alpha: fade the colours by the score.  `options`: the keyword
    arguments of ops.render_labels (alpha, gray, edge_px, factor, out, ...)."""
    labels, score = _maps(result)
    gt = None if gt is None else torch.as_tensor(gt).to(labels.device, torch.int32)
    return ops.render_labels(labels, palette, image=_device_image(image, labels.device), gt=gt,
                             score=score if score_alpha else None, **options)


def panel_names(image: bool, gt: bool) -> list:
    """The panels of `panels`, left to right."""
    return (["image"] if image else []) + ["overlay", "labels"] + (["gt", "error"] if gt else [])


def panels(result, palette, image=None, gt=None, *, factor=1, ignore_label=255, score_alpha=False,
           **options) -> torch.Tensor:
    """The reference figure's panels side by side in one (Ho, k Wo, 3) uint8 device tensor (panel_names): the
    image, the overlay (render_result with `options`), the plain label colours and, with gt, the ground truth's
    colours and the error map (the overlay with wrong pixels in error_rgb and ignored ones in ignore_rgb).  Every
    panel is one ops.render_labels launch into its own columns of the result; nothing is concatenated afterwards."""
    labels, score = _maps(result)
    dev = labels.device
    image = _device_image(image, dev)
    gt = None if gt is None else torch.as_tensor(gt).to(dev, torch.int32)
    names = panel_names(image is not None, gt is not None)
    H, W = labels.shape
    Ho, Wo = -(-H // factor), -(-W // factor)
    wide = torch.empty((Ho, len(names) * Wo, 3), dtype=torch.uint8, device=dev)
    score = score if score_alpha else None
    gt_options = {k: options[k] for k in ("error_rgb", "ignore_rgb") if k in options}
    overlay = {k: v for k, v in options.items() if k not in gt_options}
    for k, name in enumerate(names):
        out = wide[:, k * Wo:(k + 1) * Wo]
        if name == "image":                        # alpha 0 leaves the image: the same sampling and cell means
            ops.render_labels(labels, palette, image=image, gray=False, alpha=0.0, factor=factor, out=out)
        elif name == "overlay":
            ops.render_labels(labels, palette, image=image, score=score, factor=factor, out=out, **overlay)
        elif name == "labels":
            ops.render_labels(labels, palette, factor=factor, out=out,
                              **{k: overlay[k] for k in ("other_rgb", "clamp_pred") if k in overlay})
        elif name == "gt":
            ops.render_labels(gt, palette, factor=factor, out=out,
                              **{k: overlay[k] for k in ("other_rgb",) if k in overlay})
        else:
            ops.render_labels(labels, palette, image=image, score=score, gt=gt, ignore_label=ignore_label,
                              factor=factor, out=out, **options)
    return wide


def classes_present(labels: torch.Tensor, n: int) -> list:
    """The class numbers 0 .. n-1 that occur in the map, from a bincount on the device (n values come back)."""
    flat = labels.reshape(-1).to(torch.int64)
    flat = flat[(flat >= 0) & (flat < n)]
    return torch.nonzero(torch.bincount(flat, minlength=n)).reshape(-1).tolist()


def legend_strip(names: Sequence[str], palette, present: Sequence[int], width: int, swatch: int = 12) -> np.ndarray:
    """A (h, width, 3) uint8 legend on the host: a swatch and the name of every class of `present`, set in PIL's
    default font, wrapped into as many lines as the width asks for."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default()
    pal = palette.cpu().numpy() if torch.is_tensor(palette) else np.asarray(palette)
    probe = ImageDraw.Draw(Image.new("RGB", (1, 1)))
    pad, line = 4, swatch + 4
    items, x, y = [], pad, pad
    for c in present:
        text = str(names[c]) if c < len(names) else str(c)
        w = swatch + 3 + int(probe.textlength(text, font=font)) + 2 * pad
        if x > pad and x + w > width:
            x, y = pad, y + line
        items.append((x, y, c, text))
        x += w
    img = Image.new("RGB", (int(width), y + line), (255, 255, 255))
    draw = ImageDraw.Draw(img)
    for x, y, c, text in items:
        colour = tuple(int(v) for v in pal[c]) if c < len(pal) else (0, 0, 0)
        draw.rectangle([x, y, x + swatch - 1, y + swatch - 1], fill=colour, outline=(0, 0, 0))
        draw.text((x + swatch + 3, y), text, fill=(0, 0, 0), font=font)
    return np.asarray(img, dtype=np.uint8)


def save_png(path: str, rgb, legend: Optional[np.ndarray] = None) -> None:
    """Write an (h, w, 3) uint8 picture (a device tensor: its one copy to the host happens here) as a PNG, with the
    legend strip (legend_strip, as wide as the picture) under it."""
    from PIL import Image
    arr = rgb.cpu().numpy() if torch.is_tensor(rgb) else np.asarray(rgb)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"save_png: an (h, w, 3) uint8 picture is expected, got {arr.dtype} {arr.shape}")
    if legend is not None:
        if legend.shape[1] != arr.shape[1]:
            raise ValueError(f"save_png: the legend is {legend.shape[1]} wide, the picture {arr.shape[1]}")
        arr = np.concatenate([arr, legend], axis=0)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(arr)).save(path)


class PredictionVisualizer:
    """Writes <output_dir>/viz/<file stem>.png per image, the panels of `panels` (the reference's viz.py), in the
    evaluators' reset / process / evaluate shape, so it sits in DatasetEvaluators beside SemSegEvaluator.

    The palette and the class names come from the dataset's metadata (palette_for; stuff_classes) unless given.
    The ground truth is the input's "sem_seg_gt", else `gt_loader(input)`, else the label file the catalog
    registers for the input's "file_name" (the evaluators' loader); with gt=False, or where none of them is
    there, the two ground-truth panels are left out.  Accepts OUTPUT "labels" results and "sem_seg" probabilities
    (argmax on the device).  `options`: the keyword arguments of `panels` (alpha, gray, edge_px, factor, ...)."""

    def __init__(self, dataset_name: Optional[str] = None, output_dir: str = ".", *, palette=None,
                 class_names: Optional[Sequence[str]] = None, gt: bool = True, gt_loader=None, legend: bool = False,
                 **options):
        from .evaluation import _metadata
        meta = _metadata(dataset_name)
        self._dataset_name, self._output_dir = dataset_name, output_dir
        if class_names is None:
            class_names = (meta.get("stuff_classes", None) or []) if meta is not None else []
        self._names = list(class_names)
        self._palette_arg, self._palette = palette, None
        self._gt, self._gt_loader, self._legend, self._options = bool(gt), gt_loader, bool(legend), dict(options)
        if meta is not None and "ignore_label" not in self._options and meta.get("ignore_label", None) is not None:
            self._options["ignore_label"] = int(meta.get("ignore_label"))
        self.written: list = []

    def reset(self):
        self.written = []

    def path_for(self, inp, index: int = 0) -> str:
        """<output_dir>/viz/<stem of the input's file_name>.png; an input without a file name is numbered."""
        name = inp.get("file_name") if isinstance(inp, dict) else None
        stem = os.path.splitext(os.path.basename(name))[0] if name else f"{index:06d}"
        return os.path.join(self._output_dir, "viz", stem + ".png")

    def _ground_truth(self, inp):
        if not self._gt:
            return None
        gt = inp.get("sem_seg_gt")
        if gt is None:
            if self._gt_loader is None and self._dataset_name and "file_name" in inp:
                from .evaluation import _catalog_gt_loader
                self._gt_loader = _catalog_gt_loader(self._dataset_name)
            if self._gt_loader is None:
                return None
            gt = self._gt_loader(inp)
        return torch.as_tensor(np.asarray(gt) if not torch.is_tensor(gt) else gt)

    def picture(self, inp, out) -> torch.Tensor:
        """The panels of one input / output pair, on the device."""
        labels, _ = _maps(out)
        if self._palette is None or self._palette.device != labels.device:
            pal = self._palette_arg
            n = max(len(self._names), 1) if self._names else None
            self._palette = (palette_for(self._dataset_name, n, device=labels.device) if pal is None
                             else torch.as_tensor(pal).to(labels.device, torch.uint8))
        return panels(out, self._palette, image=inp.get("image"), gt=self._ground_truth(inp), **self._options)

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            labels, _ = _maps(out)
            with torch.cuda.device(labels.device) if labels.is_cuda else contextlib.nullcontext():
                pic = self.picture(inp, out)
                legend = None
                if self._legend:
                    n = int(self._palette.shape[0])
                    legend = legend_strip(self._names, self._palette, classes_present(labels, n), pic.shape[1])
            path = self.path_for(inp, len(self.written))
            save_png(path, pic, legend)
            self.written.append(path)

    def evaluate(self):
        return OrderedDict()
