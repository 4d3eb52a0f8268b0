"""The TTA wrapper the package exports (`from cat_seg import SemanticSegmentorWithTTA`, train_net.py:74-80,
260-274): cat_seg.test_time_augmentation's with MODEL.CATSEG_HIP.TTA_MERGE.

"host" (default) is that wrapper as it stands: it averages the probabilities of the augmented views in
torch; a label map cannot be averaged, so a model built with MODEL.CATSEG_HIP.OUTPUT "labels" is refused
at construction (without this check the first call would fail on the missing "sem_seg" key).

"device" replaces the merge (reference test_time_augmentation.py:81-108): the views' low-resolution logits
(CATSeg.forward_logits) go through one catseg_postprocess_tta launch, which resizes, flips back, sums and
scales without the K full-size volumes, and returns a label map for a model built with OUTPUT "labels"."""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from . import test_time_augmentation as _tta
from .data import transforms as T

MAX_DEVICE_VIEWS = 32        # catseg_postprocess_tta's view table


def tta_merge_from_cfg(cfg) -> str:
    """MODEL.CATSEG_HIP.TTA_MERGE: "host" (default, also when the key is absent) or "device"."""
    node = cfg
    for k in ("MODEL", "CATSEG_HIP", "TTA_MERGE"):
        node = node.get(k, None) if isinstance(node, dict) else getattr(node, k, None)
        if node is None:
            return "host"
    if node not in ("host", "device"):
        raise ValueError(f"MODEL.CATSEG_HIP.TTA_MERGE must be 'host' or 'device', got {node!r}")
    return node


class SemanticSegmentorWithTTA(_tta.SemanticSegmentorWithTTA):
    def __init__(self, cfg, model, tta_mapper=None, batch_size: int = 1):
        inner = model.module if isinstance(model, nn.parallel.DistributedDataParallel) else model
        output = getattr(inner, "output", "probs")
        merge = tta_merge_from_cfg(cfg)
        if output != "probs" and merge == "host":
            raise ValueError("SemanticSegmentorWithTTA averages probabilities over the augmented views: wrap a model "
                             f"built with MODEL.CATSEG_HIP.OUTPUT 'probs', not {output!r}")
        if merge == "device" and bool(getattr(inner, "sliding_window", False)):
            raise ValueError("SemanticSegmentorWithTTA: MODEL.CATSEG_HIP.TTA_MERGE 'device' merges the views' logits "
                             "before the resize, which TEST.SLIDING_WINDOW has no single tensor of: use 'host'")
        if merge == "device" and bool(getattr(inner, "confidence", False)):
            raise ValueError("SemanticSegmentorWithTTA: MODEL.CATSEG_HIP.TTA_MERGE 'device' does not serve "
                             "MODEL.CATSEG_HIP.CONFIDENCE: the merge of the views ranks averaged probabilities and "
                             "keeps one class per pixel")
        super().__init__(cfg, model, tta_mapper=tta_mapper, batch_size=batch_size)
        self.tta_merge = merge

    def _inference_one_image(self, inp):
        if self.tta_merge == "host":
            return super()._inference_one_image(inp)
        return self._inference_one_image_device(inp)

    def _inference_one_image_device(self, inp):
        """The views' logits collected in one (K, T, h, w) buffer and merged by one catseg_postprocess_tta
        launch into fresh outputs; the K full-size volumes of the host merge are never formed."""
        augmented = self.tta_mapper(inp)
        K = len(augmented)
        if not 1 <= K <= MAX_DEVICE_VIEWS:
            raise ValueError(f"SemanticSegmentorWithTTA: TTA_MERGE 'device' merges 1 to {MAX_DEVICE_VIEWS} views per "
                             f"image, the mapper produced {K}: use fewer TEST.AUG.MIN_SIZES or TTA_MERGE 'host'")
        flips = [int(any(isinstance(t, T.HFlipTransform) for t in a.pop("transforms"))) for a in augmented]
        height, width = int(inp["height"]), int(inp["width"])
        buf, views = None, []
        for i in range(0, K, self.batch_size):
            logits, crops = self.model.forward_logits(augmented[i:i + self.batch_size])
            if buf is None:
                buf = torch.empty((K,) + tuple(logits.shape[1:]), device=logits.device, dtype=torch.float32)
            elif tuple(logits.shape[1:]) != tuple(buf.shape[1:]):
                raise RuntimeError(f"SemanticSegmentorWithTTA: views with logits {tuple(logits.shape[1:])} and "
                                   f"{tuple(buf.shape[1:])} cannot be merged on the device")
            # before the next model call: on the hipGraph branch `logits` is the captured buffer
            buf[i:i + logits.shape[0]].copy_(logits)
            views += [(ch, cw, flips[i + j]) for j, (ch, cw) in enumerate(crops)]
        del augmented
        dev = buf.device
        if getattr(self.model, "output", "probs") == "labels":
            labels = torch.empty(height, width, device=dev, dtype=torch.int32)
            score = torch.empty(height, width, device=dev, dtype=torch.float32)
            ops.postprocess_tta(buf, views, labels=labels, score=score)
            result = {"sem_seg_labels": labels, "sem_seg_score": score}
            add_regions = getattr(self.model, "add_regions", None)     # MODEL.CATSEG_HIP.REGIONS, on the merged map
            # (and MODEL.CATSEG_HIP.RENDER, over the image the views were made from)
            return add_regions(result, inp.get("image")) if add_regions is not None else result
        probs = torch.empty(buf.shape[1], height, width, device=dev, dtype=torch.float32)
        ops.postprocess_tta(buf, views, probs=probs)
        return {"sem_seg": probs}
