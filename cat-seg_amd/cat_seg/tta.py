"""The TTA wrapper the package exports (`from cat_seg import SemanticSegmentorWithTTA`, train_net.py:74-80,
260-274): cat_seg.test_time_augmentation's, which refuses a model built with MODEL.CATSEG_HIP.OUTPUT
"labels" at construction.  The wrapper averages the probabilities of the augmented views; a label map
cannot be averaged, and without this check the first call would fail on the missing "sem_seg" key."""
from __future__ import annotations

from torch import nn

from . import test_time_augmentation as _tta


class SemanticSegmentorWithTTA(_tta.SemanticSegmentorWithTTA):
    def __init__(self, cfg, model, tta_mapper=None, batch_size: int = 1):
        inner = model.module if isinstance(model, nn.parallel.DistributedDataParallel) else model
        output = getattr(inner, "output", "probs")
        if output != "probs":
            raise ValueError("SemanticSegmentorWithTTA averages probabilities over the augmented views: wrap a model "
                             f"built with MODEL.CATSEG_HIP.OUTPUT 'probs', not {output!r}")
        super().__init__(cfg, model, tta_mapper=tta_mapper, batch_size=batch_size)
