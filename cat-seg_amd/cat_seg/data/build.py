"""Data loading: the test loader (detectron2 `build_detection_test_loader` + `InferenceSampler`,
used by the reference through `Trainer.test`, train_net.py:302) and the train loader
(`build_detection_train_loader` + `TrainingSampler`, train_net.py:160-172).

Every rank takes a contiguous slice of the dataset (the first len % world ranks one item
more: `cat_seg.distributed.shard_range`, the InferenceSampler split), maps it with the test
mapper and yields lists of `batch_size` dicts (detectron2 uses 1; CATSeg.forward takes any
number and runs them as one batch on the device).
"""
from __future__ import annotations

import itertools
from typing import List, Optional, Sequence, Union

import torch
import torch.distributed as dist
import torch.utils.data as tud

from ..distributed import shard_range
from .catalog import DatasetCatalog
from .dataset_mappers import CATSegTestDatasetMapper


def trivial_batch_collator(batch):
    return batch


class _MapDataset(tud.Dataset):
    def __init__(self, dicts: Sequence[dict], mapper):
        self.dicts, self.mapper = list(dicts), mapper

    def __len__(self):
        return len(self.dicts)

    def __getitem__(self, i):
        return self.mapper(self.dicts[i])


class InferenceSampler(tud.Sampler):
    """This rank's contiguous [begin, end) of range(size), in order."""

    def __init__(self, size: int, rank: Optional[int] = None, world: Optional[int] = None):
        if rank is None or world is None:
            on = dist.is_available() and dist.is_initialized()
            rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
        self._range = range(*shard_range(size, rank, world))

    def __iter__(self):
        return iter(self._range)

    def __len__(self):
        return len(self._range)


class TrainingSampler(tud.Sampler):
    """detectron2's TrainingSampler: an infinite stream of indices, one shuffled epoch of range(size)
    after the other (in order when `shuffle` is off), of which this rank takes every `world`-th element
    starting at `rank`.  Every rank shuffles with the same seed, so the ranks partition each epoch."""

    def __init__(self, size: int, shuffle: bool = True, seed: int = 0, rank: Optional[int] = None,
                 world: Optional[int] = None):
        if size <= 0:
            raise ValueError(f"TrainingSampler: dataset of size {size}")
        if rank is None or world is None:
            on = dist.is_available() and dist.is_initialized()
            rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
        self.size, self.shuffle, self.seed, self.rank, self.world = size, shuffle, int(seed), rank, world

    def _infinite(self):
        g = torch.Generator()
        g.manual_seed(self.seed)
        while True:
            yield from (torch.randperm(self.size, generator=g) if self.shuffle else torch.arange(self.size)).tolist()

    def __iter__(self):
        yield from itertools.islice(self._infinite(), self.rank, None, self.world)


class _TrainBatches:
    """The infinite iterable `build_train_loader` returns: the DataLoader's batches, each passed through
    `post` (the device augmentation) in the main process when there is one."""

    def __init__(self, loader, post=None):
        self.loader, self.post = loader, post

    def __iter__(self):
        for batch in self.loader:
            yield self.post(batch) if self.post is not None else batch


def build_train_loader(dataset: Union[str, Sequence[dict]], *, cfg, mapper=None, total_batch_size: Optional[int] = None,
                       num_workers: Optional[int] = None, seed: int = 0, rank: Optional[int] = None,
                       world: Optional[int] = None, device=None):
    """detectron2's `build_detection_train_loader` for CAT-Seg, without detectron2: yields lists of
    IMS_PER_BATCH / world mapped dicts, forever (TrainingSampler).  `dataset`: a registered name or a list
    of dataset dicts.  MODEL.CATSEG_HIP.TRAIN_INPUT selects where the augmentation runs:

      "host"    workers run MaskFormerSemanticDatasetMapper (PIL / numpy); the batches are what it returns
      "device"  workers run RawTrainMapper (decode only) and every batch goes through DeviceTrainAugment
                in the main process: one fused kernel per batch (csrc/train_input.hip)

    A `mapper` of the caller's replaces the worker-side one."""
    from .dataset_mappers import MaskFormerSemanticDatasetMapper
    mode = str(getattr(cfg.MODEL.CATSEG_HIP, "TRAIN_INPUT", "host"))
    if mode not in ("host", "device"):
        raise ValueError(f"MODEL.CATSEG_HIP.TRAIN_INPUT {mode!r}: expected 'host' or 'device'")
    if rank is None or world is None:
        on = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
    total = int(total_batch_size if total_batch_size is not None else cfg.SOLVER.IMS_PER_BATCH)
    if total <= 0 or total % world:
        raise ValueError(f"total batch size {total} is not a positive multiple of the world size {world}")
    dicts: List[dict] = DatasetCatalog.get(dataset) if isinstance(dataset, str) else list(dataset)
    post = None
    if mode == "device":
        from .device_input import DeviceTrainAugment
        from .train_input import RawTrainMapper
        post = DeviceTrainAugment(cfg, device if device is not None else "cuda", seed=seed, rank=rank)
        mapper = mapper if mapper is not None else RawTrainMapper(cfg)
    else:
        mapper = mapper if mapper is not None else MaskFormerSemanticDatasetMapper(cfg, True)
    ds = _MapDataset(dicts, mapper)
    sampler = TrainingSampler(len(ds), True, seed, rank, world)
    bs = tud.BatchSampler(sampler, total // world, drop_last=True)
    workers = int(num_workers if num_workers is not None else cfg.DATALOADER.NUM_WORKERS)
    loader = tud.DataLoader(ds, batch_sampler=bs, num_workers=workers, collate_fn=trivial_batch_collator,
                            worker_init_fn=_seed_worker if workers > 0 else None)
    return _TrainBatches(loader, post)


def _seed_worker(worker_id: int):
    """detectron2's worker_init_reset_seed: the host mapper draws from `random` and `numpy.random`."""
    import random

    import numpy as np
    s = torch.initial_seed() % 2 ** 31 + worker_id
    random.seed(s)
    np.random.seed(s)


def build_test_loader(dataset: Union[str, Sequence[dict]], mapper=None, *, cfg=None, batch_size: int = 1,
                      num_workers: int = 0, rank: Optional[int] = None, world: Optional[int] = None):
    """`dataset`: a registered name (DatasetCatalog) or a list of dataset dicts."""
    dicts: List[dict] = DatasetCatalog.get(dataset) if isinstance(dataset, str) else list(dataset)
    mapper = mapper if mapper is not None else CATSegTestDatasetMapper(cfg)
    ds = _MapDataset(dicts, mapper)
    sampler = InferenceSampler(len(ds), rank, world)
    bs = tud.BatchSampler(sampler, batch_size, drop_last=False)
    return tud.DataLoader(ds, batch_sampler=bs, num_workers=num_workers, collate_fn=trivial_batch_collator)
