"""Config surface of the reference (`add_cat_seg_config`, cat_seg/config.py:6-93, plus the
detectron2 defaults the eval path reads).

When detectron2 is installed its `CfgNode` / `get_cfg` are used unchanged, so the
reference's `train_net.py` / `eval.sh` overrides work as-is.  Without detectron2 a
small yacs-compatible `CfgNode` (attribute access, `merge_from_file` with `_BASE_`,
`merge_from_list`, `freeze`) stands in, so configs/*.yaml load identically.
"""
from __future__ import annotations

import ast
import copy
import os

import yaml

try:  # pragma: no cover - detectron2 is not in this image
    from detectron2.config import CfgNode as _D2CfgNode, get_cfg as _d2_get_cfg
    HAVE_D2 = True
except Exception:  # noqa: BLE001
    _D2CfgNode, _d2_get_cfg = None, None
    HAVE_D2 = False


def _decode(v):
    """yacs `_decode_cfg_value`: strings that are Python literals ("(384, 384)", "[1,1]", "True")
    become those values; anything else stays as given."""
    if isinstance(v, str):
        try:
            return ast.literal_eval(v)
        except (ValueError, SyntaxError):
            return v
    return v


class CfgNode(dict):
    """Minimal yacs.CfgNode: nested dict with attribute access."""

    def __init__(self, init=None):
        super().__init__()
        for k, v in (init or {}).items():
            self[k] = CfgNode(v) if isinstance(v, dict) and not isinstance(v, CfgNode) else v
        object.__setattr__(self, "_frozen", False)

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        if self._frozen:
            raise AttributeError("config is frozen")
        self[k] = v

    def freeze(self):
        object.__setattr__(self, "_frozen", True)
        for v in self.values():
            if isinstance(v, CfgNode):
                v.freeze()

    def defrost(self):
        object.__setattr__(self, "_frozen", False)
        for v in self.values():
            if isinstance(v, CfgNode):
                v.defrost()

    def clone(self):
        return copy.deepcopy(self)

    def _merge(self, other: dict):
        for k, v in other.items():
            if isinstance(v, dict):
                node = self.get(k)
                if not isinstance(node, CfgNode):
                    node = CfgNode()
                    self[k] = node
                node._merge(v)
            else:
                v = _decode(v)
                self[k] = tuple(v) if isinstance(self.get(k), tuple) and isinstance(v, list) else v

    def merge_from_file(self, path: str):
        with open(path) as f:
            d = yaml.safe_load(f) or {}
        base = d.pop("_BASE_", None)
        if base is not None:
            self.merge_from_file(base if os.path.isabs(base) else os.path.join(os.path.dirname(path), base))
        self._merge(d)

    def merge_from_list(self, opts):
        assert len(opts) % 2 == 0, "KEY VALUE pairs expected"
        for k, v in zip(opts[0::2], opts[1::2]):
            node = self
            parts = k.split(".")
            for p in parts[:-1]:
                node = node[p]
            node[parts[-1]] = _decode(v)


def get_cfg():
    """detectron2's get_cfg (subset read by the CAT-Seg eval path when detectron2 is absent)."""
    if HAVE_D2:  # pragma: no cover
        return _d2_get_cfg()
    return CfgNode({
        "MODEL": {"META_ARCHITECTURE": "CATSeg", "DEVICE": "cuda", "WEIGHTS": "",
                  "PIXEL_MEAN": [103.530, 116.280, 123.675], "PIXEL_STD": [1.0, 1.0, 1.0],
                  "SEM_SEG_HEAD": {"NAME": "CATSegHead", "IGNORE_VALUE": 255, "NUM_CLASSES": 54,
                                   "IN_FEATURES": ["res2", "res3", "res4", "res5"]}},
        # detectron2 v0.6 defaults (config/defaults.py) of the keys the data / eval path reads;
        # MIN/MAX_SIZE_TEST are the CAT-Seg configs' values (configs/config.yaml:52-53)
        "INPUT": {"MIN_SIZE_TRAIN": (800,), "MIN_SIZE_TRAIN_SAMPLING": "choice", "MAX_SIZE_TRAIN": 1333,
                  "MIN_SIZE_TEST": 640, "MAX_SIZE_TEST": 2560, "FORMAT": "RGB",
                  "CROP": {"ENABLED": False, "TYPE": "relative_range", "SIZE": [0.9, 0.9]}},
        "DATASETS": {"TRAIN": (), "TEST": ()},
        "SOLVER": {"IMS_PER_BATCH": 16, "BASE_LR": 0.001, "WEIGHT_DECAY": 0.0001, "WEIGHT_DECAY_NORM": 0.0,
                   "MOMENTUM": 0.9, "MAX_ITER": 40000,
                   "CLIP_GRADIENTS": {"ENABLED": False, "CLIP_TYPE": "value", "CLIP_VALUE": 1.0, "NORM_TYPE": 2.0}},
        "TEST": {"EVAL_PERIOD": 0, "EXPECTED_RESULTS": [],
                 "AUG": {"ENABLED": False, "MIN_SIZES": (400, 500, 600, 700, 800, 900, 1000, 1100, 1200),
                         "MAX_SIZE": 4000, "FLIP": True}},
        "DATALOADER": {"NUM_WORKERS": 4},
        "OUTPUT_DIR": "./output",
        "VERSION": 2,
    })


def add_cat_seg_config(cfg):
    """Same keys and defaults as the reference add_cat_seg_config (cat_seg/config.py:6-93)."""
    C = type(cfg)
    cfg.INPUT.DATASET_MAPPER_NAME = "mask_former_semantic"
    cfg.DATASETS.VAL_ALL = ("coco_2017_val_all_stuff_sem_seg",)
    cfg.INPUT.COLOR_AUG_SSD = False
    cfg.INPUT.CROP.SINGLE_CATEGORY_MAX_AREA = 1.0
    cfg.INPUT.SIZE_DIVISIBILITY = -1
    cfg.SOLVER.WEIGHT_DECAY_EMBED = 0.0
    cfg.SOLVER.OPTIMIZER = "ADAMW"
    cfg.SOLVER.BACKBONE_MULTIPLIER = 0.1
    cfg.MODEL.MASK_FORMER = C()
    cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY = 32
    cfg.MODEL.SWIN = C()
    cfg.MODEL.SWIN.PRETRAIN_IMG_SIZE = 224
    cfg.MODEL.SWIN.PATCH_SIZE = 4
    cfg.MODEL.SWIN.EMBED_DIM = 96
    cfg.MODEL.SWIN.DEPTHS = [2, 2, 6, 2]
    cfg.MODEL.SWIN.NUM_HEADS = [3, 6, 12, 24]
    cfg.MODEL.SWIN.WINDOW_SIZE = 7
    cfg.MODEL.SWIN.MLP_RATIO = 4.0
    cfg.MODEL.SWIN.QKV_BIAS = True
    cfg.MODEL.SWIN.QK_SCALE = None
    cfg.MODEL.SWIN.DROP_RATE = 0.0
    cfg.MODEL.SWIN.ATTN_DROP_RATE = 0.0
    cfg.MODEL.SWIN.DROP_PATH_RATE = 0.3
    cfg.MODEL.SWIN.APE = False
    cfg.MODEL.SWIN.PATCH_NORM = True
    cfg.MODEL.SWIN.OUT_FEATURES = ["res2", "res3", "res4", "res5"]
    h = cfg.MODEL.SEM_SEG_HEAD
    h.TRAIN_CLASS_JSON = "datasets/ADE20K_2021_17_01/ADE20K_847.json"
    h.TEST_CLASS_JSON = "datasets/ADE20K_2021_17_01/ADE20K_847.json"
    h.TRAIN_CLASS_INDEXES = "datasets/coco/coco_stuff/split/seen_indexes.json"
    h.TEST_CLASS_INDEXES = "datasets/coco/coco_stuff/split/unseen_indexes.json"
    h.CLIP_PRETRAINED = "ViT-B/16"
    cfg.MODEL.PROMPT_ENSEMBLE = False
    cfg.MODEL.PROMPT_ENSEMBLE_TYPE = "single"
    cfg.MODEL.CLIP_PIXEL_MEAN = [122.7709383, 116.7460125, 104.09373615]
    cfg.MODEL.CLIP_PIXEL_STD = [68.5005327, 66.6321579, 70.3231630]
    h.TEXT_GUIDANCE_DIM = 512
    h.TEXT_GUIDANCE_PROJ_DIM = 128
    h.APPEARANCE_GUIDANCE_DIM = 512
    h.APPEARANCE_GUIDANCE_PROJ_DIM = 128
    h.DECODER_DIMS = [64, 32]
    h.DECODER_GUIDANCE_DIMS = [256, 128]
    h.DECODER_GUIDANCE_PROJ_DIMS = [32, 16]
    h.NUM_LAYERS = 4
    h.NUM_HEADS = 4
    h.HIDDEN_DIMS = 128
    h.POOLING_SIZES = [6, 6]
    h.FEATURE_RESOLUTION = [24, 24]
    h.WINDOW_SIZES = 12
    h.ATTENTION_TYPE = "linear"
    h.PROMPT_DEPTH = 0
    h.PROMPT_LENGTH = 0
    cfg.SOLVER.CLIP_MULTIPLIER = 0.01
    h.CLIP_FINETUNE = "attention"
    cfg.TEST.SLIDING_WINDOW = False
    # MI355X build extensions (absent from the reference; defaults keep reference behaviour)
    cfg.MODEL.CATSEG_HIP = C()
    cfg.MODEL.CATSEG_HIP.DTYPE = "bf16"          # "bf16" | "f32"
    cfg.MODEL.CATSEG_HIP.RETURN_ALL_IMAGES = True  # reference returns batched_inputs[0] only
    cfg.MODEL.CATSEG_HIP.BPE_VOCAB = ""          # path to CLIP's bpe_simple_vocab_16e6.txt.gz
    cfg.MODEL.CATSEG_HIP.SYNTHETIC_SEED = 0      # weights when MODEL.WEIGHTS is empty
    cfg.MODEL.CATSEG_HIP.VIT_FP8 = False         # config 5: e4m3 CLIP image-encoder GEMMs (bf16 engine)
    cfg.MODEL.CATSEG_HIP.GRAPH = True            # eval forward replayed from a hipGraph per input geometry
    # eval output: "probs" {"sem_seg": (T, H, W) fp32} | "labels" {"sem_seg_labels": (H, W) int32,
    # "sem_seg_score": (H, W) fp32} (the argmax map and its probability, without the volume)
    cfg.MODEL.CATSEG_HIP.OUTPUT = "probs"
    # SemanticSegmentorWithTTA: "host" merges the views' full-size probability volumes in torch (the
    # reference's merge; "probs" models only) | "device" merges the views' logits in one kernel
    # (catseg_postprocess_tta) and also serves "labels" models
    cfg.MODEL.CATSEG_HIP.TTA_MERGE = "host"
    # tiled inference at native resolution: every image cut into TILE x TILE windows STRIDE apart (the last
    # one of an axis shifted back to end at the border), each through the network as an image of its own,
    # the windows' probabilities averaged on the device (catseg_tiled_merge); the map is at input
    # resolution.  TILE a multiple of SIZE_DIVISIBILITY, TILE / 2 <= STRIDE <= TILE, BATCH tiles per launch
    cfg.MODEL.CATSEG_HIP.TILED = C()
    cfg.MODEL.CATSEG_HIP.TILED.ENABLED = False
    cfg.MODEL.CATSEG_HIP.TILED.TILE = 384
    cfg.MODEL.CATSEG_HIP.TILED.STRIDE = 256     # the reference's int(384 * (1 - 0.333))
    cfg.MODEL.CATSEG_HIP.TILED.BATCH = 8
    # the window over every tile in the merge ("uniform", or "pyramid": w(l) = min(l + 1, t' - l) per axis, no
    # step where a tile's cover begins or ends) and the reference's extra global view (the whole scene resized
    # to the tile's extent, averaged with the tiles' merge); catseg_tiled_blend
    cfg.MODEL.CATSEG_HIP.TILED.WINDOW = "uniform"
    cfg.MODEL.CATSEG_HIP.TILED.GLOBAL = False
    # build_train_loader: "host" = workers run MaskFormerSemanticDatasetMapper (PIL / numpy) | "device" =
    # workers only decode and the batch is resized, cropped, colour-augmented, flipped and padded by one fused
    # kernel (catseg_train_augment), byte for byte the host composition of the same draws
    cfg.MODEL.CATSEG_HIP.TRAIN_INPUT = "host"
    # OUTPUT "labels" only: every returned label map is turned into objects on the device (ops.label_regions /
    # ops.sieve_labels): MIN_AREA > 1 replaces "sem_seg_labels" by its sieve (regions smaller than MIN_AREA pixels
    # take the label of their largest large neighbour), then "sem_seg_regions" ((H, W) int32 region numbers) and
    # "regions_info" (label, area, bbox, first, score per region) describe the returned map.  CONNECTIVITY 4 | 8
    cfg.MODEL.CATSEG_HIP.REGIONS = C()
    cfg.MODEL.CATSEG_HIP.REGIONS.ENABLED = False
    cfg.MODEL.CATSEG_HIP.REGIONS.CONNECTIVITY = 8
    cfg.MODEL.CATSEG_HIP.REGIONS.MIN_AREA = 0
    # REGIONS.ENABLED only: "regions_outlines" = ops.region_outlines of "sem_seg_regions" under CONNECTIVITY, the
    # regions' boundaries as polygon rings on the device (cat_seg.vectorize turns them into GeoJSON)
    cfg.MODEL.CATSEG_HIP.REGIONS.OUTLINES = False
    # REGIONS.OUTLINES only: "regions_outlines_simplified" = ops.simplify_outlines of "regions_outlines", Douglas-
    # Peucker with TOLERANCE (pixels, 0 .. 16384) on the device, arc by arc, so neighbours share their simplified
    # boundary; "regions_outlines" stays as it is
    cfg.MODEL.CATSEG_HIP.REGIONS.SIMPLIFY = C()
    cfg.MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.ENABLED = False
    cfg.MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.TOLERANCE = 1.0
    # OUTPUT "labels" only: every returned dict gains "sem_seg_render", its final label map as an RGB picture
    # ((ceil(h / FACTOR), ceil(w / FACTOR), 3) uint8 on the device; CATSeg.add_render, ops.render_labels): the palette
    # colours blended at ALPHA over the dict's own input image (GRAY: over its luma), label edges EDGE_PX (0 .. 8)
    # wide in white, reduced by FACTOR (1 .. 64; 8 makes a quicklook), SCORE_ALPHA fading the colours by
    # "sem_seg_score".  PALETTE: a catalog name whose stuff_colors to use; "" = the PASCAL VOC colour map over the
    # test classes
    cfg.MODEL.CATSEG_HIP.RENDER = C()
    cfg.MODEL.CATSEG_HIP.RENDER.ENABLED = False
    cfg.MODEL.CATSEG_HIP.RENDER.ALPHA = 0.5
    cfg.MODEL.CATSEG_HIP.RENDER.GRAY = True
    cfg.MODEL.CATSEG_HIP.RENDER.EDGE_PX = 1
    cfg.MODEL.CATSEG_HIP.RENDER.FACTOR = 1
    cfg.MODEL.CATSEG_HIP.RENDER.SCORE_ALPHA = False
    cfg.MODEL.CATSEG_HIP.RENDER.PALETTE = ""
    # OUTPUT "labels" only (plain and sliding branch): the maps are made by catseg_postprocess_topk and every
    # returned dict gains "sem_seg_topk_labels" / "sem_seg_topk_score" ((TOPK, H, W): the TOPK best classes of a
    # pixel and their values, rank 0 first) and "sem_seg_mass" ((H, W): the sum of the class values).
    # "sem_seg_labels" is rank 0 with REJECT_LABEL where its score is below MIN_SCORE or, TOPK >= 2, leads rank 1
    # by less than MIN_MARGIN; with both 0.0 nothing is rejected.  REJECT_LABEL -1 = the number of test classes,
    # the row the evaluators' confusion matrix accepts as a prediction.  TOPK 1 .. 4
    cfg.MODEL.CATSEG_HIP.CONFIDENCE = C()
    cfg.MODEL.CATSEG_HIP.CONFIDENCE.ENABLED = False
    cfg.MODEL.CATSEG_HIP.CONFIDENCE.TOPK = 2
    cfg.MODEL.CATSEG_HIP.CONFIDENCE.MIN_SCORE = 0.0
    cfg.MODEL.CATSEG_HIP.CONFIDENCE.MIN_MARGIN = 0.0
    cfg.MODEL.CATSEG_HIP.CONFIDENCE.REJECT_LABEL = -1
    # OUTPUT "labels" only, every branch: "sem_seg_labels" is replaced by its majority filter (CATSeg.add_smooth,
    # ops.mode_filter) before the sieve, the regions, the picture and the evaluators see it: every pixel takes the
    # label with the most votes in its SIZE x SIZE window (odd, 3 .. 15, clipped to the map), ties to its own label,
    # then to the smallest; ITERATIONS 1 .. 8 passes.  RULE "plurality" | "half" (write the winner only where it
    # holds more than half of the window's votes).  WEIGHT "count" (one vote per pixel) | "score" (the pixel votes
    # with "sem_seg_score" in Q16).  The reject label of CONFIDENCE casts no votes; REJECT "keep" leaves rejected
    # pixels rejected, "fill" gives them their window's winner
    cfg.MODEL.CATSEG_HIP.SMOOTH = C()
    cfg.MODEL.CATSEG_HIP.SMOOTH.ENABLED = False
    cfg.MODEL.CATSEG_HIP.SMOOTH.SIZE = 3
    cfg.MODEL.CATSEG_HIP.SMOOTH.ITERATIONS = 1
    cfg.MODEL.CATSEG_HIP.SMOOTH.RULE = "plurality"
    cfg.MODEL.CATSEG_HIP.SMOOTH.WEIGHT = "count"
    cfg.MODEL.CATSEG_HIP.SMOOTH.REJECT = "keep"
    # OUTPUT "labels" only: every returned dict gains "sem_seg_overviews", {factor: ops.mode_overview of the final
    # label map}: the map reduced by each factor (distinct ints in 2 .. 32), a cell taking its most frequent label
    # (gdal's -r mode), with the winner's votes, the cell's total and their share.  WEIGHT as for SMOOTH
    cfg.MODEL.CATSEG_HIP.OVERVIEW = C()
    cfg.MODEL.CATSEG_HIP.OVERVIEW.FACTORS = ()
    cfg.MODEL.CATSEG_HIP.OVERVIEW.WEIGHT = "count"
    return cfg
