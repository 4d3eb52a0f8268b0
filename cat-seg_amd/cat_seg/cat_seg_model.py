"""CATSeg meta-architecture — the drop-in boundary of the MI355X path (reference
cat_seg/cat_seg_model.py:18-229).

`@META_ARCH_REGISTRY.register() class CATSeg`, built by `build_model(cfg)` from the
same config keys, with `forward(batched_inputs: list[dict]) -> list[dict]`:
  input  {"image": (3, H, W) uint8/float 0-255 (CPU or device), optional "height", "width"}
  output {"sem_seg": (T, height, width) fp32 sigmoid probabilities on the model device}
         or, with MODEL.CATSEG_HIP.OUTPUT "labels", {"sem_seg_labels": (height, width) int32 argmax
         over the classes, "sem_seg_score": (height, width) fp32 its probability} from one fused
         kernel that never writes the (T, height, width) volume
The reference returns results for batched_inputs[0] only (cat_seg_model.py:227-229);
this boundary returns one result per input image by default
(MODEL.CATSEG_HIP.RETURN_ALL_IMAGES; set False for the reference's exact behaviour).
The output stage (CATSeg._finish) resizes a uniform batch (equal image sizes, equal output sizes) with one
launch, with MODEL.CATSEG_HIP.GRAPH on or off, and its results are views of that launch's tensor.
With MODEL.CATSEG_HIP.TILED.ENABLED an image of any size is segmented at its own resolution: cut into
tiles, each through the network as an image of its own, merged on the device (engine.forward_tiled).
With MODEL.CATSEG_HIP.REGIONS.ENABLED (OUTPUT "labels") every returned label map is sieved (MIN_AREA) and
described by "sem_seg_regions" + "regions_info" on the device (CATSeg.add_regions; ops.label_regions), with
REGIONS.OUTLINES by "regions_outlines", the regions' boundaries as polygon rings (ops.region_outlines), and with
REGIONS.SIMPLIFY.ENABLED by "regions_outlines_simplified", those rings simplified arc by arc (ops.simplify_outlines).
With MODEL.CATSEG_HIP.RENDER.ENABLED (OUTPUT "labels") every returned dict gains "sem_seg_render", the final label
map as an RGB picture over its own input image (CATSeg.add_render; ops.render_labels).
With MODEL.CATSEG_HIP.CONFIDENCE.ENABLED (OUTPUT "labels", plain and sliding branch) the maps come from
ops.postprocess_topk: every dict gains "sem_seg_topk_labels", "sem_seg_topk_score" ((TOPK, H, W)) and "sem_seg_mass",
and "sem_seg_labels" is rank 0 after the reject rule (MIN_SCORE, MIN_MARGIN, REJECT_LABEL).
With MODEL.CATSEG_HIP.SMOOTH.ENABLED (OUTPUT "labels", every branch) "sem_seg_labels" is replaced by its majority
filter (CATSeg.add_smooth; ops.mode_filter) before the sieve, the regions and the picture see it, and with
MODEL.CATSEG_HIP.OVERVIEW.FACTORS every dict gains "sem_seg_overviews", {factor: ops.mode_overview of the final map}.

Everything between the input copy and the returned tensors runs in the HIP kernels of
libcatseg_hip.so through `CatSegEngine`; there is no CPU or PyTorch-op fallback.
Parameters live under the reference checkpoint keys (`state_dict()` /
`load_state_dict()`, detectron2 `{"model": ...}` files accepted), synthesized
deterministically when no checkpoint is given.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Iterable, List, Optional, Tuple

import torch
from torch import nn
from torch.nn.modules.module import _IncompatibleKeys

from . import custom_ops, ops, tiling
from .arch import CatSegArch, arch_from_cfg
from .engine import CatSegEngine
from .modeling.heads.cat_seg_head import CATSegHead  # noqa: F401  (registers the head)
from .params import apply_clip_finetune, attach_parameters
from .registry import META_ARCH_REGISTRY, build_sem_seg_head, configurable
from .training import clip_image_train_forward, clip_text_train_forward, head_train_forward, vpt_strip_rows
from .weights import CLIP as CLIP_PREFIX, synthesize_state_dict

_DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32, "fp32": torch.float32}


def _weights_version(params: Iterable[nn.Parameter]) -> int:
    """Sum of the parameters' in-place version counters: an optimizer step or a copy_ bumps it."""
    return sum(p._version for p in params)


def returned_inputs(batched_inputs: List[dict], return_all_images: bool) -> List[dict]:
    """The inputs that get a result: every one, or the first alone as the reference does."""
    return batched_inputs if return_all_images else batched_inputs[:1]


def output_plan(batched_inputs: List[dict], sizes, logits_hw, return_all_images: bool):
    """What the output stage does per returned image, [((h, w), (crop_h, crop_w))]: the result's size (a dict's
    "height" / "width", each defaulting to the image's own) and the region of the image's logits that the
    resize reads (sem_seg_postprocess's crop to the image, at the logits' resolution).  `sizes`: the (h, w)
    of every image; `logits_hw`: the logits' resolution.  Python ints in and out, so dynamo traces through it."""
    h_l, w_l = logits_hw
    return [((int(x.get("height", ih)), int(x.get("width", iw))), (min(h_l, ih), min(w_l, iw)))
            for x, (ih, iw) in zip(returned_inputs(batched_inputs, return_all_images), sizes)]


def convert_openai_clip_keys(sd: Dict[str, torch.Tensor], prefix: str = "") -> Dict[str, torch.Tensor]:
    """OpenAI CLIP `attn.in_proj_weight` -> q/k/v_proj_weight split (model_vpt.py:520-528), the
    metadata entries input_resolution / context_length / vocab_size dropped (:511-512), every
    key prefixed with `prefix`."""
    out = {}
    for k, v in sd.items():
        if k.endswith("attn.in_proj_weight"):
            q, kk, vv = v.chunk(3, dim=0)
            out[prefix + k.replace("in_proj", "q_proj")] = q
            out[prefix + k.replace("in_proj", "k_proj")] = kk
            out[prefix + k.replace("in_proj", "v_proj")] = vv
        elif k not in ("input_resolution", "context_length", "vocab_size"):
            out[prefix + k] = v
    return out


@META_ARCH_REGISTRY.register()
class CATSeg(nn.Module):
    @configurable
    def __init__(self, *, backbone, sem_seg_head: nn.Module, size_divisibility: int, pixel_mean: Tuple[float],
                 pixel_std: Tuple[float], clip_pixel_mean: Tuple[float], clip_pixel_std: Tuple[float],
                 train_class_json: str, test_class_json: str, sliding_window: bool, clip_finetune: str,
                 backbone_multiplier: float, clip_pretrained: str, arch: Optional[CatSegArch] = None,
                 dtype: str = "bf16", return_all_images: bool = True, synthetic_seed: int = 0,
                 vit_fp8: bool = False, graph: bool = True, output: str = "probs", tiled: bool = False,
                 tiled_tile: int = 384, tiled_stride: int = 256, tiled_batch: int = 8, tta_merge: str = "host",
                 tiled_window: str = "uniform", tiled_global: bool = False, regions: bool = False,
                 regions_connectivity: int = 8, regions_min_area: int = 0, regions_outlines: bool = False,
                 regions_simplify: bool = False, regions_simplify_tolerance: float = 1.0, render: bool = False,
                 render_alpha: float = 0.5, render_gray: bool = True, render_edge_px: int = 1, render_factor: int = 1,
                 render_score_alpha: bool = False, render_palette: str = "", confidence: bool = False,
                 confidence_topk: int = 2, confidence_min_score: float = 0.0, confidence_min_margin: float = 0.0,
                 confidence_reject_label: int = -1, smooth: bool = False, smooth_size: int = 3,
                 smooth_iterations: int = 1, smooth_rule: str = "plurality", smooth_weight: str = "count",
                 smooth_reject: str = "keep", overview_factors: Tuple[int, ...] = (), overview_weight: str = "count"):
        super().__init__()
        if output not in ("probs", "labels"):
            raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.OUTPUT must be 'probs' or 'labels', got {output!r}")
        # connected regions / sieve of the returned label maps (MODEL.CATSEG_HIP.REGIONS; ops.label_regions)
        self.regions = bool(regions)
        self.regions_connectivity, self.regions_min_area = int(regions_connectivity), int(regions_min_area)
        if self.regions and output != "labels":
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.REGIONS post-processes the label map of "
                             f"MODEL.CATSEG_HIP.OUTPUT 'labels', not {output!r}")
        if self.regions_connectivity not in (4, 8):
            raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.REGIONS.CONNECTIVITY must be 4 or 8, got {regions_connectivity!r}")
        if self.regions_min_area < 0:
            raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.REGIONS.MIN_AREA must be >= 0, got {regions_min_area!r}")
        # the regions' boundaries as polygon rings (MODEL.CATSEG_HIP.REGIONS.OUTLINES; ops.region_outlines)
        self.regions_outlines = bool(regions_outlines)
        if self.regions_outlines and not self.regions:
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.REGIONS.OUTLINES traces the regions of "
                             "MODEL.CATSEG_HIP.REGIONS.ENABLED, which is off")
        # the outlines simplified arc by arc (MODEL.CATSEG_HIP.REGIONS.SIMPLIFY; ops.simplify_outlines)
        self.regions_simplify = bool(regions_simplify)
        self.regions_simplify_tolerance = float(regions_simplify_tolerance)
        if self.regions_simplify and not self.regions_outlines:
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.ENABLED simplifies the rings of "
                             "MODEL.CATSEG_HIP.REGIONS.OUTLINES, which is off")
        if self.regions_simplify and not 0.0 <= self.regions_simplify_tolerance <= ops.SIMPLIFY_MAX_SIDE:
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.TOLERANCE must be in "
                             f"[0, {ops.SIMPLIFY_MAX_SIDE}] pixels, got {regions_simplify_tolerance!r}")
        # the returned label map as an RGB picture (MODEL.CATSEG_HIP.RENDER; ops.render_labels)
        self.render = bool(render)
        self.render_alpha, self.render_gray = float(render_alpha), bool(render_gray)
        self.render_edge_px, self.render_factor = int(render_edge_px), int(render_factor)
        self.render_score_alpha, self.render_palette = bool(render_score_alpha), str(render_palette)
        self._render_palettes: Dict[tuple, torch.Tensor] = {}
        if self.render and output != "labels":
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.RENDER draws the label map of "
                             f"MODEL.CATSEG_HIP.OUTPUT 'labels', not {output!r}")
        if self.render and not (0.0 <= self.render_alpha <= 1.0 and 0 <= self.render_edge_px <= 8
                                and 1 <= self.render_factor <= 64):
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.RENDER needs ALPHA in [0, 1], EDGE_PX in 0 .. 8 and FACTOR in "
                             f"1 .. 64, got {render_alpha!r}, {render_edge_px!r}, {render_factor!r}")
        # top-k maps, class mass and the reject rule (MODEL.CATSEG_HIP.CONFIDENCE; ops.postprocess_topk)
        self.confidence = bool(confidence)
        self.confidence_topk, self.confidence_reject_label = int(confidence_topk), int(confidence_reject_label)
        self.confidence_min_score, self.confidence_min_margin = float(confidence_min_score), float(confidence_min_margin)
        if self.confidence:
            if output != "labels":
                raise ValueError("CATSeg: MODEL.CATSEG_HIP.CONFIDENCE adds the top-k maps to the label map of "
                                 f"MODEL.CATSEG_HIP.OUTPUT 'labels', not {output!r}")
            if not 1 <= self.confidence_topk <= 4:
                raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.CONFIDENCE.TOPK must be in 1 .. 4, got {confidence_topk!r}")
            if self.confidence_reject_label < -1:
                raise ValueError("CATSeg: MODEL.CATSEG_HIP.CONFIDENCE.REJECT_LABEL must be a label >= 0, or -1 for the "
                                 f"number of test classes, got {confidence_reject_label!r}")
            if tiled:
                raise ValueError("CATSeg: MODEL.CATSEG_HIP.CONFIDENCE does not serve MODEL.CATSEG_HIP.TILED: the tiled "
                                 "merge ranks averaged probabilities and keeps one class per pixel")
            if tta_merge == "device":
                raise ValueError("CATSeg: MODEL.CATSEG_HIP.CONFIDENCE does not serve MODEL.CATSEG_HIP.TTA_MERGE "
                                 "'device': the merge of the views ranks averaged probabilities and keeps one class "
                                 "per pixel")
        # majority filter of the returned label maps (MODEL.CATSEG_HIP.SMOOTH; ops.mode_filter)
        self.smooth = bool(smooth)
        self.smooth_size, self.smooth_iterations = int(smooth_size), int(smooth_iterations)
        self.smooth_rule, self.smooth_weight, self.smooth_reject = str(smooth_rule), str(smooth_weight), str(smooth_reject)
        if self.smooth and output != "labels":
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.SMOOTH filters the label map of "
                             f"MODEL.CATSEG_HIP.OUTPUT 'labels', not {output!r}")
        if self.smooth_size % 2 != 1 or not 3 <= self.smooth_size <= 15:
            raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.SMOOTH.SIZE must be odd, 3 .. 15, got {smooth_size!r}")
        if not 1 <= self.smooth_iterations <= 8:
            raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.SMOOTH.ITERATIONS must be in 1 .. 8, got {smooth_iterations!r}")
        if self.smooth_rule not in ("plurality", "half"):
            raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.SMOOTH.RULE must be 'plurality' or 'half', got {smooth_rule!r}")
        if self.smooth_weight not in ("count", "score"):
            raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.SMOOTH.WEIGHT must be 'count' or 'score', got {smooth_weight!r}")
        if self.smooth_reject not in ("keep", "fill"):
            raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.SMOOTH.REJECT must be 'keep' or 'fill', got {smooth_reject!r}")
        # mode-resampled overviews of the final label map (MODEL.CATSEG_HIP.OVERVIEW; ops.mode_overview)
        try:
            self.overview_factors = tuple(int(f) for f in overview_factors)
        except (TypeError, ValueError):
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.OVERVIEW.FACTORS must be a tuple of ints, got "
                             f"{overview_factors!r}") from None
        self.overview_weight = str(overview_weight)
        if self.overview_factors and output != "labels":
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.OVERVIEW reduces the label map of "
                             f"MODEL.CATSEG_HIP.OUTPUT 'labels', not {output!r}")
        if (any(not 2 <= f <= 32 for f in self.overview_factors)
                or len(set(self.overview_factors)) != len(self.overview_factors)):
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.OVERVIEW.FACTORS must be distinct ints in 2 .. 32, got "
                             f"{overview_factors!r}")
        if self.overview_weight not in ("count", "score"):
            raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.OVERVIEW.WEIGHT must be 'count' or 'score', got {overview_weight!r}")
        # tiled inference at native resolution (MODEL.CATSEG_HIP.TILED; cat_seg.tiling, engine.forward_tiled)
        self.tiled = bool(tiled)
        self.tiled_tile, self.tiled_stride, self.tiled_batch = int(tiled_tile), int(tiled_stride), int(tiled_batch)
        self.tiled_window, self.tiled_global = str(tiled_window), bool(tiled_global)
        tiling.check_window(self.tiled_window, self.tiled_tile)      # an unknown WINDOW; "pyramid" with TILE > 2048
        if self.tiled:
            if sliding_window:
                raise ValueError("CATSeg: MODEL.CATSEG_HIP.TILED and TEST.SLIDING_WINDOW are two ways to cut one image "
                                 "into windows: enable one of them")
            if tta_merge == "device":
                raise ValueError("CATSeg: MODEL.CATSEG_HIP.TILED has no single logits tensor per image, which "
                                 "MODEL.CATSEG_HIP.TTA_MERGE 'device' merges: use TTA_MERGE 'host'")
            tiling.check_tile_stride(self.tiled_tile, self.tiled_stride, max(int(size_divisibility), 1))
            if not 1 <= self.tiled_batch <= 32:
                raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.TILED.BATCH must be in [1, 32], got {tiled_batch}")
        self.output = output
        self.backbone = backbone
        self.sem_seg_head = sem_seg_head
        self.size_divisibility = size_divisibility
        self.register_buffer("pixel_mean", torch.Tensor(pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.Tensor(pixel_std).view(-1, 1, 1), False)
        self.register_buffer("clip_pixel_mean", torch.Tensor(clip_pixel_mean).view(-1, 1, 1), False)
        self.register_buffer("clip_pixel_std", torch.Tensor(clip_pixel_std).view(-1, 1, 1), False)
        self.train_class_json, self.test_class_json = train_class_json, test_class_json
        self.clip_finetune = clip_finetune
        self.sliding_window = sliding_window
        arch = arch or arch_from_cfg_defaults(clip_pretrained)
        # cat_seg_model.py:78 (384 for ViT-B/16, else 336); non-reference presets keep their own
        self.clip_resolution = ((384, 384) if clip_pretrained == "ViT-B/16" else
                                (336, 336) if clip_pretrained.startswith("ViT-") else (arch.clip_resolution,) * 2)
        self.arch = arch.replace(
            clip_resolution=self.clip_resolution[0], size_divisibility=size_divisibility,
            clip_pixel_mean=tuple(clip_pixel_mean), clip_pixel_std=tuple(clip_pixel_std))
        self.compute_dtype = _DTYPES[dtype]
        self.return_all_images = return_all_images
        self.vit_fp8 = bool(vit_fp8)
        # eval forward: host images through one reused pinned canvas, the network replayed from a
        # hipGraph captured per input geometry (MODEL.CATSEG_HIP.GRAPH)
        self.use_graph = bool(graph)
        self._stage: Dict[tuple, dict] = {}
        self._graphs: Dict[tuple, dict] = {}
        # the weights as real nn.Parameters under the reference's module names (cat_seg.params):
        # CLIP under sem_seg_head.predictor.clip_model, the Aggregator under .transformer, and the
        # guidance upsamplers (cat_seg_model.py:81-82); requires_grad per CLIP_FINETUNE (:57-75)
        sd = synthesize_state_dict(self.arch, seed=synthetic_seed)
        attach_parameters(self, sd)
        apply_clip_finetune(self.sem_seg_head.predictor.clip_model, clip_finetune)
        # the engines hold kernel-layout copies of the weights, keyed by the parameters' version counters
        self._engine: Optional[CatSegEngine] = None
        self._train_engine: Optional[CatSegEngine] = None
        self._engine_key = self._train_engine_key = None
        self.input_format = "RGB"          # read by SemanticSegmentorWithTTA / DefaultPredictor
        self._op_handle = custom_ops.register_model(self)   # catseg::head_logits (torch.compile path)

    @classmethod
    def from_config(cls, cfg):
        hip = cfg.MODEL.get("CATSEG_HIP", {}) if hasattr(cfg.MODEL, "get") else {}
        tiled = (hip.get("TILED", None) if hip else None) or {}
        regions = (hip.get("REGIONS", None) if hip else None) or {}
        render = (hip.get("RENDER", None) if hip else None) or {}
        confidence = (hip.get("CONFIDENCE", None) if hip else None) or {}
        smooth = (hip.get("SMOOTH", None) if hip else None) or {}
        overview = (hip.get("OVERVIEW", None) if hip else None) or {}
        return {
            "backbone": None,
            "sem_seg_head": build_sem_seg_head(cfg, None),
            "size_divisibility": cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY,
            "pixel_mean": cfg.MODEL.PIXEL_MEAN,
            "pixel_std": cfg.MODEL.PIXEL_STD,
            "clip_pixel_mean": cfg.MODEL.CLIP_PIXEL_MEAN,
            "clip_pixel_std": cfg.MODEL.CLIP_PIXEL_STD,
            "train_class_json": cfg.MODEL.SEM_SEG_HEAD.TRAIN_CLASS_JSON,
            "test_class_json": cfg.MODEL.SEM_SEG_HEAD.TEST_CLASS_JSON,
            "sliding_window": cfg.TEST.SLIDING_WINDOW,
            "clip_finetune": cfg.MODEL.SEM_SEG_HEAD.CLIP_FINETUNE,
            "backbone_multiplier": cfg.SOLVER.BACKBONE_MULTIPLIER,
            "clip_pretrained": cfg.MODEL.SEM_SEG_HEAD.CLIP_PRETRAINED,
            "arch": arch_from_cfg(cfg),
            "dtype": hip.get("DTYPE", "bf16") if hip else "bf16",
            "return_all_images": bool(hip.get("RETURN_ALL_IMAGES", True)) if hip else True,
            "synthetic_seed": int(hip.get("SYNTHETIC_SEED", 0)) if hip else 0,
            "vit_fp8": bool(hip.get("VIT_FP8", False)) if hip else False,
            "graph": bool(hip.get("GRAPH", True)) if hip else True,
            "output": str(hip.get("OUTPUT", "probs")) if hip else "probs",
            "tiled": bool(tiled.get("ENABLED", False)),
            "tiled_tile": int(tiled.get("TILE", 384)),
            "tiled_stride": int(tiled.get("STRIDE", 256)),
            "tiled_batch": int(tiled.get("BATCH", 8)),
            "tiled_window": str(tiled.get("WINDOW", "uniform")),
            "tiled_global": bool(tiled.get("GLOBAL", False)),
            "tta_merge": str(hip.get("TTA_MERGE", "host")) if hip else "host",
            "regions": bool(regions.get("ENABLED", False)),
            "regions_connectivity": int(regions.get("CONNECTIVITY", 8)),
            "regions_min_area": int(regions.get("MIN_AREA", 0)),
            "regions_outlines": bool(regions.get("OUTLINES", False)),
            "regions_simplify": bool((regions.get("SIMPLIFY", None) or {}).get("ENABLED", False)),
            "regions_simplify_tolerance": float((regions.get("SIMPLIFY", None) or {}).get("TOLERANCE", 1.0)),
            "render": bool(render.get("ENABLED", False)),
            "render_alpha": float(render.get("ALPHA", 0.5)),
            "render_gray": bool(render.get("GRAY", True)),
            "render_edge_px": int(render.get("EDGE_PX", 1)),
            "render_factor": int(render.get("FACTOR", 1)),
            "render_score_alpha": bool(render.get("SCORE_ALPHA", False)),
            "render_palette": str(render.get("PALETTE", "")),
            "confidence": bool(confidence.get("ENABLED", False)),
            "confidence_topk": int(confidence.get("TOPK", 2)),
            "confidence_min_score": float(confidence.get("MIN_SCORE", 0.0)),
            "confidence_min_margin": float(confidence.get("MIN_MARGIN", 0.0)),
            "confidence_reject_label": int(confidence.get("REJECT_LABEL", -1)),
            "smooth": bool(smooth.get("ENABLED", False)),
            "smooth_size": int(smooth.get("SIZE", 3)),
            "smooth_iterations": int(smooth.get("ITERATIONS", 1)),
            "smooth_rule": str(smooth.get("RULE", "plurality")),
            "smooth_weight": str(smooth.get("WEIGHT", "count")),
            "smooth_reject": str(smooth.get("REJECT", "keep")),
            "overview_factors": tuple(overview.get("FACTORS", ())),
            "overview_weight": str(overview.get("WEIGHT", "count")),
        }

    # ------------------------------------------------------------------ parameters
    @property
    def device(self):
        return self.pixel_mean.device

    @property
    def _sd(self) -> Dict[str, torch.Tensor]:
        """The weights by reference checkpoint key (detached views of the nn.Parameters)."""
        return OrderedDict((k, p.detach()) for k, p in self.named_parameters())

    def state_dict(self, *args, **kwargs):        # reference checkpoint keys
        return OrderedDict(self._sd)

    def load_state_dict(self, state_dict, strict: bool = True, **_):
        """Reference checkpoint keys (detectron2 `{"model": sd}` accepted, OpenAI `in_proj_weight`
        split).  Returns torch's `_IncompatibleKeys(missing_keys, unexpected_keys)` (lists), which
        fvcore's Checkpointer._load_model reads and edits (DetectionCheckpointer drops
        pixel_mean / pixel_std from missing_keys)."""
        sd = state_dict.get("model", state_dict)
        sd = {k: (v if torch.is_tensor(v) else torch.as_tensor(v)) for k, v in sd.items()}
        if any(k.endswith("attn.in_proj_weight") for k in sd):
            # an OpenAI CLIP state dict (clip.load -> build_model, model_vpt.py:515-531) has no
            # module prefix: its keys belong under sem_seg_head.predictor.clip_model.
            prefix = "" if any(k.startswith(CLIP_PREFIX) for k in sd) else CLIP_PREFIX
            sd = convert_openai_clip_keys(sd, prefix)
        params = dict(self.named_parameters())
        missing = [k for k in params if k not in sd]
        unexpected = [k for k in sd if k not in params]
        if strict and (missing or unexpected):
            raise KeyError(f"load_state_dict: missing {missing[:5]}... unexpected {unexpected[:5]}...")
        with torch.no_grad():
            for k, p in params.items():
                if k in sd:
                    if tuple(sd[k].shape) != tuple(p.shape):
                        raise ValueError(f"{k}: shape {tuple(sd[k].shape)} != {tuple(p.shape)}")
                    p.copy_(sd[k].to(p.device, p.dtype))
        self._engine = self._train_engine = None
        self._graphs.clear()
        return _IncompatibleKeys(list(missing), list(unexpected))

    def _engine_device(self) -> torch.device:
        """The CUDA device the engine runs on: the module's device when it is on the GPU,
        else the current CUDA device (the HIP path has no CPU fallback)."""
        d = self.device
        if d.type == "cuda":
            return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
        return torch.device("cuda", torch.cuda.current_device())

    @property
    def engine(self) -> CatSegEngine:
        """Built once per resolved device (weights converted / uploaded once), rebuilt only when
        the model moves to another GPU or new weights are loaded."""
        dev = self._engine_device()
        key = (dev, _weights_version(self.parameters()))
        if self._engine is None or self._engine_key != key:
            self._engine = CatSegEngine(self.arch, self._sd, dtype=self.compute_dtype, device=dev,
                                        vit_fp8=self.vit_fp8)
            self._engine_key = key
            self._graphs.clear()           # captured forwards point at the old engine's weights
            self.sem_seg_head.predictor.attach_engine(self._engine)
        return self._engine

    @property
    def train_engine(self) -> CatSegEngine:
        """fp32 engine for the training step's CLIP encoders (the reference trains in fp32).  With CLIP
        fine-tuning the autograd path reads the trained block weights (and the visual prompt tokens) from
        the parameters directly and uses the engine only for the frozen embeddings -- and, under
        CLIP_FINETUNE "prompt", for the wholly frozen text encoder -- so it is rebuilt when a frozen CLIP
        weight changed (a checkpoint load bumps its version), not after every optimizer step."""
        dev = self._engine_device()
        clip = self.sem_seg_head.predictor.clip_model
        trains = any(p.requires_grad for p in clip.parameters())
        key = (dev, _weights_version(p for p in clip.parameters() if not (trains and p.requires_grad)))
        if self._train_engine is None or self._train_engine_key != key:
            self._train_engine = CatSegEngine(self.arch, self._sd, dtype=torch.float32, device=dev)
            self._train_engine_key = key
        return self._train_engine

    # ------------------------------------------------------------------ forward
    def _batch(self, eng: CatSegEngine, images: List[torch.Tensor]):
        """Stage the images into one zero-padded fp32 canvas on the device (ImageList.from_tensors
        geometry, _canvas_geometry).  Host images go through one pinned canvas and one H2D copy;
        images already on the device are copied in place there."""
        H, W = self._canvas_geometry(images)
        dev = eng.device
        on_dev = all(i.is_cuda for i in images)
        raw = torch.zeros(len(images), 3, H, W, dtype=torch.float32, device=dev if on_dev else "cpu",
                          pin_memory=not on_dev)
        for k, im in enumerate(images):
            raw[k, :, : im.shape[-2], : im.shape[-1]].copy_(im)
        sizes = [[int(i.shape[-2]), int(i.shape[-1])] for i in images]
        sizes_dev = torch.tensor(sizes, dtype=torch.int32).to(dev, non_blocking=True)
        return (raw if on_dev else raw.to(dev, non_blocking=True)), sizes_dev, sizes

    def _labels(self, logits: torch.Tensor, hw, crop, images=None) -> List[dict]:
        """OUTPUT "labels": one catseg_postprocess_argmax launch for the images of `logits`, into fresh
        tensors; each image's result (_label_result) holds views of them.  `images`: the input images of
        `logits`, which MODEL.CATSEG_HIP.RENDER draws over."""
        n, dev = logits.shape[0], logits.device
        if self.confidence:
            maps = ops.postprocess_topk(logits, self.confidence_topk, crop=crop, out_hw=hw,
                                        reject=self.confidence_reject(logits.shape[1]))
            return [self._confidence_result(maps, i, None if images is None else images[i]) for i in range(n)]
        labels = torch.empty(n, hw[0], hw[1], device=dev, dtype=torch.int32)
        score = torch.empty(n, hw[0], hw[1], device=dev, dtype=torch.float32)
        ops.postprocess_argmax(logits, labels, score, crop=crop)
        return [self._label_result(labels[i], score[i], None if images is None else images[i]) for i in range(n)]

    def _label_result(self, labels: torch.Tensor, score: torch.Tensor, image=None) -> dict:
        """One image's OUTPUT "labels" result, whichever branch made the map: with its regions (add_regions) and,
        over `image`, its picture (add_render)."""
        return self.add_regions({"sem_seg_labels": labels, "sem_seg_score": score}, image)

    def confidence_reject(self, n_classes: int):
        """MODEL.CATSEG_HIP.CONFIDENCE's reject rule as ops.postprocess_topk takes it, (MIN_SCORE, MIN_MARGIN, label)
        with REJECT_LABEL -1 resolved to `n_classes`; None while both thresholds are 0 (nothing is rejected and the
        label map is rank 0 itself)."""
        if not self.confidence or (self.confidence_min_score <= 0.0 and self.confidence_min_margin <= 0.0):
            return None
        label = self.confidence_reject_label if self.confidence_reject_label >= 0 else int(n_classes)
        return self.confidence_min_score, self.confidence_min_margin, label

    def _confidence_result(self, maps: dict, i: int, image=None) -> dict:
        """Image i of ops.postprocess_topk's maps as one OUTPUT "labels" result: "sem_seg_labels" is rank 0 after
        the reject rule, "sem_seg_score" rank 0's score, and the top-k maps and the mass ride along through
        add_regions / add_render."""
        labels = maps["labels"][i] if "labels" in maps else maps["topk_labels"][i, 0]
        return self.add_regions({"sem_seg_labels": labels, "sem_seg_score": maps["topk_score"][i, 0],
                                 "sem_seg_topk_labels": maps["topk_labels"][i],
                                 "sem_seg_topk_score": maps["topk_score"][i], "sem_seg_mass": maps["mass"][i]}, image)

    def _palette(self, device) -> torch.Tensor:
        """The (P, 3) uint8 palette of MODEL.CATSEG_HIP.RENDER on `device`: RENDER.PALETTE's catalog colours, or
        the colour map over the test classes; made once per class count.  With MODEL.CATSEG_HIP.CONFIDENCE rejecting
        into a label beyond the test classes, black rows up to that label."""
        n = int(self.sem_seg_head.predictor.class_tokens("test").shape[0])
        key = (n, str(device))
        if key not in self._render_palettes:
            from .visualize import palette_for
            palette = palette_for(self.render_palette or None, n, device=device)
            reject = self.confidence_reject(n)
            if reject is not None and reject[2] >= palette.shape[0]:
                palette = torch.cat([palette, palette.new_zeros((reject[2] + 1 - palette.shape[0], 3))])
            self._render_palettes[key] = palette
        return self._render_palettes[key]

    def add_render(self, result: dict, image) -> dict:
        """MODEL.CATSEG_HIP.RENDER: one image's result with "sem_seg_render", (ceil(h / FACTOR), ceil(w / FACTOR), 3)
        uint8 on the device: ops.render_labels of the final "sem_seg_labels" (after the sieve of REGIONS.MIN_AREA)
        over `image`, the dict's own (3, H, W) input image, sampled to the map's size by the nearest pixel centre;
        ALPHA, GRAY, EDGE_PX and FACTOR as configured, SCORE_ALPHA fading the colours by "sem_seg_score".  A float
        image is clamped to 0 .. 255 and truncated to uint8.  One launch after the graph replay or the merge,
        outside any captured graph.  A no-op with RENDER.ENABLED False."""
        if not self.render:
            return result
        labels = result["sem_seg_labels"]
        if image is None:
            raise ValueError("CATSeg: MODEL.CATSEG_HIP.RENDER draws over the input image, which this call has none of")
        image = image.to(labels.device)
        if image.dtype != torch.uint8:
            image = image.clamp(0, 255).to(torch.uint8)
        picture = ops.render_labels(labels, self._palette(labels.device), image=image, gray=self.render_gray,
                                    alpha=self.render_alpha, edge_px=self.render_edge_px, factor=self.render_factor,
                                    score=result["sem_seg_score"] if self.render_score_alpha else None)
        return {**result, "sem_seg_render": picture}

    def _reject_label(self):
        """The label MODEL.CATSEG_HIP.CONFIDENCE's reject rule writes, or None while nothing is rejected."""
        if self.confidence_reject(0) is None:
            return None
        if self.confidence_reject_label >= 0:
            return self.confidence_reject_label
        return self.confidence_reject(int(self.sem_seg_head.predictor.class_tokens("test").shape[0]))[2]

    def add_smooth(self, result: dict) -> dict:
        """MODEL.CATSEG_HIP.SMOOTH: "sem_seg_labels" replaced by its majority filter (ops.mode_filter with SIZE,
        ITERATIONS and RULE; WEIGHT "score" votes with "sem_seg_score").  "sem_seg_score" and the top-k planes stay
        as they are, as with the sieve.  The reject label of MODEL.CATSEG_HIP.CONFIDENCE casts no votes: REJECT
        "keep" leaves rejected pixels rejected, "fill" lets their neighbourhood fill them.  ITERATIONS launches,
        no host synchronisation.  A no-op with SMOOTH.ENABLED False."""
        if not self.smooth:
            return result
        labels = ops.mode_filter(result["sem_seg_labels"], self.smooth_size, iterations=self.smooth_iterations,
                                 rule=self.smooth_rule,
                                 score=result["sem_seg_score"] if self.smooth_weight == "score" else None,
                                 novote_label=self._reject_label(), fill=self.smooth_reject == "fill")
        return {**result, "sem_seg_labels": labels}

    def add_overviews(self, result: dict) -> dict:
        """MODEL.CATSEG_HIP.OVERVIEW: "sem_seg_overviews" = {factor: ops.mode_overview of the final "sem_seg_labels"}
        (after SMOOTH and the sieve), every factor from the full-resolution map; WEIGHT "score" votes with
        "sem_seg_score"; the reject label of MODEL.CATSEG_HIP.CONFIDENCE casts no votes.  A no-op with FACTORS ()."""
        if not self.overview_factors:
            return result
        score = result["sem_seg_score"] if self.overview_weight == "score" else None
        novote = self._reject_label()
        return {**result, "sem_seg_overviews": {f: ops.mode_overview(result["sem_seg_labels"], f, score=score,
                                                                     novote_label=novote)
                                                for f in self.overview_factors}}

    def add_regions(self, result: dict, image=None) -> dict:
        """MODEL.CATSEG_HIP.REGIONS: one image's {"sem_seg_labels", "sem_seg_score"} turned into objects, after
        the graph replay or the merge and outside any captured graph (the table's size depends on the data: one
        4-byte read of R).  MIN_AREA > 1 replaces "sem_seg_labels" by its sieve ("sem_seg_score" stays as it is);
        "sem_seg_regions" (the region numbers) and "regions_info" (label, area, bbox, first, score = the mean
        of "sem_seg_score" over the region) describe the returned map.  With REGIONS.OUTLINES, "regions_outlines" =
        ops.region_outlines of "sem_seg_regions" (two more 4-byte reads: corners, rings): ring_value is a region
        number, every region has one exterior ring, and they come in region order.  With REGIONS.SIMPLIFY.ENABLED,
        "regions_outlines_simplified" = ops.simplify_outlines of those rings under SIMPLIFY.TOLERANCE (two more
        4-byte reads: nodes, kept vertices); "regions_outlines" stays as it is.  A no-op with REGIONS.ENABLED
        False.  The junction every branch that returns labels passes: with `image` the result goes on through
        add_render (MODEL.CATSEG_HIP.RENDER), drawn from the final map.  MODEL.CATSEG_HIP.SMOOTH filters the map
        first (add_smooth), and MODEL.CATSEG_HIP.OVERVIEW reduces the final one (add_overviews)."""
        result = self.add_smooth(result)
        if not self.regions:
            return self.add_render(self.add_overviews(result), image)
        labels, conn = result["sem_seg_labels"], self.regions_connectivity
        if self.regions_min_area > 1:
            labels = ops.sieve_labels(labels, self.regions_min_area, connectivity=conn)
        ids, table = ops.label_regions(labels, connectivity=conn, score=result["sem_seg_score"])
        table.pop("score_q16")
        out = {**result, "sem_seg_labels": labels, "sem_seg_regions": ids, "regions_info": table}
        if self.regions_outlines:
            out["regions_outlines"] = ops.region_outlines(ids, connectivity=conn)
            if self.regions_simplify:
                out["regions_outlines_simplified"] = ops.simplify_outlines(ids, out["regions_outlines"],
                                                                           self.regions_simplify_tolerance)
        return self.add_render(self.add_overviews(out), image)

    def _forward_traced(self, batched_inputs: List[dict]):
        """The eval forward as dynamo traces it (torch.compile): the canvas staging in torch ops, the
        network as the one registered operator catseg::head_logits (custom_ops), the resize through
        catseg::postprocess; same kernels and results as the eager branch below."""
        if self.regions:
            raise RuntimeError("CATSeg.forward with MODEL.CATSEG_HIP.REGIONS cannot be traced by torch.compile: the "
                               "region table's size depends on the data; call it eagerly")
        if self.smooth or self.overview_factors:
            raise RuntimeError("CATSeg.forward with MODEL.CATSEG_HIP.SMOOTH or MODEL.CATSEG_HIP.OVERVIEW cannot be "
                               "traced by torch.compile: the filter and the overviews are launches outside the "
                               "registered operators; call it eagerly")
        if self.render:
            raise RuntimeError("CATSeg.forward with MODEL.CATSEG_HIP.RENDER cannot be traced by torch.compile: the "
                               "picture is drawn by a launch outside the registered operators; call it eagerly")
        if self.confidence:
            raise RuntimeError("CATSeg.forward with MODEL.CATSEG_HIP.CONFIDENCE cannot be traced by torch.compile: "
                               "the traced forward returns the argmax map alone; call it eagerly (the operator "
                               "catseg::postprocess_topk itself traces)")
        handle = self._op_handle
        n_classes, res = custom_ops.head_meta(handle)
        images = [x["image"] for x in batched_inputs]
        H, W = self._canvas_geometry(images)
        dev = self._engine_device()
        raw = torch.zeros(len(images), 3, H, W, dtype=torch.float32, device=dev)
        for k, im in enumerate(images):
            raw[k, :, : im.shape[-2], : im.shape[-1]] = im.to(dev, torch.float32)
        sizes = [(int(i.shape[-2]), int(i.shape[-1])) for i in images]
        sizes_dev = torch.tensor(sizes, dtype=torch.int32, device=dev)
        logits = torch.ops.catseg.head_logits(raw, sizes_dev, handle, n_classes, res)
        results = []
        plan = output_plan(batched_inputs, sizes, (res, res), self.return_all_images)
        for i, ((h, w), (crop_h, crop_w)) in enumerate(plan):
            if self.output == "labels":
                lab, sc = torch.ops.catseg.postprocess_argmax(logits[i:i + 1], h, w, crop_h, crop_w, True)
                results.append(self._label_result(lab[0], sc[0]))
                continue
            out = torch.ops.catseg.postprocess(logits[i:i + 1], h, w, crop_h, crop_w)
            results.append({"sem_seg": out[0]})
        return results

    def _stage_canvas(self, eng: CatSegEngine, images: List[torch.Tensor], canvas: torch.Tensor) -> None:
        """Write the images into the zero-padded fp32 device canvas (ImageList.from_tensors geometry;
        the padding stays zero: every call of one geometry writes the same regions).  Host images go
        through pinned staging canvases of their own dtype (uint8 from detectron2's mappers: 4x fewer
        bytes than fp32), reused across calls in two slots; the H2D copy and the device-side dtype
        conversion run on the compute stream, and an event per slot keeps the host from rewriting a
        slot whose copy has not run yet (the host runs at most two calls ahead).  A separate copy
        stream ordered by events measured slower on the box (tools/probe_boundary.py: 10.20 vs 10.11
        ms per bs-8 call, 10.05 with the images already on the device): the cross-stream waits cost
        more than the ~0.1 ms copy they would hide."""
        if all(i.is_cuda for i in images):
            for k, im in enumerate(images):
                canvas[k, :, : im.shape[-2], : im.shape[-1]].copy_(im)
            return
        dt = images[0].dtype if all(i.dtype == images[0].dtype for i in images) else torch.float32
        key = (tuple(canvas.shape), dt, canvas.device)
        st = self._stage.get(key)
        if st is None:
            st = {"slots": [{"host": torch.zeros(canvas.shape, dtype=dt, pin_memory=True),
                             "dev": torch.zeros(canvas.shape, dtype=dt, device=canvas.device),
                             "done": None} for _ in range(2)],
                  "next": 0}
            self._stage[key] = st
        slot = st["slots"][st["next"]]
        st["next"] ^= 1
        if slot["done"] is not None:
            slot["done"].synchronize()         # this slot's previous H2D has read the pinned canvas
        host = slot["host"]
        for k, im in enumerate(images):
            host[k, :, : im.shape[-2], : im.shape[-1]].copy_(im)
        slot["dev"].copy_(host, non_blocking=True)
        canvas.copy_(slot["dev"])              # device-side dtype conversion
        slot["done"] = torch.cuda.Event()
        slot["done"].record(torch.cuda.current_stream(canvas.device))

    def _canvas_geometry(self, images: List[torch.Tensor]):
        """(H, W) of the batch's canvas: the batch maximum, rounded up to size_divisibility."""
        d = max(self.size_divisibility, 1)
        H = max(int(i.shape[-2]) for i in images)
        W = max(int(i.shape[-1]) for i in images)
        return -(-H // d) * d, -(-W // d) * d

    def _graph_logits(self, eng: CatSegEngine, batched_inputs: List[dict]):
        """One hipGraph replay per input geometry: the first call of a geometry captures
        engine.head_logits, every call stages its images into the captured canvas and replays.
        Returns (the captured logits buffer, valid until the next call; the image sizes)."""
        images = [x["image"] for x in batched_inputs]
        H, W = self._canvas_geometry(images)
        sizes = tuple((int(i.shape[-2]), int(i.shape[-1])) for i in images)
        key = (id(eng), id(eng._text), len(images), H, W, sizes)
        g = self._graphs.get(key)
        dev = eng.device
        if g is None:
            raw = torch.zeros(len(images), 3, H, W, dtype=torch.float32, device=dev)
            sizes_dev = torch.tensor(sizes, dtype=torch.int32, device=dev)
            stream = torch.cuda.Stream(device=dev)
            stream.wait_stream(torch.cuda.current_stream(dev))

            with torch.cuda.stream(stream):
                eng.head_logits(raw, sizes_dev)  # warm the allocator outside the capture
            torch.cuda.current_stream(dev).wait_stream(stream)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                logits = eng.head_logits(raw, sizes_dev)
            # the graph replays raw device pointers: hold every tensor it reads that was allocated
            # outside the capture (the canvas, the sizes), the engine and its class-set buffers (ids in
            # the key stay unique while referenced); keep the 4 newest geometries
            g = {"graph": graph, "raw": raw, "sizes": sizes_dev, "logits": logits, "refs": (eng, eng._text)}
            while len(self._graphs) >= 4:
                self._graphs.pop(next(iter(self._graphs)))
            self._graphs[key] = g
        self._stage_canvas(eng, images, g["raw"])
        g["graph"].replay()
        return g["logits"], sizes

    def _eval_engine(self) -> CatSegEngine:
        """The eval engine with the test class set's text embeddings set on it."""
        eng = self.engine
        self.sem_seg_head.predictor.get_text_embeds()
        return eng

    def _eval_logits(self, batched_inputs: List[dict]):
        """(logits, image sizes) of the whole batch: one hipGraph replay per input geometry under
        MODEL.CATSEG_HIP.GRAPH (what bench.py times; the captured buffer, valid until the next call),
        else eager launches on a fresh canvas."""
        eng = self._eval_engine()
        if self.use_graph:
            return self._graph_logits(eng, batched_inputs)
        raw, sizes_dev, sizes = self._batch(eng, [x["image"] for x in batched_inputs])
        return eng.head_logits(raw, sizes_dev), sizes

    def _finish(self, logits: torch.Tensor, sizes, plan, images=None) -> List[dict]:
        """The output stage of the graph and the eager branch: the resize of `logits` by output_plan's
        `plan` into FRESH tensors (on the graph branch it runs after the replay; the caller may keep the
        results across calls).  A batch of more than one image whose image sizes and output sizes are all
        equal takes one launch (the engine leg's form) and its results are views of that launch's tensor;
        any other batch takes one launch per image."""
        n = len(plan)
        uniform = n > 1 and all(p == plan[0] for p in plan) and all(s == sizes[0] for s in sizes[:n])
        results = []
        for lo, hi in [(0, n)] if uniform else [(i, i + 1) for i in range(n)]:
            part, (hw, crop) = logits[lo:hi], plan[lo]
            if self.output == "labels":
                results += self._labels(part, hw, crop, None if images is None else images[lo:hi])
                continue
            out = torch.empty(part.shape[0], part.shape[1], hw[0], hw[1], device=logits.device)
            ops.postprocess(part, out, crop=crop)
            results += [{"sem_seg": o} for o in out]
        return results

    def forward_logits(self, batched_inputs: List[dict]):
        """The eval forward without the resize: (logits, crops).  `logits` is fp32 (n, T, h, w) for ALL n
        images of the batch, whatever RETURN_ALL_IMAGES says; `crops[i] = (min(h, image_h), min(w, image_w))`
        is the region of image i's logits that the resize reads, as `forward` computes it.  Serves the
        eager and the hipGraph branch; on the graph branch `logits` is the captured buffer, valid until
        the next call of the model (copy what has to outlive it).  What the device-side merge of
        SemanticSegmentorWithTTA consumes (catseg_postprocess_tta)."""
        if self.training:
            raise RuntimeError("CATSeg.forward_logits is an eval entry point: call model.eval() first")
        if self.sliding_window:
            raise RuntimeError("CATSeg.forward_logits does not serve TEST.SLIDING_WINDOW: the sliding branch "
                               "merges its windows before the resize and has no single logits tensor")
        if self.tiled:
            raise RuntimeError("CATSeg.forward_logits does not serve MODEL.CATSEG_HIP.TILED: the tiled branch "
                               "merges its tiles before the resize and has no single logits tensor")
        if torch.compiler.is_compiling():
            raise RuntimeError("CATSeg.forward_logits cannot be traced by torch.compile: call it eagerly")
        with torch.no_grad():
            logits, sizes = self._eval_logits(batched_inputs)
            return logits, [crop for _, crop in output_plan(batched_inputs, sizes, logits.shape[-2:], True)]

    def forward(self, batched_inputs: List[dict]):
        if self.training:
            return self._training_loss(batched_inputs)
        if self.sliding_window:
            return self._forward_sliding(batched_inputs)
        if self.tiled:
            return self._forward_tiled(batched_inputs)
        if torch.compiler.is_compiling():
            return self._forward_traced(batched_inputs)
        with torch.no_grad():
            logits, sizes = self._eval_logits(batched_inputs)
            plan = output_plan(batched_inputs, sizes, logits.shape[-2:], self.return_all_images)
            return self._finish(logits, sizes, plan, [x["image"] for x in batched_inputs])

    def _forward_tiled(self, batched_inputs: List[dict]):
        """MODEL.CATSEG_HIP.TILED eval: every image (or image 0 in the reference mode) at its own resolution
        through CatSegEngine.forward_tiled; the map is at input resolution, so a dict's height / width must
        be its image's size."""
        if torch.compiler.is_compiling():
            raise RuntimeError("CATSeg.forward with MODEL.CATSEG_HIP.TILED cannot be traced by torch.compile: the "
                               "tile grid follows each image's size; call it eagerly")
        with torch.no_grad():
            eng = self._eval_engine()
            results = []
            for x in returned_inputs(batched_inputs, self.return_all_images):
                im = x["image"]
                ih, iw = int(im.shape[-2]), int(im.shape[-1])
                if (int(x.get("height", ih)), int(x.get("width", iw))) != (ih, iw):
                    raise ValueError(f"CATSeg: MODEL.CATSEG_HIP.TILED returns the map at input resolution, but the "
                                     f"image is {ih} x {iw} and height / width ask for {x.get('height', ih)} x "
                                     f"{x.get('width', iw)}: set INPUT.MIN_SIZE_TEST 0 (CATSegTestDatasetMapper then "
                                     f"applies no resize)")
                img = im.to(eng.device, torch.float32).contiguous()
                out = eng.forward_tiled(img, self.output == "labels", tile=self.tiled_tile,
                                        stride=self.tiled_stride, batch=self.tiled_batch,
                                        window=self.tiled_window, global_view=self.tiled_global)
                if self.output == "labels":
                    results.append(self._label_result(*out, im))
                else:
                    results.append({"sem_seg": out})
            return results

    def _training_loss(self, batched_inputs: List[dict]):
        """The training branch (cat_seg_model.py:136-146,178-203): fp32 CLIP dense features + hooks and
        the training class set's text embeddings (re-encoded every step, cat_seg_predictor.py:190-224),
        the head with its HIP backward (cat_seg.training.head_train_forward), the logits upsampled to
        the targets' size and BCE-with-logits against one-hot targets (ops.BCEOneHotLoss).
        Returns {"loss_sem_seg": 0-d tensor}; `loss.backward()` fills `.grad` of every Aggregator and
        upsampler parameter and of the CLIP parameters CLIP_FINETUNE trains (cat_seg_model.py:57-75:
        'attention' = the q / v projections of both encoders' blocks, 'prompt' = the visual prompt tokens,
        'full' = every transformer parameter): an encoder with any of those runs as autograd Functions
        too (cat_seg.training.clip_*_train_forward), else without a graph on the engine."""
        if self.device.type != "cuda":
            raise RuntimeError("CATSeg training runs on the GPU: move the model there first (model.to('cuda'))")
        eng = self.train_engine
        pred = self.sem_seg_head.predictor
        params = dict(self.named_parameters())
        raw, sizes_dev, _ = self._batch(eng, [x["image"] for x in batched_inputs])
        # each encoder runs as autograd Functions only when one of ITS OWN parameters trains (CLIP_FINETUNE
        # "prompt" trains the visual prompt tokens alone: the text encoder is frozen, re-encoded every
        # step on the engine as the reference does, without a graph)
        vis = CLIP_PREFIX + "visual."
        clip_named = [(k, p) for k, p in params.items() if k.startswith(CLIP_PREFIX)]
        train_text = any(p.requires_grad for k, p in clip_named if not k.startswith(vis))
        train_image = any(p.requires_grad for k, p in clip_named if k.startswith(vis))
        if train_text:
            text = clip_text_train_forward(self.arch, params, eng, pred.class_tokens("train"))
        else:
            with torch.no_grad():
                text = eng.encode_text(pred.class_tokens("train"))
        if train_image:
            feats, hooks = clip_image_train_forward(self.arch, params, eng, raw, sizes_dev)
        else:
            with torch.no_grad():
                # the engine's rows carry the visual prompt rows (stride vision_seq_len): the head takes
                # them without, as every reference block drops them from its output
                feats, hooks = eng.encode_image(raw, sizes_dev)
                feats = vpt_strip_rows(self.arch, feats)
                hooks = [vpt_strip_rows(self.arch, h) for h in hooks]
        logits = head_train_forward(self.arch, params, feats, hooks, text)
        targets = torch.stack([x["sem_seg"].to(eng.device) for x in batched_inputs], dim=0)
        loss = ops.BCEOneHotLoss.apply(logits, targets, self.sem_seg_head.ignore_value)
        return {"loss_sem_seg": loss}

    def _forward_sliding(self, batched_inputs: List[dict]):
        """TEST.SLIDING_WINDOW eval (cat_seg_model.py:156-176,204-218): every image (or image 0 in
        the reference mode) through 4 Unfold tiles + 1 global crop; height/width default to 640."""
        with torch.no_grad():
            eng = self._eval_engine()
            inputs = returned_inputs(batched_inputs, self.return_all_images)
            raw, sizes_dev, _ = self._batch(eng, [x["image"] for x in inputs])
            res = eng.SLIDE_OUT
            out_hw = [(int(x.get("height", res)), int(x.get("width", res))) for x in inputs]
            if self.output == "labels" and self.confidence:
                n_classes = int(self.sem_seg_head.predictor.class_tokens("test").shape[0])
                return [self._confidence_result(maps, 0, x["image"]) for x, maps in
                        zip(inputs, eng.forward_sliding(raw, sizes_dev, out_hw, labels=True,
                                                        topk=(self.confidence_topk, self.confidence_reject(n_classes))))]
            if self.output == "labels":
                return [self._label_result(lab, sc, x["image"])
                        for x, (lab, sc) in zip(inputs, eng.forward_sliding(raw, sizes_dev, out_hw, labels=True))]
            return [{"sem_seg": o} for o in eng.forward_sliding(raw, sizes_dev, out_hw)]


def arch_from_cfg_defaults(clip_pretrained: str) -> CatSegArch:
    from .arch import PRESETS
    return PRESETS[clip_pretrained]
