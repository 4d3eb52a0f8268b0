"""CPU tests of the host side: config surface, registry/build_model, the C-ABI library
exports, loud failure without a GPU, the tokenizer and the weight synthesizer."""
import os
import re

import numpy as np
import pytest

from cat_seg.weights import CLIP
import torch

from cat_seg import CATSeg, add_cat_seg_config, build_model, get_cfg
from cat_seg import _lib as L
from cat_seg.arch import TINY, VIT_L14_336
from cat_seg.weights import synthesize_state_dict

from conftest import GOLDEN, ROOT

REF_VOCAB = "/root/reference/cat_seg/third_party/bpe_simple_vocab_16e6.txt.gz"


def tiny_cfg(**over):
    cfg = get_cfg()
    add_cat_seg_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "cat-seg_amd", "configs", "vitb_384.yaml"))
    cfg.merge_from_list(["MODEL.SEM_SEG_HEAD.POOLING_SIZES", "[1,1]", "MODEL.SEM_SEG_HEAD.CLIP_PRETRAINED", "tiny",
                         "MODEL.SEM_SEG_HEAD.TEXT_GUIDANCE_DIM", "96", "MODEL.SEM_SEG_HEAD.APPEARANCE_GUIDANCE_DIM",
                         "96", "MODEL.CATSEG_HIP.DTYPE", "f32"])
    for k, v in over.items():
        cfg.merge_from_list([k, v])
    return cfg


def test_config_base_and_overrides():
    cfg = tiny_cfg()
    assert cfg.MODEL.META_ARCHITECTURE == "CATSeg"
    assert list(cfg.MODEL.SEM_SEG_HEAD.POOLING_SIZES) == [1, 1]
    assert cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY == 32
    assert cfg.MODEL.CLIP_PIXEL_MEAN[0] == pytest.approx(122.7709383)
    assert cfg.TEST.SLIDING_WINDOW is False


def test_attention_type_config_key_reaches_the_arch():
    """MODEL.SEM_SEG_HEAD.ATTENTION_TYPE (config.py:86) selects AttentionLayer's attention
    (model.py:331-336): "linear" and "full" build; anything else fails as the reference does."""
    from cat_seg.arch import arch_from_cfg
    assert arch_from_cfg(tiny_cfg()).attention_type == "linear"
    cfg = tiny_cfg(**{"MODEL.SEM_SEG_HEAD.ATTENTION_TYPE": "full"})
    assert arch_from_cfg(cfg).attention_type == "full"
    assert build_model(cfg).sem_seg_head.predictor.attention_type == "full"
    with pytest.raises(NotImplementedError):
        build_model(tiny_cfg(**{"MODEL.SEM_SEG_HEAD.ATTENTION_TYPE": "softmax"}))


def test_prompt_ensemble_imagenet_refused_like_the_reference_fails():
    """PROMPT_ENSEMBLE_TYPE "imagenet" (cat_seg_predictor.py:80-83): the reference's eval text path
    raises in CLIP.encode_text on its (T, 80, 77) token stack (probe fixture made by running the
    reference's encode_text, tests/golden/make_golden.py ensemble); the build refuses it up front."""
    import json
    from conftest import GOLDEN
    rec = json.load(open(os.path.join(GOLDEN, "prompt_ensemble_probe.json")))
    assert rec["tokens_shape"][1] == 80 and rec["raised"] == "RuntimeError"
    for kind in ("imagenet", "imagenet_select"):
        with pytest.raises(NotImplementedError, match="encode_text"):
            build_model(tiny_cfg(**{"MODEL.PROMPT_ENSEMBLE_TYPE": kind}))


def test_visual_prompt_config_keys_reach_the_arch():
    """MODEL.SEM_SEG_HEAD.PROMPT_DEPTH / PROMPT_LENGTH (config.py:88-89, clip.load prompt args,
    model_vpt.py:243-265): the arch carries them, the synthesized state dict gets the reference's
    visual.transformer.prompt_tokens (depth, length, width) parameter, and CLIP_FINETUNE 'prompt'
    leaves exactly those trainable."""
    from cat_seg.arch import arch_from_cfg
    from cat_seg.weights import synthesize_state_dict
    cfg = tiny_cfg(**{"MODEL.SEM_SEG_HEAD.PROMPT_DEPTH": "4", "MODEL.SEM_SEG_HEAD.PROMPT_LENGTH": "3"})
    arch = arch_from_cfg(cfg)
    assert (arch.prompt_depth, arch.prompt_length, arch.vpt) == (4, 3, 3)
    assert arch_from_cfg(tiny_cfg()).vpt == 0
    sd = synthesize_state_dict(arch)
    assert sd[CLIP + "visual.transformer.prompt_tokens"].shape == (4, 3, arch.vision_width)
    m = build_model(cfg)
    assert m.sem_seg_head.predictor.prompt_length == 3


def test_vit_fp8_config_key_reaches_the_model():
    assert build_model(tiny_cfg()).vit_fp8 is False
    m = build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.DTYPE": "bf16", "MODEL.CATSEG_HIP.VIT_FP8": "True"}))
    assert m.vit_fp8 is True


def test_build_model_registry_and_state_dict_keys():
    m = build_model(tiny_cfg())
    assert isinstance(m, CATSeg)
    sd = m.state_dict()
    assert "sem_seg_head.predictor.clip_model.visual.transformer.resblocks.0.attn.q_proj_weight" in sd
    assert "sem_seg_head.predictor.transformer.layers.1.swin_block.block_2.attn.q.weight" in sd
    assert "upsample1.weight" in sd
    # round trip + OpenAI in_proj format accepted
    m.load_state_dict({"model": sd})
    with pytest.raises(KeyError):
        m.load_state_dict({"bogus": torch.zeros(1)})


def test_forward_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = build_model(tiny_cfg()).eval()
    with pytest.raises(RuntimeError):
        m([{"image": torch.zeros(3, 64, 64)}])


def test_output_plan_sizes_and_crops():
    """cat_seg_model.output_plan, the one statement of what the output stage does per image: how many results,
    each result's size ("height" / "width", each defaulting to the image's own) and the crop of the logits
    (here 96 x 96) that the resize reads."""
    from cat_seg.cat_seg_model import output_plan
    a, b, c = torch.zeros(3, 384, 384), torch.zeros(3, 300, 352), torch.zeros(3, 40, 48)

    def sizes(*ims):
        return [tuple(i.shape[-2:]) for i in ims]

    inputs = [{"image": a, "height": 200, "width": 300}, {"image": b}]
    assert output_plan(inputs, sizes(a, b), (96, 96), True) == [((200, 300), (96, 96)), ((300, 352), (96, 96))]
    # an image below the logits' resolution: the crop is the image's own size
    assert output_plan([{"image": c}], sizes(c), (96, 96), True) == [((40, 48), (40, 48))]
    # only "height" given: "width" is the image's own
    assert output_plan([{"image": b, "height": 200}], sizes(b), (96, 96), True) == [((200, 352), (96, 96))]
    assert output_plan([{"image": c, "width": 50}], sizes(c), (96, 96), True) == [((40, 50), (40, 48))]
    # the reference mode: one entry, for image 0
    assert output_plan(inputs, sizes(a, b), (96, 96), False) == [((200, 300), (96, 96))]
    # ints and tuples only (what lets dynamo trace through it), whatever the sizes came as
    plan = output_plan(inputs, [[384, 384], [300, 352]], torch.Size((96, 96)), True)
    assert plan == [((200, 300), (96, 96)), ((300, 352), (96, 96))]
    assert all(type(v) is int for hw, crop in plan for v in (*hw, *crop))


def test_capi_library_exports_every_header_symbol():
    hdr = open(os.path.join(ROOT, "include", "catseg_hip.h")).read()
    declared = set(re.findall(r"\b(catseg_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    assert declared <= set(L.EXPORTED)
    assert lib.catseg_abi_version() == 1
    # no A/B switches in the product ABI: they sit behind the diagnostics header only
    assert not any(s.startswith("catseg_set_") or "tuning" in s for s in declared)
    thdr = open(os.path.join(ROOT, "include", "catseg_hip_tuning.h")).read()
    tdecl = set(re.findall(r"\b(catseg_[a-z0-9_]+)\s*\(", thdr))
    assert tdecl == {"catseg_tuning_set", "catseg_tuning_get", "catseg_tuning_list"}
    assert all(hasattr(lib, s) for s in tdecl)
    knobs = L.tuning_knobs()
    assert "gemm_variant" in knobs and len(knobs) == len(set(knobs))
    L.tune("gemm_variant", 5)
    assert L.tuning("gemm_variant") == 5
    L.tune("gemm_variant", 0)
    with pytest.raises(RuntimeError):
        L.tune("no_such_knob", 1)
    assert lib.catseg_conv_tile_rows() == 128


def test_capi_argument_validation_without_gpu():
    """Host-side checks reject bad shapes before any launch (no GPU needed)."""
    a = L.GemmArgs()
    a.A, a.W, a.out = 16, 16, 16
    a.M, a.N, a.K = 8, 6, 8          # N % 4 != 0
    a.amap = L.IDENTITY
    lib = L.load()
    assert lib.catseg_gemm(a, None) == -1
    assert b"multiple of 4" in lib.catseg_last_error()


def test_weight_synthesizer_deterministic():
    a = synthesize_state_dict(TINY, seed=0)
    b = synthesize_state_dict(TINY, seed=0)
    c = synthesize_state_dict(TINY, seed=1)
    k = "sem_seg_head.predictor.transformer.conv1.weight"
    assert torch.equal(a[k], b[k]) and not torch.equal(a[k], c[k])
    # fingerprint pinned so the GPU box regenerates exactly the fixtures' weights
    assert abs(float(a[k].double().sum()) - float(np.load(os.path.join(GOLDEN, "synth_fingerprint.npy")))) < 1e-9


@pytest.mark.skipif(not os.path.exists(REF_VOCAB), reason="CLIP BPE vocabulary not present")
def test_tokenizer_matches_reference_token_ids():
    import json
    from cat_seg.tokenizer import BPETokenizer, class_prompts
    tok = BPETokenizer(REF_VOCAB)
    g = np.load(os.path.join(GOLDEN, "class_tokens.npz"))
    for ds in ("voc20", "ade150", "pc459", "ade847"):
        names = json.load(open(f"/root/reference/datasets/{ds}.json"))
        np.testing.assert_array_equal(tok.tokenize(class_prompts(names)), g[ds].astype(np.int64))


def test_bundled_tokens_for_reference_lists():
    from cat_seg.modeling.transformer.cat_seg_predictor import bundled_tokens
    assert bundled_tokens(["not", "a", "reference", "list"]) is None
    if os.path.exists("/root/reference/datasets/voc20.json"):
        import json
        names = json.load(open("/root/reference/datasets/voc20.json"))
        np.testing.assert_array_equal(bundled_tokens(names), np.load(os.path.join(GOLDEN, "class_tokens.npz"))["voc20"])
