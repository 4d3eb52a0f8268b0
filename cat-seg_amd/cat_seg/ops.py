"""Python mirror of the C ABI (include/catseg_hip.h): one thin wrapper per entry point.

Every wrapper takes device tensors, derives pointers / strides / dtypes, launches on
`torch.cuda.current_stream()` and raises RuntimeError on a non-zero status.  No
wrapper has a fallback: a missing library or device raises.
"""
from __future__ import annotations

from typing import Optional

import torch

import ctypes as C

from . import _lib as L
from ._lib import rowmap, IDENTITY


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# Optional launch recorder (bench.py's roofline pass): when a list, every wrapped launch
# appends {"kernel", "flops", "bytes", "start", "end"} with HIP events recorded on the
# launch stream around it.
PROFILE: Optional[list] = None


class _rec:
    """flops = the work the launch executes; ref_flops = the reference's count for the same module
    (class padding rows, guidance halves recomputed per class and the
    ConvTranspose maps are algorithmic work the build skips); defaults to flops."""

    def __init__(self, kernel, flops=0, nbytes=0, ref_flops=None, shape=None):
        self.kernel, self.flops, self.nbytes, self.shape = kernel, flops, nbytes, shape
        self.ref_flops = flops if ref_flops is None else ref_flops

    def __enter__(self):
        if PROFILE is not None:
            _ACTIVE[0] = True
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if PROFILE is not None:
            _ACTIVE[0] = False
            if exc[0] is None:
                self.e1.record(torch.cuda.current_stream())
                PROFILE.append({"kernel": self.kernel, "flops": self.flops, "ref_flops": self.ref_flops,
                                "bytes": self.nbytes, "start": self.e0, "end": self.e1, "shape": self.shape})
        return False


_ACTIVE = [False]


def call(name, *args):
    """Launch through the C ABI; under PROFILE, launches without their own record get one."""
    if PROFILE is None or _ACTIVE[0]:
        return L.call(name, *args)
    with _rec(name[len("catseg_"):]):
        return L.call(name, *args)


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return L.F32
    if t.dtype == torch.bfloat16:
        return L.BF16
    if t.dtype == torch.float8_e4m3fn:
        return L.FP8
    raise TypeError(f"unsupported dtype {t.dtype}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ld(t: torch.Tensor) -> int:
    assert t.dim() >= 2 and t.stride(-1) == 1, "row-major rows expected"
    return t.stride(-2)


def gemm(A, W, out, *, M=None, K=None, bias=None, act=L.ACT_NONE, alpha=1.0,
         add=None, addmap=None, add_ncols=None, res=None, res2=None, amap=None,
         lda=None, ldo=None, store=None):
    """out = act(A[amap(m)] . W^T + bias + add) * alpha + res + res2   (catseg_gemm)."""
    N = W.shape[0]
    K = K if K is not None else W.shape[1]
    M = M if M is not None else A.shape[0]
    a = L.GemmArgs()
    a.A, a.lda, a.amap = A.data_ptr(), lda if lda is not None else _ld(A), amap or IDENTITY
    a.W, a.ldw = W.data_ptr(), _ld(W)
    a.M, a.N, a.K = M, N, K
    a.bias = _p(bias)
    if add is not None:
        a.add, a.ld_add = add.data_ptr(), _ld(add)
        a.addmap = addmap or IDENTITY
        a.add_ncols = add_ncols if add_ncols is not None else N
    else:
        a.addmap = IDENTITY
    a.act, a.alpha = act, alpha
    if res is not None:
        a.res, a.ld_res = res.data_ptr(), _ld(res)
    if res2 is not None:
        a.res2, a.ld_res2 = res2.data_ptr(), _ld(res2)
    a.out = out.data_ptr()
    a.ldo = ldo if ldo is not None else (_ld(out) if store is None else 0)
    if store is not None:
        a.store_mode = 1
        a.cvt_k, a.cvt_hin, a.cvt_win, a.cvt_cout = store
    a.dtype_a, a.dtype_out = _dt(A), _dt(out)
    kname = "gemm_bf16" if a.dtype_a == L.BF16 else "gemm_f32"
    with _rec(kname, 2 * M * N * K, A.element_size() * (M * K + N * K) + out.element_size() * M * N,
              shape=(M, N, K)):
        call("catseg_gemm", a, _stream())
    return out


def quant_fp8_rows(x, q, scale, *, rows=None, cols=None):
    """Per-row e4m3 quantization (catseg_quant_fp8_rows): scale[r] = max|x[r]| / 448,
    q[r] = e4m3(x[r] / scale[r]).  q: torch.float8_e4m3fn, scale: fp32 [rows]."""
    rows = rows if rows is not None else x.shape[0]
    cols = cols if cols is not None else x.shape[1]
    with _rec("quant_fp8", 0, rows * cols * (x.element_size() + 1) + 4 * rows):
        call("catseg_quant_fp8_rows", x.data_ptr(), _dt(x), _ld(x), rows, cols, q.data_ptr(), _ld(q),
             scale.data_ptr(), _stream())
    return q, scale


def layernorm_fp8(x, gamma, beta, q, scale, *, rows=None, inmap=None, eps=1e-5):
    """LayerNorm straight to per-row e4m3 (catseg_layernorm_fp8)."""
    cols = gamma.shape[0]
    rows = rows if rows is not None else q.shape[0]
    with _rec("layernorm_fp8", 0, rows * cols * (x.element_size() + 1) + 4 * rows):
        call("catseg_layernorm_fp8", x.data_ptr(), _ld(x), inmap or IDENTITY, _dt(x), q.data_ptr(), _ld(q),
             scale.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rows, cols, eps, _stream())
    return q, scale


def gemm_fp8(A, sa, W, sw, out, *, bias=None, act=L.ACT_NONE, alpha=1.0, add=None, addmap=None,
             add_ncols=None, res=None, res2=None, amap=None, M=None):
    """out = epilogue((A8[amap(m)] . W8^T) * sa[amap(m)] * sw[n]) (catseg_gemm_fp8): the config-5 ViT GEMMs.
    A, W: torch.float8_e4m3fn rows; sa [M], sw [N] fp32 dequant scales."""
    N, K = W.shape
    M = M if M is not None else A.shape[0]
    a = L.GemmArgs()
    a.A, a.lda, a.amap = A.data_ptr(), _ld(A), amap or IDENTITY
    a.W, a.ldw = W.data_ptr(), _ld(W)
    a.M, a.N, a.K = M, N, K
    a.bias = _p(bias)
    if add is not None:
        a.add, a.ld_add = add.data_ptr(), _ld(add)
        a.addmap = addmap or IDENTITY
        a.add_ncols = add_ncols if add_ncols is not None else N
    else:
        a.addmap = IDENTITY
    a.act, a.alpha = act, alpha
    if res is not None:
        a.res, a.ld_res = res.data_ptr(), _ld(res)
    if res2 is not None:
        a.res2, a.ld_res2 = res2.data_ptr(), _ld(res2)
    a.out, a.ldo = out.data_ptr(), _ld(out)
    a.dtype_a, a.dtype_out = L.FP8, _dt(out)
    with _rec("gemm_fp8", 2 * M * N * K, M * K + N * K + out.element_size() * M * N):
        call("catseg_gemm_fp8", a, sa.data_ptr(), sw.data_ptr(), _stream())
    return out


def layernorm(x, gamma, beta, out, *, rows=None, inmap=None, eps=1e-5, cols=None):
    cols = cols if cols is not None else gamma.shape[0]
    rows = rows if rows is not None else out.shape[0]
    with _rec("layernorm", 0, rows * cols * (x.element_size() + out.element_size())):
      call("catseg_layernorm", x.data_ptr(), _ld(x), inmap or IDENTITY, _dt(x), out.data_ptr(), _ld(out), _dt(out),
         gamma.data_ptr(), beta.data_ptr(), rows, cols, eps, _stream())
    return out


def l2normalize(x, out, *, rows=None, cols=None, inmap=None, eps=1e-12):
    cols = cols if cols is not None else out.shape[-1]
    rows = rows if rows is not None else out.shape[0]
    with _rec("l2normalize", 0, rows * cols * (x.element_size() + out.element_size())):
        call("catseg_l2normalize", x.data_ptr(), _ld(x), inmap or IDENTITY, _dt(x), out.data_ptr(), _ld(out),
             _dt(out), rows, cols, eps, _stream())
    return out


def convert(x, out, *, rows=None, cols=None, inmap=None):
    cols = cols if cols is not None else out.shape[-1]
    rows = rows if rows is not None else out.shape[0]
    with _rec("convert", 0, rows * cols * (x.element_size() + out.element_size())):
        call("catseg_convert", x.data_ptr(), _ld(x), inmap or IDENTITY, _dt(x), out.data_ptr(), _ld(out), _dt(out),
             rows, cols, _stream())
    return out


def attention(q, k, v, out, *, n_seq, seq_len, n_heads, head_dim, scale, causal=False,
              mode=0, img_hw=(0, 0), window=0, shift=0):
    a = L.AttnArgs()
    a.q, a.k, a.v, a.ld_qkv = q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q)
    assert _ld(k) == a.ld_qkv and _ld(v) == a.ld_qkv
    a.out, a.ld_out = out.data_ptr(), _ld(out)
    a.n_seq, a.seq_len, a.n_heads, a.head_dim = n_seq, seq_len, n_heads, head_dim
    a.scale, a.causal = scale, int(causal)
    a.mode, a.img_h, a.img_w, a.window, a.shift = mode, img_hw[0], img_hw[1], window, shift
    a.dtype = _dt(q)
    # algorithmic bytes: q, k, v read once, the output written once
    nbytes = n_seq * seq_len * n_heads * head_dim * (3 * q.element_size() + out.element_size())
    with _rec("attention_window" if mode == 1 else "attention", 4 * n_seq * n_heads * seq_len * seq_len * head_dim,
              nbytes):
        call("catseg_attention", a, _stream())
    return out


def swin_window_attention(x, ln, w_qkv, b_qkv, gqk, gmap, out, *, S, img_hw, window, shift, n_heads, head_dim,
                          scale, eps=1e-5):
    """Fused norm1 + q/k/v (+ guidance half) + shifted-window attention (catseg_swin_window_attention)."""
    a = L.SwinAttnArgs()
    a.x, a.ld_x = x.data_ptr(), _ld(x)
    a.ln_g, a.ln_b, a.eps = ln[0].data_ptr(), ln[1].data_ptr(), eps
    a.w_qkv, a.b_qkv = w_qkv.data_ptr(), b_qkv.data_ptr()
    a.gqk, a.ld_g, a.gmap = gqk.data_ptr(), _ld(gqk), gmap
    a.out, a.ld_out = out.data_ptr(), _ld(out)
    a.S, a.img_h, a.img_w, a.window, a.shift = S, img_hw[0], img_hw[1], window, shift
    a.n_heads, a.head_dim, a.scale, a.dtype = n_heads, head_dim, scale, _dt(x)
    R = S * img_hw[0] * img_hw[1]
    C = n_heads * head_dim
    L_ = window * window
    flops = 2 * R * C * 3 * C + 4 * R * L_ * C
    ref = 2 * R * (2 * 2 * C * C + C * C) + 4 * R * L_ * C        # q, k = Linear(2C -> C) on [x | g] (model.py:94-96)
    with _rec("swin_window_attention", flops, x.element_size() * R * 2 * C, ref_flops=ref):
        call("catseg_swin_window_attention", a, _stream())
    return out


def class_attention(x, ln, w_qkv, b_qkv, tg, y, *, B, T, HW, n_heads, head_dim, tg_bstride=0, n_pad=0,
                    k_pad=None, v_pad=None, eps=1e-5, attn_eps=1e-6, tgk_t=None):
    """Fused norm1 + q/k/v (+ text-guidance half) + linear class attention + residual
    (catseg_class_attention): y = x + LinearAttention(...).  tgk_t: the transposed k half of tg
    (class_attention_kt), made here when not given."""
    if tgk_t is None:
        tgk_t = class_attention_kt(tg if tg_bstride == 0 else tg[:B * T], T, 1 if tg_bstride == 0 else B)
    a = L.ClassAttnArgs()
    a.x, a.ld_x = x.data_ptr(), _ld(x)
    a.ln_g, a.ln_b, a.eps = ln[0].data_ptr(), ln[1].data_ptr(), eps
    a.w_qkv, a.b_qkv = w_qkv.data_ptr(), b_qkv.data_ptr()
    a.tg, a.ld_tg, a.tg_bstride = tg.data_ptr(), _ld(tg), tg_bstride
    a.n_pad, a.k_pad, a.v_pad, a.attn_eps = n_pad, _p(k_pad), _p(v_pad), attn_eps
    a.y, a.ld_y = y.data_ptr(), _ld(y)
    a.B, a.T, a.HW, a.n_heads, a.head_dim, a.dtype = B, T, HW, n_heads, head_dim, _dt(x)
    a.tgk_t, a.ld_tgk_t = tgk_t.data_ptr(), tgk_t.shape[-1]
    a.tgk_t_bstride = tgk_t.shape[-2] * tgk_t.shape[-1] if tgk_t.shape[0] > 1 else 0
    R = B * T * HW
    C = n_heads * head_dim
    flops = 2 * R * C * 3 * C + 4 * R * n_heads * head_dim * head_dim
    Rp = B * HW * (T + n_pad)                 # the reference pads T to pad_len (model.py:397-409)
    ref = 2 * Rp * (2 * 2 * C * C + C * C) + 4 * Rp * n_heads * head_dim * head_dim
    with _rec("class_attention", flops, x.element_size() * R * 2 * C, ref_flops=ref):
        call("catseg_class_attention", a, _stream())
    return y


def linear_attention(q, k, v, x, y, *, B, T, HW, n_heads, head_dim, n_pad=0, k_pad=None, v_pad=None, eps=1e-6):
    a = L.LinAttnArgs()
    a.q, a.k, a.v, a.ld_qkv = q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q)
    a.x, a.y, a.ld_xy = x.data_ptr(), y.data_ptr(), _ld(x)
    assert _ld(y) == a.ld_xy
    a.B, a.T, a.HW, a.n_heads, a.head_dim = B, T, HW, n_heads, head_dim
    a.n_pad, a.k_pad, a.v_pad, a.eps = n_pad, _p(k_pad), _p(v_pad), eps
    a.dtype = _dt(q)
    with _rec("linear_attention", 4 * B * HW * T * n_heads * head_dim * head_dim):
        call("catseg_linear_attention", a, _stream())
    return y


def full_attention(qkv, x, y, *, B, T, HW, n_heads, head_dim, n_pad=0, k_pad=None, v_pad=None):
    """ATTENTION_TYPE "full" (FullAttention, model.py:300-320): y = x + softmax(q k^T / sqrt(d)) v over
    every pixel's T classes plus the n_pad learned padding tokens (model.py:397-410).
    qkv: class-major rows (b*T + t)*HW + p, [q | k | v].  catseg_class_seq_pack -> catseg_attention
    (mode 0, the MFMA flash kernel) -> catseg_class_seq_unpack_add."""
    C_ = n_heads * head_dim
    Lp = T + n_pad
    n_seq = B * HW
    packed = torch.empty(n_seq * Lp, 3 * C_, device=qkv.device, dtype=qkv.dtype)
    o = torch.empty(n_seq * Lp, C_, device=qkv.device, dtype=qkv.dtype)
    a = L.ClassSeqArgs()
    a.qkv, a.ld_qkv = qkv.data_ptr(), _ld(qkv)
    a.packed, a.ld_packed = packed.data_ptr(), _ld(packed)
    a.o, a.ld_o = o.data_ptr(), _ld(o)
    a.x, a.y, a.ld_xy = x.data_ptr(), y.data_ptr(), _ld(x)
    assert _ld(y) == a.ld_xy and x.dtype == y.dtype == qkv.dtype
    a.B, a.T, a.HW, a.C = B, T, HW, C_
    a.n_pad, a.k_pad, a.v_pad = n_pad, _p(k_pad), _p(v_pad)
    a.dtype = _dt(qkv)
    es = qkv.element_size()
    with _rec("class_seq_pack", 0, es * (B * T * HW + n_seq * Lp) * 3 * C_):
        call("catseg_class_seq_pack", a, _stream())
    attention(packed[:, :C_], packed[:, C_:2 * C_], packed[:, 2 * C_:], o, n_seq=n_seq, seq_len=Lp,
              n_heads=n_heads, head_dim=head_dim, scale=head_dim ** -0.5)
    with _rec("class_seq_unpack_add", 0, es * 3 * B * T * HW * C_):
        call("catseg_class_seq_unpack_add", a, _stream())
    return y


def _conv_args(src1, weight, out, S, H, W, c1, s1_slice_stride, s1_offset, src2, c2, s2_slice_stride, s2_offset,
               src2_div, bias, act, gn, stats, stats_cpg, addend, addend_div):
    a = L.ConvArgs()
    a.src1, a.s1_slice_stride, a.s1_offset, a.c1 = (src1.data_ptr(),
                                                   s1_slice_stride if s1_slice_stride is not None else H * W * c1,
                                                   s1_offset, c1)
    if src2 is not None:
        a.src2, a.s2_slice_stride, a.s2_offset, a.c2, a.src2_div = (src2.data_ptr(), s2_slice_stride or H * W * c2,
                                                                   s2_offset, c2, src2_div)
    else:
        a.src2_div = 1
    a.S, a.H, a.W = S, H, W
    a.weight, a.c_out = weight.data_ptr(), weight.shape[0]
    a.bias, a.act = _p(bias), act
    if gn is not None:
        mean, rstd, gamma, beta, cpg = gn
        a.gn_mean, a.gn_rstd, a.gn_gamma, a.gn_beta, a.gn_cpg = (mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                                 beta.data_ptr(), cpg)
    a.out = _p(out)
    a.stats, a.stats_cpg = _p(stats), stats_cpg
    a.dtype = _dt(out if out is not None else weight)
    if addend is not None:
        assert addend.dtype == torch.float32 and addend.is_contiguous()
        a.addend, a.addend_slice_stride, a.addend_div = addend.data_ptr(), H * W * weight.shape[0], addend_div
    return a


def _conv_bytes(src1, weight, out, S, HW, c1, src2, c2, src2_div, addend, addend_div, out_px=None, out_ch=None):
    """Algorithmic bytes of a 3x3 conv launch: each input pixel read once (the per-image src2 and
    addend once per image), each output pixel written once, the weights read once."""
    out_px = HW if out_px is None else out_px
    out_ch = weight.shape[0] if out_ch is None else out_ch
    n = S * HW * c1 * src1.element_size() + weight.numel() * weight.element_size()
    if src2 is not None:
        n += (S // max(src2_div, 1)) * HW * c2 * src2.element_size()
    if out is not None:
        n += S * out_px * out_ch * out.element_size()
    if addend is not None:
        n += (S // max(addend_div, 1)) * out_px * out_ch * 4
    return n


def conv3x3(src1, weight, out, *, S, H, W, c1, s1_slice_stride=None, s1_offset=0,
            src2=None, c2=0, s2_slice_stride=0, s2_offset=0, src2_div=1,
            bias=None, act=L.ACT_NONE, gn=None, stats=None, stats_cpg=16, addend=None, addend_div=1):
    """3x3 / pad-1 conv over NHWC (catseg_conv3x3).  `stats` receives GroupNorm partials per
    conv3x3_stats_tile(...) pixels (query it with the same arguments to size the buffer)."""
    a = _conv_args(src1, weight, out, S, H, W, c1, s1_slice_stride, s1_offset, src2, c2, s2_slice_stride, s2_offset,
                   src2_div, bias, act, gn, stats, stats_cpg, addend, addend_div)
    ws_bytes = L.load().catseg_conv3x3_workspace(C.byref(a))
    ws = None
    if ws_bytes > 0:   # split-K scratch of small-grid convs (caching allocator; graph-capturable)
        ws = torch.empty(ws_bytes // 4, device=out.device, dtype=torch.float32)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    with _rec("conv3x3", 2 * S * H * W * weight.shape[0] * weight.shape[1],
              _conv_bytes(src1, weight, out, S, H * W, c1, src2, c2, src2_div, addend, addend_div)):
        call("catseg_conv3x3", a, _stream())
    return out


def conv3x3_stats_tile(src1, weight, *, S, H, W, c1, s1_slice_stride=None, s1_offset=0,
                       src2=None, c2=0, s2_slice_stride=0, s2_offset=0, src2_div=1,
                       bias=None, act=L.ACT_NONE, gn=None, stats_cpg=16, addend=None, addend_div=1) -> int:
    """Pixels per GroupNorm partial of the conv kernel catseg_conv3x3 picks for these arguments."""
    a = _conv_args(src1, weight, None, S, H, W, c1, s1_slice_stride, s1_offset, src2, c2, s2_slice_stride, s2_offset,
                   src2_div, bias, act, gn, None, stats_cpg, addend, addend_div)
    a.stats = 1   # any non-null: the query only inspects whether statistics are requested
    return L.load().catseg_conv3x3_stats_tile(C.byref(a))


def conv3x3_partial(g, weight, out, *, B, H, W):
    """out[b][pix][co] = conv3x3 of g (NHWC [B][H][W][cin]) with fp32 weight [cout][9][cin], no bias:
    the per-image guidance half of a conv over [x | g] (catseg_conv3x3_partial)."""
    cout, k = weight.shape
    cin = k // 9
    assert g.shape[-1] == cin and out.dtype == torch.float32 and weight.dtype == torch.float32
    with _rec("conv3x3_partial", 2 * B * H * W * cout * k,
              B * H * W * (cin * g.element_size() + 4 * cout) + 4 * cout * k):
        call("catseg_conv3x3_partial", g.data_ptr(), B, H, W, cin, weight.data_ptr(), cout, out.data_ptr(), _dt(g),
             _stream())
    return out


def upconv3x3(src1, weight, out, *, S, H, W, c1, s1_slice_stride=None, gn=None, stats=None, stats_cpg=16,
              addend=None, addend_div=1, ref_convt_out=None, ref_guid=0):
    """ConvTranspose2d(k=2, s=2) + conv3x3 folded into one 4-parity conv over the ConvTranspose
    input (catseg_upconv3x3): src1 [S][H][W][c1] -> out [S][2H][2W][c_out/4] with the composite
    weight [4 * cout][9 * c1] (CatSegEngine._upconv_weights) and the parity-layout addend
    (upconv_addend).  `stats` receives [S][4 * H*W / upconv3x3_stats_tile()][cout/16][2]."""
    a = _conv_args(src1, weight, out, S, H, W, c1, s1_slice_stride, 0, None, 0, 0, 0, 1, None, L.ACT_NONE, gn,
                   stats, stats_cpg, addend, addend_div)
    cout = weight.shape[0] // 4
    # reference: ConvTranspose2d(c1 -> m, k=2, s=2) then conv3x3 over [up (m) | guidance (ref_guid)]
    m = ref_convt_out or 0
    ref = (2 * S * H * W * 4 * m * c1 + 2 * S * 4 * H * W * cout * 9 * (m + ref_guid)) if m else None
    nbytes = _conv_bytes(src1, weight, out, S, H * W, c1, None, 0, 1, addend, addend_div, out_px=4 * H * W,
                         out_ch=cout)
    with _rec("upconv3x3", 2 * S * H * W * weight.shape[0] * 4 * c1, nbytes, ref_flops=ref):
        call("catseg_upconv3x3", a, _stream())
    return out


def upconv3x3_stats_tile() -> int:
    return L.load().catseg_upconv3x3_stats_tile()


def upconv_addend(g, weight, tap_bias, out, *, B, H2, W2):
    """catseg_upconv_addend: the guidance half of the Up conv on the 2H x 2W grid (fp32 weight
    [cout][9 * cin]) + the ConvTranspose bias through the in-image taps (tap_bias [9][cout]), in
    the parity layout [B][H2/2 * W2/2][4 * cout] of upconv3x3's addend."""
    cout, k = weight.shape
    cin = k // 9
    assert g.shape[-1] == cin and out.dtype == torch.float32 and weight.dtype == torch.float32
    with _rec("conv3x3_partial", 2 * B * H2 * W2 * cout * k,
              B * H2 * W2 * (cin * g.element_size() + 4 * cout) + 4 * cout * k, ref_flops=0):   # in upconv3x3's reference count
        call("catseg_upconv_addend", g.data_ptr(), B, H2, W2, cin, weight.data_ptr(), _p(tap_bias), cout,
             out.data_ptr(), _dt(g), _stream())
    return out


def conv_tile_rows() -> int:
    return L.load().catseg_conv_tile_rows()


def groupnorm_stats(partials, S, tiles, groups, tile_count, mean, rstd, eps=1e-5):
    with _rec("groupnorm_stats", 0, 4 * (S * tiles * groups * 2 + 2 * S * groups)):
        call("catseg_groupnorm_stats", partials.data_ptr(), S, tiles, groups, tile_count, eps, mean.data_ptr(),
             rstd.data_ptr(), _stream())


def groupnorm_relu(x, y, *, S, HW, C, cpg, mean, rstd, gamma, beta):
    call("catseg_groupnorm_relu", x.data_ptr(), y.data_ptr(), S, HW, C, cpg, mean.data_ptr(), rstd.data_ptr(),
         gamma.data_ptr(), beta.data_ptr(), _dt(x), _stream())
    return y


def conv3x3_head(x, *, B, T, H, W, C, weight, bias, out, T_out, classes=None, gn=None):
    if gn is None:
        call("catseg_conv3x3_head", x.data_ptr(), B, T, H, W, C, weight.data_ptr(), bias, _p(classes), T_out,
             out.data_ptr(), _dt(x), _stream())
    else:
        mean, rstd, gamma, beta, cpg = gn
        # one output channel: 9 taps x C MACs per pixel; x read once, the fp32 logit plane written once
        with _rec("conv3x3_head_gn", 2 * B * T * H * W * C * 9, B * T * H * W * (C * x.element_size() + 4)):
            call("catseg_conv3x3_head_gn", x.data_ptr(), B, T, H, W, C, weight.data_ptr(), bias, mean.data_ptr(),
                 rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), cpg, _p(classes), T_out, out.data_ptr(),
                 _dt(x), _stream())
    return out


def corr_embed(corr, *, t_stride, b_stride, B, T, H, W, weight, bias, out, classes=None):
    hidden = weight.shape[0]
    # Conv2d(1, hidden, 7, pad 3): 49 MACs per output channel; each fp32 cost slice read once, X written once
    with _rec("corr_embed", 2 * B * T * H * W * hidden * 49, B * T * H * W * (4 + hidden * out.element_size())):
        call("catseg_corr_embed", corr.data_ptr(), t_stride, b_stride, _p(classes), B, T, H, W, weight.data_ptr(),
             bias.data_ptr(), hidden, out.data_ptr(), _dt(out), _stream())
    return out


def topk_classes(corr, *, t_stride, b_stride, B, T, HW, k, out):
    """The k classes of largest max-over-pixels cost per image, sorted (catseg_topk_classes)."""
    ws = torch.empty(B * T, device=corr.device, dtype=torch.float32)
    call("catseg_topk_classes", corr.data_ptr(), t_stride, b_stride, B, T, HW, k, out.data_ptr(), ws.data_ptr(),
         _stream())
    return out


def transpose_rows(x, out, *, rows, batch=1, in_bstride=0):
    """out[b][c][r] = x[b*in_bstride + r][c] (r < rows), zero for rows <= r < out.shape[-1]
    (catseg_transpose_rows); x (., cols) with any row stride, out (batch, cols, ld) contiguous."""
    cols = out.shape[-2]
    call("catseg_transpose_rows", x.data_ptr(), _ld(x), rows, cols, batch, in_bstride, out.data_ptr(),
         out.shape[-1], _dt(x), _stream())
    return out


def class_attention_kt(tg, T, batch=1):
    """The k half of the class-attention text guidance transposed per image: (batch, 128, Tp),
    Tp = T rounded up to 16, zero past T (catseg_class_attention's tgk_t)."""
    Tp = (T + 15) // 16 * 16
    out = torch.empty(batch, tg.shape[1] // 2, Tp, device=tg.device, dtype=tg.dtype)
    return transpose_rows(tg[:, tg.shape[1] // 2:], out, rows=T, batch=batch, in_bstride=T if batch > 1 else 0)


def gather_rows(x, idx, out):
    call("catseg_gather_rows", x.data_ptr(), _ld(x), idx.data_ptr(), idx.numel(), out.shape[-1], out.data_ptr(),
         _ld(out), _dt(x), _stream())
    return out


def fill(out, value):
    call("catseg_fill_f32", out.data_ptr(), out.numel(), value, _stream())
    return out


def preprocess_im2col(raw, sizes, *, mean, std, res, patch, out):
    B, _, Hp, Wp = raw.shape
    # the padded fp32 canvas read once, the patch matrix (with its zero K padding) written once
    G = res // patch
    with _rec("preprocess_im2col", 0, raw.numel() * 4 + B * G * G * _ld(out) * out.element_size()):
        call("catseg_preprocess_im2col", raw.data_ptr(), sizes.data_ptr(), B, Hp, Wp, mean.data_ptr(),
             std.data_ptr(), res, patch, out.data_ptr(), _ld(out), _dt(out), _stream())
    return out


def vit_embed(patches, cls, pos, gamma, beta, out, *, B, G2, width):
    # fp32 patch rows read, the fp32 residual stream written (pos / cls / LN params are L2-resident)
    with _rec("vit_embed", 0, 4 * width * (B * G2 + B * (G2 + 1))):
        call("catseg_vit_embed", patches.data_ptr(), cls.data_ptr(), pos.data_ptr(), gamma.data_ptr(),
             beta.data_ptr(), B, G2, width, out.data_ptr(), _stream())
    return out


def bicubic_resize(grid, S_in, D, out, S_out):
    call("catseg_bicubic_resize", grid.data_ptr(), S_in, D, out.data_ptr(), S_out, _stream())
    return out


def postprocess(logits, out, *, crop=None):
    B, T, h, w = logits.shape
    H, W = out.shape[-2:]
    ch, cw = crop if crop is not None else (h, w)
    with _rec("postprocess", 0, 4 * B * T * (ch * cw + H * W)):
        call("catseg_postprocess", logits.data_ptr(), B, T, h, w, ch, cw, out.data_ptr(), H, W, _stream())
    return out


def resize_bilinear(x, out, *, crop=None):
    """Bilinear (align_corners=False) of fp32 planes [B][T][h][w] cropped to `crop` -> out [B][T][H][W]."""
    B, T, h, w = x.shape
    H, W = out.shape[-2:]
    ch, cw = crop if crop is not None else (h, w)
    with _rec("resize_bilinear", 0, 4 * (B * T * (ch * cw + H * W))):
        call("catseg_resize_bilinear", x.data_ptr(), B, T, h, w, ch, cw, out.data_ptr(), H, W, _stream())
    return out


def postprocess_argmax(logits, labels, score=None, *, crop=None, sigmoid=True):
    """labels[b] = argmax over T of the sigmoid'ed (sigmoid=True, as `postprocess`) or plain (as
    `resize_bilinear`) fp32 planes [B][T][h][w] cropped to `crop` and resized to labels' (H, W);
    score[b] = that maximum (catseg_postprocess_argmax).  labels (B, H, W) int32, score (B, H, W)
    fp32 or None; the (B, T, H, W) volume is never written."""
    B, T, h, w = logits.shape
    H, W = labels.shape[-2:]
    ch, cw = crop if crop is not None else (h, w)
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == B * H * W
    assert score is None or (score.dtype == torch.float32 and score.is_contiguous() and score.numel() == B * H * W)
    with _rec("postprocess_argmax", 0, 4 * B * (T * ch * cw + H * W * (1 if score is None else 2))):
        call("catseg_postprocess_argmax", logits.data_ptr(), B, T, h, w, ch, cw, 1 if sigmoid else 0,
             labels.data_ptr(), 0 if score is None else score.data_ptr(), H, W, _stream())
    return labels


def postprocess_topk(logits, k, *, crop=None, sigmoid=True, mass=True, reject=None, out_hw):
    """The k best classes of every pixel of the sigmoid'ed (sigmoid=True, as `postprocess`) or plain (as
    `resize_bilinear`) fp32 planes [B][T][h][w] cropped to `crop` and resized to out_hw = (H, W)
    (catseg_postprocess_topk; DESIGN.md section 4, "Confidence outputs"); the (B, T, H, W) volume is never
    written.  1 <= k <= min(4, T).  Returns a dict of fresh tensors: "topk_labels" (B, k, H, W) int32 and
    "topk_score" (B, k, H, W) fp32, rank 0 first (a NaN above every number, then the larger value, the lower
    class among equals: torch.sort(descending=True, stable=True) cut at k; plane 0 is `postprocess_argmax`);
    with mass=True "mass" (B, H, W) fp32, the class-order fp32 sum over all T classes; with reject =
    (min_score, min_margin, reject_label) "labels" (B, H, W) int32, plane 0 with reject_label where
    score_0 < min_score or (k >= 2 and) score_0 - score_1 < min_margin."""
    B, T, h, w = logits.shape
    H, W = (int(e) for e in out_hw)
    k = int(k)
    ch, cw = crop if crop is not None else (h, w)
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    dev = logits.device
    out = {"topk_labels": torch.empty((B, k, H, W), dtype=torch.int32, device=dev),
           "topk_score": torch.empty((B, k, H, W), dtype=torch.float32, device=dev)}
    if mass:
        out["mass"] = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    min_score, min_margin, reject_label = (0.0, 0.0, 0) if reject is None else reject
    if reject is not None:
        out["labels"] = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    # the crop read once; 2 k + mass + labels maps written
    nbytes = 4 * B * (T * ch * cw + H * W * (2 * k + (1 if mass else 0) + (0 if reject is None else 1)))
    with _rec("postprocess_topk", 0, nbytes):
        call("catseg_postprocess_topk", logits.data_ptr(), B, T, h, w, ch, cw, 1 if sigmoid else 0, k,
             out["topk_labels"].data_ptr(), out["topk_score"].data_ptr(), _p(out.get("mass")), _p(out.get("labels")),
             float(min_score), float(min_margin), int(reject_label), H, W, _stream())
    return out


def confidence_bins(topk_labels, conf, gt, counters, *, num_classes, ignore_label=255, clamp_pred=-1, n_bins=15):
    """counters += the calibration counters of one image (catseg_confidence_bins): topk_labels (K, H, W) int32,
    conf (H, W) fp32 (the confidence of rank 0), gt (H, W) int32, counters (3 n_bins + K + 2,) int64 = count,
    correct, conf_q24 (n_bins each), hit (K), valid, nan.  Returns counters."""
    K, H, W = topk_labels.shape
    n_bins = int(n_bins)
    assert topk_labels.dtype == torch.int32 and topk_labels.is_contiguous()
    assert conf.dtype == torch.float32 and conf.is_contiguous() and conf.shape == (H, W)
    assert gt.dtype == torch.int32 and gt.is_contiguous() and gt.shape == (H, W)
    assert conf.device == topk_labels.device and gt.device == topk_labels.device and counters.device == gt.device
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() == 3 * n_bins + K + 2
    with _rec("confidence_bins", 0, 4 * H * W * (K + 2)):
        call("catseg_confidence_bins", topk_labels.data_ptr(), K, conf.data_ptr(), gt.data_ptr(), H, W,
             int(num_classes), int(ignore_label), int(clamp_pred), n_bins, counters.data_ptr(), _stream())
    return counters


def postprocess_tta(logits, views, *, probs=None, labels=None, score=None):
    """Merge of K test-time-augmentation views of one image (catseg_postprocess_tta): per view the
    sigmoid + crop + bilinear resize of `postprocess`, mirrored views flipped back, summed in view
    order and scaled by 1 / K.  logits (K, T, h, w) fp32; views K rows (crop_h, crop_w, flip) of host
    ints; probs (T, H, W) fp32 and / or labels (H, W) int32 (the first maximum over T) with score (H, W)
    fp32 (that maximum) or None.  Outputs not passed are not written.  Returns (probs, labels, score)."""
    K, T, h, w = logits.shape
    views = [tuple(int(e) for e in v) for v in views]
    if len(views) != K or any(len(v) != 3 for v in views):
        raise ValueError(f"postprocess_tta: views must be {K} rows of (crop_h, crop_w, flip), got {views!r}")
    if probs is None and labels is None:
        raise ValueError("postprocess_tta: pass probs and / or labels")
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    H, W = (probs if probs is not None else labels).shape[-2:]
    assert probs is None or (probs.dtype == torch.float32 and probs.is_contiguous() and probs.numel() == T * H * W)
    assert labels is None or (labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == H * W)
    assert score is None or (score.dtype == torch.float32 and score.is_contiguous() and score.numel() == H * W)
    table = (C.c_int32 * (3 * K))(*[e for v in views for e in v])
    # every view's crop read once; the merged volume and / or the label map (and score) written once
    nbytes = 4 * (T * sum(v[0] * v[1] for v in views) + (T * H * W if probs is not None else 0)
                  + (H * W * (1 if score is None else 2) if labels is not None else 0))
    with _rec("postprocess_tta", 0, nbytes):
        call("catseg_postprocess_tta", logits.data_ptr(), K, T, h, w, C.cast(table, C.c_void_p),
             0 if probs is None else probs.data_ptr(), 0 if labels is None else labels.data_ptr(),
             0 if score is None else score.data_ptr(), H, W, _stream())
    return probs, labels, score


def tile_crops(image, origins, th, tw, canvas):
    """Gather the tiles of extent (th, tw) at `origins` [(oy, ox), ...] (host ints, at most 32) of one fp32
    image (3, H, W) into canvas (B, 3, ch, cw) fp32, ch >= th and cw >= tw; the canvas is written whole,
    zero beyond (th, tw) (catseg_tile_crops)."""
    origins = [(int(oy), int(ox)) for oy, ox in origins]
    B = len(origins)
    assert image.dtype == torch.float32 and image.is_contiguous() and image.dim() == 3 and image.shape[0] == 3
    assert canvas.dtype == torch.float32 and canvas.is_contiguous() and tuple(canvas.shape[:2]) == (B, 3)
    H, W = image.shape[-2:]
    ch, cw = canvas.shape[-2:]
    table = (C.c_int32 * (2 * B))(*[e for o in origins for e in o])
    with _rec("tile_crops", 0, 4 * 3 * B * (th * tw + ch * cw)):
        call("catseg_tile_crops", image.data_ptr(), H, W, C.cast(table, C.c_void_p), B, int(th), int(tw),
             canvas.data_ptr(), ch, cw, _stream())
    return canvas


def tiled_merge(logits, geometry, window, rows, *, crop=None, probs=None, labels=None, score=None):
    """Merge of the tiles' logits of one tiled scene (catseg_tiled_merge; cat_seg.tiling holds the grid):
    per tile the sigmoid + crop + bilinear resize of `postprocess` to the tile's extent, summed over the
    covering tiles in row-major tile order and scaled by 1 / count, for output rows rows = (y0, y1).
    logits (n * nx, T, h, w) fp32 holds the tile rows window = (row0, n) of `geometry` (a tiling.TileGrid,
    or (H, W, th, tw, sy, sx)); crop the region of a tile's logits that is resized (default all of it).
    probs (T, H, W) fp32 and / or labels (H, W) int32 with score (H, W) fp32 or None are whole-image
    tensors; rows outside [y0, y1) and outputs not passed are not written.  Returns (probs, labels, score)."""
    H, W, th, tw, sy, sx = (int(v) for v in tuple(geometry)[:6])
    row0, nrows = (int(v) for v in window)
    y0, y1 = (int(v) for v in rows)
    n, T, h, w = logits.shape
    ch, cw = crop if crop is not None else (h, w)
    if probs is None and labels is None:
        raise ValueError("tiled_merge: pass probs and / or labels")
    nx = max(W - tw + sx - 1, 0) // sx + 1
    if n != nrows * nx:
        raise ValueError(f"tiled_merge: a window of {nrows} tile rows of {nx} tiles needs {nrows * nx} logits, "
                         f"got {n}")
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    assert probs is None or (probs.dtype == torch.float32 and probs.is_contiguous() and probs.numel() == T * H * W)
    assert labels is None or (labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == H * W)
    assert score is None or (score.dtype == torch.float32 and score.is_contiguous() and score.numel() == H * W)
    # the window's crops read once (at most); the rows of the outputs written once
    nbytes = 4 * (T * n * ch * cw + (y1 - y0) * W * ((T if probs is not None else 0)
                  + ((1 if score is None else 2) if labels is not None else 0)))
    with _rec("tiled_merge", 0, nbytes):
        call("catseg_tiled_merge", logits.data_ptr(), T, h, w, int(ch), int(cw), H, W, th, tw, sy, sx, row0, nrows,
             y0, y1, 0 if probs is None else probs.data_ptr(), 0 if labels is None else labels.data_ptr(),
             0 if score is None else score.data_ptr(), _stream())
    return probs, labels, score


def tiled_blend(logits, geometry, window, rows, *, weights="uniform", global_logits=None, crop=None, probs=None,
                labels=None, score=None):
    """`tiled_merge` with a window over every tile and, optionally, a global view (catseg_tiled_blend): every
    tile's value weighted by w(y - oy) * w(x - ox), w = tiling.window_weights(tile extent, weights), summed in
    row-major tile order and scaled by 1 / sum(w); with global_logits (T, h, w) fp32, the logits of the whole
    scene resized to the tile's extent, the result is 0.5 * (that + the `postprocess` of global_logits to
    (H, W)).  weights="uniform" without global_logits is `tiled_merge` bit for bit.  The other arguments and
    the return value are `tiled_merge`'s."""
    from . import tiling
    H, W, th, tw, sy, sx = (int(v) for v in tuple(geometry)[:6])
    row0, nrows = (int(v) for v in window)
    y0, y1 = (int(v) for v in rows)
    n, T, h, w = logits.shape
    ch, cw = crop if crop is not None else (h, w)
    win = tiling.check_window(weights, (th, tw))
    if probs is None and labels is None:
        raise ValueError("tiled_blend: pass probs and / or labels")
    nx = max(W - tw + sx - 1, 0) // sx + 1
    if n != nrows * nx:
        raise ValueError(f"tiled_blend: a window of {nrows} tile rows of {nx} tiles needs {nrows * nx} logits, "
                         f"got {n}")
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    assert global_logits is None or (global_logits.dtype == torch.float32 and global_logits.is_contiguous()
                                     and tuple(global_logits.shape[-3:]) == (T, h, w)
                                     and global_logits.numel() == T * h * w)
    assert probs is None or (probs.dtype == torch.float32 and probs.is_contiguous() and probs.numel() == T * H * W)
    assert labels is None or (labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == H * W)
    assert score is None or (score.dtype == torch.float32 and score.is_contiguous() and score.numel() == H * W)
    # the window's crops and the global view's read once (at most); the rows of the outputs written once
    nbytes = 4 * (T * (n + (global_logits is not None)) * ch * cw
                  + (y1 - y0) * W * ((T if probs is not None else 0)
                                     + ((1 if score is None else 2) if labels is not None else 0)))
    with _rec("tiled_blend", 0, nbytes):
        call("catseg_tiled_blend", logits.data_ptr(), T, h, w, int(ch), int(cw), H, W, th, tw, sy, sx, row0, nrows,
             y0, y1, win, 0 if global_logits is None else global_logits.data_ptr(),
             0 if probs is None else probs.data_ptr(), 0 if labels is None else labels.data_ptr(),
             0 if score is None else score.data_ptr(), _stream())
    return probs, labels, score


def avgpool_rows(x, out, *, S, H, W, C, pool):
    """nn.AvgPool2d(pool) over [S][H][W][C] rows -> out [S][H/ph][W/pw][C] (catseg_avgpool_rows)."""
    ph, pw = pool
    with _rec("avgpool_rows", 0, x.element_size() * S * C * (H * W + (H // ph) * (W // pw))):
        call("catseg_avgpool_rows", x.data_ptr(), S, H, W, C, ph, pw, out.data_ptr(), _dt(x), _stream())
    return out


def upsample_add_rows(xp, x, *, S, Hp, Wp, C, H, W):
    """x += bilinear_align_corners(xp -> H x W) on [S][.][.][C] rows (catseg_upsample_add_rows)."""
    assert xp.dtype == x.dtype
    with _rec("upsample_add_rows", 0, x.element_size() * S * C * (Hp * Wp + 2 * H * W)):
        call("catseg_upsample_add_rows", xp.data_ptr(), S, Hp, Wp, C, x.data_ptr(), H, W, _dt(x), _stream())
    return x


def sliding_crops(raw, sizes, out, *, out_res, kernel, stride):
    """Unfold crops + global crop of each image, fp32 0-255 (catseg_sliding_crops)."""
    N, _, Hc, Wc = raw.shape
    with _rec("sliding_crops", 0, 4 * out.numel()):
        call("catseg_sliding_crops", raw.data_ptr(), sizes.data_ptr(), N, Hc, Wc, out_res, kernel, stride,
             out.data_ptr(), _stream())
    return out


def sliding_merge(logits, out, *, kernel, stride, out_res):
    """(Fold(sigmoid(interp tiles))/count + interp(global)) / 2 (catseg_sliding_merge)."""
    N, T = out.shape[:2]
    h, w = logits.shape[-2:]
    with _rec("sliding_merge", 0, 4 * (logits.numel() + out.numel())):
        call("catseg_sliding_merge", logits.data_ptr(), N, T, h, w, kernel, stride, out_res, out.data_ptr(),
             _stream())
    return out


def token_embed(tokens, tok_emb, pos, out):
    n, ctx = tokens.shape
    call("catseg_token_embed", tokens.data_ptr(), n, ctx, tok_emb.data_ptr(), pos.data_ptr(), tok_emb.shape[1],
         out.data_ptr(), _stream())
    return out


def eot_gather(x, tokens, out):
    n, ctx = tokens.shape
    call("catseg_eot_gather", x.data_ptr(), tokens.data_ptr(), n, ctx, out.shape[-1], out.data_ptr(), _stream())
    return out


def _rows_epi(out, bias, add, addmap, add_ncols, act, res, res2, store):
    e = L.RowsEpi()
    e.bias = _p(bias)
    e.addmap = addmap or IDENTITY
    if add is not None:
        e.add, e.ld_add = add.data_ptr(), _ld(add)
        e.add_ncols = add_ncols if add_ncols is not None else add.shape[-1]
    e.act = act
    if res is not None:
        e.res, e.ld_res = res.data_ptr(), _ld(res)
    if res2 is not None:
        e.res2, e.ld_res2 = res2.data_ptr(), _ld(res2)
    e.out = out.data_ptr()
    if store is None:
        e.ldo = _ld(out)
    else:
        e.store_mode = 1
        e.cvt_k, e.cvt_hin, e.cvt_win, e.cvt_cout = store
    return e


def rows_gemm(x, w, out, *, ln=None, eps=1e-5, bias=None, add=None, addmap=None, add_ncols=None,
              act=L.ACT_NONE, res=None, res2=None, store=None, M=None):
    """out = epi(LN?(x) . w^T) over 128-wide rows (catseg_rows_gemm)."""
    M = M if M is not None else x.shape[0]
    N = w.shape[0]
    if x.dtype == torch.float32 and out.dtype == torch.float32:
        # fp32 (config 2): catseg_layernorm + catseg_gemm (same epilogue order: bias, add, act, res, res2)
        # run at ~76 TF/s on these K = 128 GEMMs against the fused row kernel's ~55 (64-row workgroups,
        # 4 MFMAs per k-step per wave)
        a = x
        if ln is not None:
            a = torch.empty(M, w.shape[1], device=x.device, dtype=torch.float32)
            layernorm(x, ln[0], ln[1], a, rows=M, eps=eps)
        ncols = add_ncols if add_ncols is not None else (add.shape[-1] if add is not None else None)
        gemm(a, w, out, M=M, bias=bias, add=add, addmap=addmap, add_ncols=ncols, act=act, res=res, res2=res2,
             store=store)
        return out
    e = _rows_epi(out, bias, add, addmap, add_ncols, act, res, res2, store)
    g, b = (ln if ln is not None else (None, None))
    with _rec("rows_gemm", 2 * M * N * w.shape[1], x.element_size() * M * (w.shape[1] + N)):
        call("catseg_rows_gemm", x.data_ptr(), _ld(x), M, _p(g), _p(b), eps, w.data_ptr(), N, e, _dt(x), _stream())
    return out


def convt64_gn(x, w, out, *, HW, gn, bias, store):
    """out = ConvT_k2(relu(GN(x))) over 64-channel rows (catseg_convt64_gn, bf16)."""
    mean, rstd, gamma, beta, cpg = gn
    e = _rows_epi(out, bias, None, None, None, L.ACT_NONE, None, None, store)
    M = x.shape[0]
    with _rec("convt64_gn", 2 * M * w.shape[0] * w.shape[1], x.element_size() * M * (w.shape[1] + w.shape[0])):
        call("catseg_convt64_gn", x.data_ptr(), M, HW, mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
             beta.data_ptr(), cpg, w.data_ptr(), w.shape[0], e, _stream())
    return out


def rows_mlp(y, w1, b1, w2, out, *, ln, b2=None, act=L.ACT_GELU, res=None, res2=None, eps=1e-5, M=None,
             ref_rows=None):
    """out = act(LN(y) . w1^T + b1) . w2^T + b2 + res + res2 (catseg_rows_mlp).  ref_rows: the
    reference's row count when it computes padded rows (the class MLP, model.py:413)."""
    M = M if M is not None else y.shape[0]
    hidden = w1.shape[0]
    if y.dtype == torch.float32 and out.dtype == torch.float32:
        # fp32 (config 2): LayerNorm + two GEMM launches beat the fused row kernel, whose one workgroup
        # per 64 rows re-stages the 2 x 256 KB of fp32 weights per hidden chunk at one wave per SIMD
        # (1.67 ms per launch at 345,600 rows); the hidden tensor round-trips HBM instead (M x 512 fp32)
        h = torch.empty(M, w1.shape[1], device=y.device, dtype=torch.float32)
        layernorm(y, ln[0], ln[1], h, rows=M, eps=eps)
        u = torch.empty(M, hidden, device=y.device, dtype=torch.float32)
        gemm(h, w1, u, M=M, bias=b1, act=act)
        gemm(u, w2, out, M=M, bias=b2, res=res, res2=res2)
        return out
    e = _rows_epi(out, b2, None, None, None, L.ACT_NONE, res, res2, None)
    ref = 4 * ref_rows * hidden * w1.shape[1] if ref_rows else None
    with _rec("rows_mlp", 4 * M * hidden * w1.shape[1], y.element_size() * M * 2 * w1.shape[1], ref_flops=ref):
        call("catseg_rows_mlp", y.data_ptr(), _ld(y), M, ln[0].data_ptr(), ln[1].data_ptr(), eps, w1.data_ptr(),
             b1.data_ptr(), hidden, act, w2.data_ptr(), e, _dt(y), _stream())
    return out


def swin_proj_mlp(attn, x, w_proj, b_proj, w1, b1, w2, b2, out, *, ln, eps=1e-5):
    """out = x1 + GELU(LN(x1) . w1^T + b1) . w2^T + b2, x1 = x + attn . w_proj^T + b_proj (bf16 rows of
    128; the Swin block after its window attention, catseg_swin_proj_mlp).  out may be x."""
    M, C_ = x.shape
    hidden = w1.shape[0]
    flops = 2 * M * C_ * C_ + 4 * M * hidden * C_
    with _rec("swin_proj_mlp", flops, x.element_size() * M * 3 * C_):
        call("catseg_swin_proj_mlp", attn.data_ptr(), _ld(attn), x.data_ptr(), _ld(x), M, w_proj.data_ptr(),
             b_proj.data_ptr(), ln[0].data_ptr(), ln[1].data_ptr(), eps, w1.data_ptr(), b1.data_ptr(), hidden,
             w2.data_ptr(), b2.data_ptr(), out.data_ptr(), _ld(out), _stream())
    return out


def bce_onehot_loss(logits, targets, ignore_value=255):
    """The training branch's loss (cat_seg_model.py:189-203) on the device: BCE-with-logits of
    logits (B, T, h, w) fp32 bilinearly upsampled to targets' (B, H, W) size, one-hot targets
    (ignore_value -> zeros), mean over every element.  Returns a 0-d fp32 device tensor (no grad)."""
    B, T, h, w = logits.shape
    Bt, H, W = targets.shape
    assert Bt == B and logits.dtype == torch.float32 and logits.is_contiguous()
    tg = targets.to(torch.int32).contiguous()
    ws = torch.empty(B * H, device=logits.device, dtype=torch.float64)
    loss = torch.empty((), device=logits.device, dtype=torch.float32)
    with _rec("bce_onehot_loss", 0, logits.numel() * 4 + tg.numel() * 4):
        call("catseg_bce_onehot_loss", logits.data_ptr(), B, T, h, w, tg.data_ptr(), H, W, ignore_value, ws.data_ptr(),
             loss.data_ptr(), _stream())
    return loss


def bce_onehot_loss_backward(logits, targets, ignore_value=255, grad_loss=None):
    """d bce_onehot_loss / d logits on the device (catseg_bce_onehot_loss_backward): what autograd
    computes for cat_seg_model.py:192-203 (BCE mean backward through the bilinear upsample's
    backward), times grad_loss (0-d device fp32 tensor, None = 1).  Returns (B, T, h, w) fp32."""
    B, T, h, w = logits.shape
    Bt, H, W = targets.shape
    assert Bt == B and logits.dtype == torch.float32 and logits.is_contiguous()
    tg = targets.to(torch.int32).contiguous()
    gl = None if grad_loss is None else grad_loss.to(device=logits.device, dtype=torch.float32).contiguous()
    ws = torch.empty(B * T * H * w, device=logits.device, dtype=torch.float32)
    grad = torch.empty_like(logits)
    with _rec("bce_onehot_loss_backward", 0, logits.numel() * 8 + tg.numel() * 4 + ws.numel() * 8):
        call("catseg_bce_onehot_loss_backward", logits.data_ptr(), B, T, h, w, tg.data_ptr(), H, W, ignore_value,
             None if gl is None else gl.data_ptr(), ws.data_ptr(), grad.data_ptr(), _stream())
    return grad


class BCEOneHotLoss(torch.autograd.Function):
    """bce_onehot_loss with its HIP backward: loss = BCEOneHotLoss.apply(logits, targets, ignore);
    loss.backward() fills logits.grad through catseg_bce_onehot_loss_backward (targets get none)."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_value=255):
        logits = logits.contiguous()
        ctx.save_for_backward(logits, targets)
        ctx.ignore_value = ignore_value
        return bce_onehot_loss(logits, targets, ignore_value)

    @staticmethod
    def backward(ctx, grad_loss):
        logits, targets = ctx.saved_tensors
        return bce_onehot_loss_backward(logits, targets, ctx.ignore_value, grad_loss), None, None


def semseg_confusion(probs, gt, conf, n_invalid, *, num_classes, ignore_label=255, clamp_pred=-1):
    """conf += bincount((N+1) * argmax(probs) + gt') on the device (catseg_semseg_confusion).
    probs (T, H, W) fp32, gt (H, W) int32, conf ((N+1)^2,) int64, n_invalid (1,) int64."""
    T, H, W = probs.shape
    assert probs.is_contiguous() and gt.is_contiguous() and gt.shape == (H, W) and gt.dtype == torch.int32
    assert conf.dtype == torch.int64 and conf.numel() == (num_classes + 1) ** 2 and n_invalid.dtype == torch.int64
    with _rec("semseg_confusion", 0, probs.numel() * 4 + gt.numel() * 4):
        call("catseg_semseg_confusion", probs.data_ptr(), T, H, W, gt.data_ptr(), num_classes, ignore_label,
             clamp_pred, conf.data_ptr(), n_invalid.data_ptr(), _stream())
    return conf


def semseg_confusion_labels(labels, gt, conf, n_invalid, *, num_classes, ignore_label=255, clamp_pred=-1):
    """conf += bincount((N+1) * labels' + gt') on the device (catseg_semseg_confusion_labels): the
    binning of `semseg_confusion` from an argmax map.  labels, gt (H, W) int32, conf ((N+1)^2,) int64,
    n_invalid (1,) int64."""
    H, W = labels.shape
    assert labels.is_contiguous() and labels.dtype == torch.int32
    assert gt.is_contiguous() and gt.shape == (H, W) and gt.dtype == torch.int32
    assert conf.dtype == torch.int64 and conf.numel() == (num_classes + 1) ** 2 and n_invalid.dtype == torch.int64
    with _rec("semseg_confusion_labels", 0, labels.numel() * 4 + gt.numel() * 4):
        call("catseg_semseg_confusion_labels", labels.data_ptr(), H, W, gt.data_ptr(), num_classes, ignore_label,
             clamp_pred, conf.data_ptr(), n_invalid.data_ptr(), _stream())
    return conf


def _label_map_args(labels, what):
    """(H, W, ld) of a 2-D int32 device label map whose rows are contiguous (a row-strided view is fine)."""
    if not torch.is_tensor(labels) or not labels.is_cuda:
        raise ValueError(f"{what}: labels must be a CUDA tensor")
    if labels.dtype != torch.int32 or labels.dim() != 2 or labels.numel() == 0:
        raise ValueError(f"{what}: labels must be a non-empty 2-D int32 tensor, got {labels.dtype} "
                         f"{tuple(labels.shape)}")
    H, W = labels.shape
    if W > 1 and labels.stride(1) != 1:
        raise ValueError(f"{what}: the rows of labels must be contiguous (stride {labels.stride(1)})")
    ld = labels.stride(0) if H > 1 else W
    if ld < W:
        raise ValueError(f"{what}: row stride {ld} < W = {W}")
    return H, W, ld


def boundary_distance(labels, cap, *, clamp_pred=-1, out=None):
    """min(D, cap) of a label map as int16 (catseg_boundary_distance; DESIGN.md section 4, "Boundary-aware
    evaluation"): D(p) = the Chebyshev distance from p to the nearest pixel of another label, the outside of the
    map counting as one (D >= 1; labels >= clamp_pred compare as clamp_pred, clamp_pred < 0: no fold).  labels:
    2-D int32 CUDA tensor, rows may be strided; out: (H, W) int16 (fresh when None), rows may be strided.
    Returns out.  No host synchronisation."""
    H, W, ld = _label_map_args(labels, "boundary_distance")
    nbytes = L.load().catseg_boundary_distance_workspace(H, W, int(cap))
    if nbytes <= 0:
        raise ValueError(f"boundary_distance: H, W and cap must lie in 1 .. 16384, got {H} x {W}, cap {cap!r}")
    if out is None:
        out = torch.empty((H, W), dtype=torch.int16, device=labels.device)
    if (not torch.is_tensor(out) or out.device != labels.device or out.dtype != torch.int16
            or tuple(out.shape) != (H, W) or (W > 1 and out.stride(1) != 1)):
        raise ValueError("boundary_distance: out must be an (H, W) int16 tensor on the map's device with contiguous rows")
    ld_out = out.stride(0) if H > 1 else W
    if ld_out < W:
        raise ValueError(f"boundary_distance: row stride {ld_out} of out < W = {W}")
    ws = torch.empty(nbytes // 2, dtype=torch.int16, device=labels.device)
    # bytes: the map read by both passes, the row distances written and read back, the result written
    with _rec("boundary_distance", 0, 8 * H * W + 2 * nbytes + 2 * H * W):
        call("catseg_boundary_distance", labels.data_ptr(), H, W, ld, int(clamp_pred), int(cap), out.data_ptr(),
             ld_out, ws.data_ptr(), nbytes, _stream())
    return out


def boundary_confusion(pred, gt, widths, counters, *, num_classes, ignore_label=255, clamp_pred=-1):
    """counters += the boundary counters of one image (catseg_boundary_confusion): both distance maps
    (`boundary_distance` with cap = max(widths) + 1; of pred folded by clamp_pred, of gt as it is), then per width
    band_conf ((N+1)^2, [pred][gt]), inter, gt_band and pred_band (N each).  pred, gt: (H, W) int32 contiguous
    CUDA maps; widths: 1 .. 8 ints in 1 .. 16383; counters: (K ((N+1)^2 + 3N),) int64.  Returns counters."""
    H, W, _ = _label_map_args(pred, "boundary_confusion")
    widths = [int(w) for w in widths]
    if not 1 <= len(widths) <= 8 or min(widths) < 1 or max(widths) > 16383:
        raise ValueError(f"boundary_confusion: 1 .. 8 widths in 1 .. 16383, got {widths}")
    assert pred.is_contiguous() and gt.is_contiguous() and gt.shape == (H, W) and gt.dtype == torch.int32
    assert gt.device == pred.device and counters.device == pred.device
    K, n = len(widths), int(num_classes)
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() == K * ((n + 1) ** 2 + 3 * n)
    cap = max(widths) + 1
    dist_pred = boundary_distance(pred, cap, clamp_pred=clamp_pred)
    dist_gt = boundary_distance(gt, cap)
    with _rec("boundary_confusion", 0, 12 * H * W):
        call("catseg_boundary_confusion", pred.data_ptr(), gt.data_ptr(), dist_pred.data_ptr(), dist_gt.data_ptr(),
             H, W, n, int(ignore_label), int(clamp_pred), (C.c_int * K)(*widths), K, counters.data_ptr(), _stream())
    return counters


def _rgb24(v, what):
    """(r, g, b) in 0 .. 255 or a packed 0xRRGGBB int -> the packed int."""
    if isinstance(v, int) and not isinstance(v, bool):
        if not 0 <= v <= 0xFFFFFF:
            raise ValueError(f"{what} must lie in 0x000000 .. 0xFFFFFF, got {v:#x}")
        return v
    try:
        r, g, b = (int(c) for c in v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be (r, g, b) or a packed 0xRRGGBB int, got {v!r}") from None
    if not all(0 <= c <= 255 for c in (r, g, b)):
        raise ValueError(f"{what} must hold values in 0 .. 255, got {v!r}")
    return (r << 16) | (g << 8) | b


def _render_side_map(t, name, dtype, H, W, device):
    """ld of an optional (H, W) map of `dtype` beside the labels of render_labels."""
    what = "render_labels"
    if not torch.is_tensor(t) or t.device != device:
        raise ValueError(f"{what}: {name} must be a tensor on the labels' device")
    if t.dtype != dtype or tuple(t.shape) != (H, W):
        raise ValueError(f"{what}: {name} must be an ({H}, {W}) {dtype} tensor, got {t.dtype} {tuple(t.shape)}")
    if W > 1 and t.stride(1) != 1:
        raise ValueError(f"{what}: the rows of {name} must be contiguous (stride {t.stride(1)})")
    ld = t.stride(0) if H > 1 else W
    if ld < W:
        raise ValueError(f"{what}: row stride {ld} of {name} < W = {W}")
    return ld


def render_labels(labels, palette, *, image=None, gray=True, alpha=0.5, score=None, gt=None, ignore_label=255,
                  error_rgb=(255, 0, 0), ignore_rgb=(0, 0, 0), edge_px=0, edge_rgb=(255, 255, 255), factor=1,
                  other_rgb=(0, 0, 0), clamp_pred=-1, out=None):
    """A label map as an RGB picture on the device (catseg_render_labels; DESIGN.md section 4, "Rendering"):
    (ceil(H / factor), ceil(W / factor), 3) uint8.  Per pixel the palette colour of its label (other_rgb outside the
    palette), with `gt` ignore_rgb where gt == ignore_label and error_rgb where gt differs, blended over `image`
    at `alpha` (times the score, with `score`), edge_rgb where another label lies within edge_px; then the rounded
    mean over factor x factor cells.  Integer arithmetic, bit-exact against tests/render_ref.py.
      labels  2-D int32 CUDA map, rows may be strided; labels >= clamp_pred fold to clamp_pred (< 0: no fold)
      palette (P, 3) uint8 on the same device, 1 <= P <= 8192
      image   uint8, (3, ih, iw) or (ih, iw, 3) (a first dimension of 3 reads as channels), any strides, any size:
              sampled to H x W by the nearest pixel centre; gray: use its luma (PIL's "L") as the background
      score   (H, W) float32, gt (H, W) int32: rows may be strided
      alpha   0 .. 1, used as round(256 alpha); edge_px 0 .. 8; factor 1 .. 64; colours (r, g, b) or 0xRRGGBB
      out     (Ho, Wo, 3) uint8 whose pixels are contiguous, rows may be strided (fresh when None)
    Returns out.  One launch, no workspace, no host synchronisation."""
    what = "render_labels"
    H, W, ld = _label_map_args(labels, what)
    dev = labels.device
    if H > 16384 or W > 16384:
        raise ValueError(f"{what}: H and W must lie in 1 .. 16384, got {H} x {W}")
    if (not torch.is_tensor(palette) or palette.device != dev or palette.dtype != torch.uint8 or palette.dim() != 2
            or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= 8192 or not palette.is_contiguous()):
        raise ValueError(f"{what}: palette must be a contiguous (P, 3) uint8 tensor on the labels' device, "
                         "1 <= P <= 8192")
    try:
        alpha_q8 = int(round(256 * float(alpha)))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: alpha must be a number in 0 .. 1, got {alpha!r}") from None
    if not 0 <= alpha_q8 <= 256:
        raise ValueError(f"{what}: alpha must lie in 0 .. 1, got {alpha!r}")
    if not isinstance(edge_px, int) or isinstance(edge_px, bool) or not 0 <= edge_px <= 8:
        raise ValueError(f"{what}: edge_px must be an int in 0 .. 8, got {edge_px!r}")
    if not isinstance(factor, int) or isinstance(factor, bool) or not 1 <= factor <= 64:
        raise ValueError(f"{what}: factor must be an int in 1 .. 64, got {factor!r}")
    colours = [_rgb24(v, f"{what}: {n}") for n, v in (("other_rgb", other_rgb), ("error_rgb", error_rgb),
                                                      ("ignore_rgb", ignore_rgb), ("edge_rgb", edge_rgb))]
    img_args = (None, 0, 0, 0, 0, 0)
    if image is not None:
        if (not torch.is_tensor(image) or image.device != dev or image.dtype != torch.uint8 or image.dim() != 3
                or image.numel() == 0 or 3 not in (image.shape[0], image.shape[2])):
            raise ValueError(f"{what}: image must be a (3, h, w) or (h, w, 3) uint8 tensor on the labels' device")
        sc, sr, sx = image.stride() if image.shape[0] == 3 else (image.stride(2), image.stride(0), image.stride(1))
        ih, iw = image.shape[1:] if image.shape[0] == 3 else image.shape[:2]
        if ih > 16384 or iw > 16384:
            raise ValueError(f"{what}: image sides must lie in 1 .. 16384, got {ih} x {iw}")
        img_args = (image.data_ptr(), ih, iw, sr, sx, sc)
    ld_score = 0 if score is None else _render_side_map(score, "score", torch.float32, H, W, dev)
    ld_gt = 0 if gt is None else _render_side_map(gt, "gt", torch.int32, H, W, dev)
    Ho, Wo = -(-H // factor), -(-W // factor)
    if out is None:
        out = torch.empty((Ho, Wo, 3), dtype=torch.uint8, device=dev)
    if (not torch.is_tensor(out) or out.device != dev or out.dtype != torch.uint8 or tuple(out.shape) != (Ho, Wo, 3)
            or out.stride(2) != 1 or (Wo > 1 and out.stride(1) != 3)):
        raise ValueError(f"{what}: out must be an ({Ho}, {Wo}, 3) uint8 tensor on the labels' device whose pixels are "
                         "contiguous")
    ld_out = out.stride(0) if Ho > 1 else 3 * Wo
    if ld_out < 3 * Wo:
        raise ValueError(f"{what}: row stride {ld_out} of out < 3 Wo = {3 * Wo}")
    nbytes = H * W * (4 + (3 if image is not None else 0) + (4 if score is not None else 0)
                      + (4 if gt is not None else 0)) + 3 * Ho * Wo
    with _rec("render_labels", 0, nbytes):
        call("catseg_render_labels", labels.data_ptr(), H, W, ld, int(clamp_pred), palette.data_ptr(),
             palette.shape[0], colours[0], *img_args, int(bool(gray)), _p(score), ld_score, _p(gt), ld_gt,
             int(ignore_label), colours[1], colours[2], alpha_q8, edge_px, colours[3], factor, out.data_ptr(), ld_out,
             _stream())
    return out


def _mode_votes_args(labels, score, novote_label, what):
    """(H, W, ld, ld_score, has_novote, novote_label) of a label map and its optional vote arguments."""
    H, W, ld = _label_map_args(labels, what)
    if H > 16384 or W > 16384:
        raise ValueError(f"{what}: H and W must lie in 1 .. 16384, got {H} x {W}")
    ld_score = 0
    if score is not None:
        if not torch.is_tensor(score) or score.device != labels.device:
            raise ValueError(f"{what}: score must be a tensor on the labels' device")
        if score.dtype != torch.float32 or tuple(score.shape) != (H, W):
            raise ValueError(f"{what}: score must be an ({H}, {W}) float32 tensor, got {score.dtype} "
                             f"{tuple(score.shape)}")
        if W > 1 and score.stride(1) != 1:
            raise ValueError(f"{what}: the rows of score must be contiguous (stride {score.stride(1)})")
        ld_score = score.stride(0) if H > 1 else W
        if ld_score < W:
            raise ValueError(f"{what}: row stride {ld_score} of score < W = {W}")
    if novote_label is not None and (not isinstance(novote_label, int) or isinstance(novote_label, bool)
                                     or not -2 ** 31 <= novote_label < 2 ** 31):
        raise ValueError(f"{what}: novote_label must be None or an int32 value, got {novote_label!r}")
    return H, W, ld, ld_score, int(novote_label is not None), 0 if novote_label is None else novote_label


def mode_filter(labels, size=3, *, iterations=1, rule="plurality", score=None, novote_label=None, fill=False,
                out=None):
    """The majority (mode) filter of a label map on the device (catseg_mode_filter; DESIGN.md section 4, "Mode filter
    and overviews"): every pixel takes the label with the greatest vote sum in its size x size window, clipped to the
    map.  Among equal sums its own label wins if it is one of them, otherwise the smallest label value; a pixel whose
    window holds no vote keeps its value.  Integer arithmetic, bit-exact against tests/mode_ref.py.
      labels        2-D int32 CUDA map, rows may be strided; any int32 value is a label
      size          odd, 3 .. 15; iterations 1 .. 8 applies the filter repeatedly (the score stays the same)
      rule          "plurality": the winner is written; "half": only where it holds more than half of the window's
                    votes, otherwise the pixel keeps its value
      score         (H, W) float32, rows may be strided: a pixel casts clamp(rint(score * 65536), 0, 65536) votes
                    (0 for a NaN) instead of 1
      novote_label  pixels of this label cast no votes and keep their value; with fill=True they take their
                    window's winner like any other pixel
      out           (H, W) int32, rows may be strided, must not overlap labels (fresh when None)
    Returns out.  One launch per iteration between two buffers, no workspace, no host synchronisation."""
    what = "mode_filter"
    H, W, ld, ld_score, has_novote, novote = _mode_votes_args(labels, score, novote_label, what)
    if not isinstance(size, int) or isinstance(size, bool) or size % 2 != 1 or not 3 <= size <= 15:
        raise ValueError(f"{what}: size must be an odd int in 3 .. 15, got {size!r}")
    if not isinstance(iterations, int) or isinstance(iterations, bool) or not 1 <= iterations <= 8:
        raise ValueError(f"{what}: iterations must be an int in 1 .. 8, got {iterations!r}")
    if rule not in ("plurality", "half"):
        raise ValueError(f"{what}: rule must be 'plurality' or 'half', got {rule!r}")
    if out is None:
        out = torch.empty((H, W), dtype=torch.int32, device=labels.device)
    if (not torch.is_tensor(out) or out.device != labels.device
            or _label_map_args(out, f"{what} (out)")[:2] != (H, W)):
        raise ValueError(f"{what}: out must be an ({H}, {W}) int32 tensor on the labels' device")
    ld_out = out.stride(0) if H > 1 else W
    # iteration i writes out when the iterations left after it are even, so that the last one does
    other = torch.empty((H, W), dtype=torch.int32, device=labels.device) if iterations > 1 else None
    src, ld_src = labels, ld
    for i in range(iterations):
        dst, ld_dst = (out, ld_out) if (iterations - 1 - i) % 2 == 0 else (other, W)
        with _rec("mode_filter", 0, H * W * (8 + (4 if score is not None else 0))):
            call("catseg_mode_filter", src.data_ptr(), H, W, ld_src, size, int(rule == "half"), _p(score), ld_score,
                 has_novote, novote, int(bool(fill)), dst.data_ptr(), ld_dst, _stream())
        src, ld_src = dst, ld_dst
    return out


def mode_overview(labels, factor, *, score=None, novote_label=None):
    """A label map reduced by an integer factor on the device (catseg_mode_overview; DESIGN.md section 4, "Mode filter
    and overviews"; gdal's -r mode): output (Y, X) of (ceil(H / factor), ceil(W / factor)) takes the label with the
    greatest vote sum of input rows Y f .. min(H, Y f + f) - 1 and the columns likewise, ties to the smallest label
    value; a cell without votes gets novote_label (without one: its smallest label value).  labels, score and
    novote_label as for `mode_filter`; factor 2 .. 32.  Returns {"labels", "votes" (the winner's vote sum), "total"
    (the cell's): int32; "share": float32 votes / total formed in fp64, NaN where total is 0}.  One launch, no
    workspace, no host synchronisation."""
    what = "mode_overview"
    H, W, ld, ld_score, has_novote, novote = _mode_votes_args(labels, score, novote_label, what)
    if not isinstance(factor, int) or isinstance(factor, bool) or not 2 <= factor <= 32:
        raise ValueError(f"{what}: factor must be an int in 2 .. 32, got {factor!r}")
    Ho, Wo = -(-H // factor), -(-W // factor)
    out = torch.empty((3, Ho, Wo), dtype=torch.int32, device=labels.device)
    with _rec("mode_overview", 0, H * W * (4 + (4 if score is not None else 0)) + 12 * Ho * Wo):
        call("catseg_mode_overview", labels.data_ptr(), H, W, ld, factor, _p(score), ld_score, has_novote, novote,
             out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _stream())
    return {"labels": out[0], "votes": out[1], "total": out[2], "share": (out[1].double() / out[2].double()).float()}


def label_runs_count(labels, *, clamp_pred=-1):
    """Count + scan half of `label_runs` (catseg_label_runs_count): returns the int32 workspace tensor, whose
    element 0 is the number of runs R (still on the device) and whose rest holds the write offsets."""
    H, W, ld = _label_map_args(labels, "label_runs")
    nbytes = L.load().catseg_label_runs_workspace(H, W)
    if nbytes <= 0:
        raise ValueError(f"label_runs: a {H} x {W} map needs H * W < 2^31")
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=labels.device)
    with _rec("label_runs_count", 0, 4 * H * W + nbytes):
        call("catseg_label_runs_count", labels.data_ptr(), H, W, ld, int(clamp_pred), ws.data_ptr(), nbytes, _stream())
    return ws


def label_runs_write(labels, ws, run_start, run_label, *, clamp_pred=-1):
    """Write half of `label_runs` (catseg_label_runs_write): fills the first min(R, capacity) elements of the
    int32 device tensors run_start / run_label, capacity = their common length; nothing is stored beyond it."""
    H, W, ld = _label_map_args(labels, "label_runs")
    for t in (run_start, run_label):
        assert t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and (t.numel() <= 1 or t.stride(0) == 1)
    assert ws.is_cuda and ws.dtype == torch.int32 and ws.is_contiguous()
    cap = min(run_start.numel(), run_label.numel())
    with _rec("label_runs_write", 0, 4 * H * W + 8 * cap):
        call("catseg_label_runs_write", labels.data_ptr(), H, W, ld, int(clamp_pred), ws.data_ptr(), ws.numel() * 4,
             run_start.data_ptr(), run_label.data_ptr(), cap, _stream())
    return run_start, run_label


def label_runs(labels, *, clamp_pred=-1):
    """The column-major label runs of a label map (catseg_label_runs_count / _write): with p = x * H + y and
    labels >= clamp_pred folded to clamp_pred (clamp_pred < 0: no fold), a run starts at p = 0 and wherever
    the folded label differs from the one at p - 1 (column x continues column x - 1).  labels: 2-D int32 CUDA
    tensor, possibly a row-strided view.  Returns (run_start, run_label): int32 device tensors of exactly R
    elements, starts ascending.  Every per-label COCO RLE of the map follows from them on the host
    (evaluation.rle_records_from_runs).

    Runs count + scan, reads R from the device (one synchronising 4-byte copy), allocates exactly R and runs the
    write pass.  Not registered as a torch.ops.catseg.* custom op: the output size depends on the data."""
    ws = label_runs_count(labels, clamp_pred=clamp_pred)
    R = int(ws[0].item())
    run_start = torch.empty(R, dtype=torch.int32, device=labels.device)
    run_label = torch.empty(R, dtype=torch.int32, device=labels.device)
    return label_runs_write(labels, ws, run_start, run_label, clamp_pred=clamp_pred)


def _regions_args(labels, connectivity, what):
    H, W, ld = _label_map_args(labels, what)
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    return H, W, ld


def _regions_workspace(H, W, sieve, device, what):
    nbytes = L.load().catseg_label_regions_workspace(H, W, int(sieve))
    if nbytes <= 0:
        raise ValueError(f"{what}: a {H} x {W} map needs H * W < 2^31")
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device), nbytes


def label_regions_count(labels, *, connectivity=8, clamp_pred=-1):
    """Labelling + scan half of `label_regions` (catseg_label_regions_count): returns the int32 workspace
    tensor, whose element 0 is the number of regions R (still on the device)."""
    H, W, ld = _regions_args(labels, connectivity, "label_regions")
    ws, nbytes = _regions_workspace(H, W, False, labels.device, "label_regions")
    with _rec("label_regions_count", 0, 4 * H * W + nbytes):
        call("catseg_label_regions_count", labels.data_ptr(), H, W, ld, int(clamp_pred), int(connectivity),
             ws.data_ptr(), nbytes, _stream())
    return ws


def label_regions_write(labels, ws, region_ids, table, *, clamp_pred=-1, score=None):
    """Write half of `label_regions` (catseg_label_regions_write): fills `region_ids` ((H, W) int32, rows may
    be strided) and the first min(R, capacity) rows of `table`, a dict of device tensors "label", "area", "first"
    (capacity,) int32, "bbox" (capacity, 4) int32 and, with `score` ((H, W) fp32), "score_q16" (capacity,) int64.
    Nothing is stored at a row >= capacity.  No host synchronisation."""
    H, W, ld = _label_map_args(labels, "label_regions")
    if _label_map_args(region_ids, "label_regions (region_ids)")[:2] != (H, W):
        raise ValueError("label_regions: region_ids must have the map's shape")
    ld_ids = region_ids.stride(0) if H > 1 else W
    assert ws.is_cuda and ws.dtype == torch.int32 and ws.is_contiguous()
    cols = [table[k] for k in ("label", "area", "bbox", "first")]
    cap = cols[0].numel()
    for k, t in zip(("label", "area", "bbox", "first"), cols):
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous(), k
        assert tuple(t.shape) == ((cap, 4) if k == "bbox" else (cap,)), k
    sp = ld_s = q16p = 0
    if score is not None:
        if not (score.is_cuda and score.dtype == torch.float32 and tuple(score.shape) == (H, W)
                and (W == 1 or score.stride(1) == 1)):
            raise ValueError("label_regions: score must be an (H, W) fp32 CUDA tensor with contiguous rows")
        ld_s = score.stride(0) if H > 1 else W
        q16 = table["score_q16"]
        assert q16.is_cuda and q16.dtype == torch.int64 and q16.is_contiguous() and tuple(q16.shape) == (cap,)
        sp, q16p = score.data_ptr(), q16.data_ptr()
    with _rec("label_regions_write", 0, 12 * H * W + 36 * cap):
        call("catseg_label_regions_write", labels.data_ptr(), H, W, ld, int(clamp_pred), sp or None, ld_s, ws.data_ptr(),
             ws.numel() * 4, region_ids.data_ptr(), ld_ids, *(t.data_ptr() or None for t in cols), q16p or None, cap,
             _stream())
    return region_ids, table


def label_regions(labels, *, connectivity=8, clamp_pred=-1, score=None):
    """The connected regions of a label map (catseg_label_regions_count / _write): maximal
    sets of pixels of equal label (labels >= clamp_pred folded to clamp_pred; clamp_pred < 0: no fold) connected
    under `connectivity` 4 or 8, numbered 0 .. R-1 in row-major order of their first pixel.  labels: 2-D int32
    CUDA tensor, possibly a row-strided view.  Returns (region_ids, table): region_ids (H, W) int32, table a dict
    of device tensors of exactly R rows: "label" (folded), "area", "first" (y * W + x of the first pixel) int32,
    "bbox" (R, 4) int32 [x0, y0, x1, y1] with x1 / y1 exclusive and, with `score` ((H, W) fp32), "score_q16" int64,
    the sum over the region of rint(score * 65536) (an integer sum: the same bits in any order) and "score" fp32,
    the mean derived from it.

    Runs labelling + scan, reads R from the device (one synchronising 4-byte copy), allocates exactly R and runs
    the write pass.  Not registered as a torch.ops.catseg.* custom op: the output size depends on the data."""
    ws = label_regions_count(labels, connectivity=connectivity, clamp_pred=clamp_pred)
    R = int(ws[0].item())
    dev = labels.device
    table = {"label": torch.empty(R, dtype=torch.int32, device=dev), "area": torch.empty(R, dtype=torch.int32, device=dev),
             "bbox": torch.empty(R, 4, dtype=torch.int32, device=dev), "first": torch.empty(R, dtype=torch.int32, device=dev)}
    if score is not None:
        table["score_q16"] = torch.empty(R, dtype=torch.int64, device=dev)
    region_ids = torch.empty(labels.shape, dtype=torch.int32, device=dev)
    label_regions_write(labels, ws, region_ids, table, clamp_pred=clamp_pred, score=score)
    if score is not None:
        table["score"] = region_mean_score(table["score_q16"], table["area"])
    return region_ids, table


def region_mean_score(score_q16, area):
    """The mean score of every region from the table's fixed-point sum: score_q16 / 65536 / area in fp64, then fp32."""
    return (score_q16.double() / 65536.0 / area.double()).float()


def sieve_labels(labels, min_area, *, connectivity=8, clamp_pred=-1, out=None):
    """The minimum-mapping-unit sieve of a label map (catseg_sieve_labels), one pass: with
    the regions of `labels` (as `label_regions` defines them), every region of area < min_area that touches a
    region of area >= min_area takes the (folded) label of the touching one with the largest area, ties to the
    smallest region number; every other pixel keeps its value (min_area 1 copies the map).  labels: 2-D int32
    CUDA tensor, rows may be strided; out: the same shape (fresh when None), rows may be strided, must not
    overlap labels.  Returns out.  No host synchronisation."""
    H, W, ld = _regions_args(labels, connectivity, "sieve_labels")
    if int(min_area) < 1:
        raise ValueError(f"sieve_labels: min_area must be >= 1, got {min_area!r}")
    ws, nbytes = _regions_workspace(H, W, True, labels.device, "sieve_labels")
    if out is None:
        out = torch.empty((H, W), dtype=torch.int32, device=labels.device)
    if _label_map_args(out, "sieve_labels (out)")[:2] != (H, W):
        raise ValueError("sieve_labels: out must have the map's shape")
    ld_out = out.stride(0) if H > 1 else W
    with _rec("sieve_labels", 0, 8 * H * W + nbytes):
        call("catseg_sieve_labels", labels.data_ptr(), H, W, ld, int(clamp_pred), int(connectivity), int(min_area),
             out.data_ptr(), ld_out, ws.data_ptr(), nbytes, _stream())
    return out


def _outlines_args(ids, connectivity, what):
    H, W, ld = _label_map_args(ids, what)
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    return H, W, ld


def _outlines_workspace(H, W, corners, device, what):
    nbytes = L.load().catseg_region_outlines_workspace(H, W, int(corners))
    if nbytes <= 0:
        raise ValueError(f"{what}: a {H} x {W} map needs H * W < 2^31 and 4 (H + 1) (W + 1) < 2^31" +
                         (f", and at most 4 (H + 1) (W + 1) corners (got {corners})" if corners >= 0 else ""))
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device), nbytes


def region_outlines_count(ids, *, connectivity=8):
    """Corner count + scan third of `region_outlines` (catseg_region_outlines_count): returns the int32 map
    workspace, whose element 0 is the number of corners K (still on the device).  No host synchronisation."""
    H, W, ld = _outlines_args(ids, connectivity, "region_outlines")
    ws, nbytes = _outlines_workspace(H, W, -1, ids.device, "region_outlines")
    with _rec("region_outlines_count", 0, 4 * H * W + nbytes):
        call("catseg_region_outlines_count", ids.data_ptr(), H, W, ld, int(connectivity), ws.data_ptr(), nbytes,
             _stream())
    return ws


def region_outlines_rank(ids, ws, corners, *, connectivity=8):
    """Link + ranking third of `region_outlines` (catseg_region_outlines_rank): with the map workspace `ws` of
    `region_outlines_count` and corners = K read from it, returns the int32 ring workspace, whose element 1 is the
    number of rings NR (still on the device).  No host synchronisation."""
    H, W, ld = _outlines_args(ids, connectivity, "region_outlines")
    corners = int(corners)
    if corners < 1:
        raise ValueError(f"region_outlines: corners must be >= 1, got {corners}")
    assert ws.is_cuda and ws.dtype == torch.int32 and ws.is_contiguous()
    rws, nbytes = _outlines_workspace(H, W, corners, ids.device, "region_outlines")
    with _rec("region_outlines_rank", 0, 4 * H * W + ws.numel() * 4 + nbytes):
        call("catseg_region_outlines_rank", ids.data_ptr(), H, W, ld, int(connectivity), ws.data_ptr(), ws.numel() * 4,
             corners, rws.data_ptr(), nbytes, _stream())
    return rws


def region_outlines_write(ids, rws, corners, out):
    """Write third of `region_outlines` (catseg_region_outlines_write): with the ring workspace `rws` of
    `region_outlines_rank` for the same corners, fills `out`, a dict of device tensors "ring_offset" (capacity + 1,)
    int32, "ring_value" (capacity,) int32, "ring_area2" (capacity,) int64 and "vertices" (vertex capacity, 2) int32:
    rings below min(NR, capacity) and vertices below the vertex capacity; nothing is stored beyond either.  No host
    synchronisation."""
    H, W, ld = _label_map_args(ids, "region_outlines")
    corners = int(corners)
    assert rws.is_cuda and rws.dtype == torch.int32 and rws.is_contiguous()
    off, val, a2, vert = (out[k] for k in ("ring_offset", "ring_value", "ring_area2", "vertices"))
    for k, t, dt in (("ring_offset", off, torch.int32), ("ring_value", val, torch.int32),
                     ("ring_area2", a2, torch.int64), ("vertices", vert, torch.int32)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise ValueError(f"region_outlines: {k} must be a contiguous {dt} CUDA tensor")
    cap = val.numel()
    if off.dim() != 1 or val.dim() != 1 or tuple(off.shape) != (cap + 1,) or tuple(a2.shape) != (cap,):
        raise ValueError("region_outlines: ring_offset must have one element more than ring_value and ring_area2")
    if vert.dim() != 2 or vert.shape[1] != 2:
        raise ValueError(f"region_outlines: vertices must be (capacity, 2), got {tuple(vert.shape)}")
    with _rec("region_outlines_write", 0, rws.numel() * 4 + 16 * cap + 8 * vert.shape[0]):
        call("catseg_region_outlines_write", ids.data_ptr(), H, W, ld, rws.data_ptr(), rws.numel() * 4, corners,
             off.data_ptr(), val.data_ptr() or None, a2.data_ptr() or None, cap, vert.data_ptr() or None,
             vert.shape[0], _stream())
    return out


def region_outlines(ids, *, connectivity=8):
    """The outlines of the regions of a map as polygon rings (catseg_region_outlines_*; DESIGN.md section 4,
    "Region outlines").  ids: 2-D int32 CUDA tensor, possibly a row-strided view; in practice the region numbers of
    `label_regions` under the same connectivity.  Vertices are pixel corners, x in 0..W, y in 0..H, y down.  A ring
    keeps its value on its right: an exterior ring runs clockwise on screen and has ring_area2 > 0, a hole has
    ring_area2 < 0.  At a diagonal pinch a ring turns left under connectivity 8 and right under 4.  Collinear points
    are dropped; a ring is closed implicitly and starts at its corner of smallest key (y * (W + 1) + x) * 4 + d_in;
    rings are ordered by that key.  Returns a dict of device tensors, allocated exactly: "ring_offset" (NR + 1,)
    int32, "ring_value" (NR,) int32, "ring_area2" (NR,) int64 (the shoelace sum, twice the signed area) and
    "vertices" (K, 2) int32 [x, y]; ring j is vertices[ring_offset[j]:ring_offset[j + 1]].

    Two synchronising 4-byte reads (K, then NR) size the buffers.  Not registered as a torch.ops.catseg.* custom op:
    the output sizes depend on the data."""
    ws = region_outlines_count(ids, connectivity=connectivity)
    K = int(ws[0].item())
    rws = region_outlines_rank(ids, ws, K, connectivity=connectivity)
    NR = int(rws[1].item())
    dev = ids.device
    out = {"ring_offset": torch.empty(NR + 1, dtype=torch.int32, device=dev),
           "ring_value": torch.empty(NR, dtype=torch.int32, device=dev),
           "ring_area2": torch.empty(NR, dtype=torch.int64, device=dev),
           "vertices": torch.empty(K, 2, dtype=torch.int32, device=dev)}
    return region_outlines_write(ids, rws, K, out)


SIMPLIFY_MAX_SIDE = 16384
_OUTLINE_KEYS = (("ring_offset", torch.int32), ("ring_value", torch.int32), ("ring_area2", torch.int64),
                 ("vertices", torch.int32))


def _simplify_args(ids, outlines, what="simplify_outlines"):
    """(H, W, ld, NR, K) of a map and the rings `region_outlines` made for it."""
    H, W, ld = _label_map_args(ids, what)
    if H > SIMPLIFY_MAX_SIDE or W > SIMPLIFY_MAX_SIDE:
        raise ValueError(f"{what}: a {H} x {W} map exceeds H, W <= {SIMPLIFY_MAX_SIDE} (the scores are exact int64)")
    for k, dt in _OUTLINE_KEYS:
        t = outlines[k]
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.device == ids.device):
            raise ValueError(f"{what}: outlines[{k!r}] must be a contiguous {dt} CUDA tensor on the map's device")
    off, val, a2, vert = (outlines[k] for k, _ in _OUTLINE_KEYS)
    NR = val.numel()
    if off.dim() != 1 or val.dim() != 1 or tuple(off.shape) != (NR + 1,) or tuple(a2.shape) != (NR,):
        raise ValueError(f"{what}: ring_offset must have one element more than ring_value and ring_area2")
    if vert.dim() != 2 or vert.shape[1] != 2:
        raise ValueError(f"{what}: vertices must be (K, 2), got {tuple(vert.shape)}")
    K = vert.shape[0]
    if not (1 <= NR <= K <= 4 * (H + 1) * (W + 1)):
        raise ValueError(f"{what}: {NR} rings and {K} corners are not the outlines of a {H} x {W} map")
    return H, W, ld, NR, K


def _simplify_workspace(H, W, K, nodes, device, what="simplify_outlines"):
    nbytes = L.load().catseg_outline_simplify_workspace(H, W, K, int(nodes))
    if nbytes <= 0:
        raise ValueError(f"{what}: no workspace for a {H} x {W} map with {K} corners" +
                         (f" and {nodes} nodes (corners <= nodes <= 4 (H + 1) (W + 1))" if nodes >= 0 else ""))
    return torch.empty(nbytes // 4, dtype=torch.int32, device=device), nbytes


def _simplify_tolerance(tolerance, what="simplify_outlines"):
    t = float(tolerance)
    if not 0.0 <= t <= SIMPLIFY_MAX_SIDE:                     # refuses NaN too
        raise ValueError(f"{what}: tolerance must be in [0, {SIMPLIFY_MAX_SIDE}] pixels, got {tolerance!r}")
    return t


def simplify_outlines_count(ids, outlines):
    """Junction + node-count third of `simplify_outlines` (catseg_outline_simplify_count): returns the int32 map
    workspace, whose element 0 is the number of nodes N (still on the device).  No host synchronisation."""
    H, W, ld, NR, K = _simplify_args(ids, outlines)
    ws, nbytes = _simplify_workspace(H, W, K, -1, ids.device)
    with _rec("outline_simplify_count", 0, 4 * H * W + 8 * K + nbytes):
        call("catseg_outline_simplify_count", ids.data_ptr(), H, W, ld, outlines["ring_offset"].data_ptr(), NR,
             outlines["vertices"].data_ptr(), K, ws.data_ptr(), nbytes, _stream())
    return ws


def simplify_outlines_run(ids, outlines, ws, nodes, tolerance):
    """Node, arc and Douglas-Peucker third of `simplify_outlines` (catseg_outline_simplify_run): with the map
    workspace `ws` of `simplify_outlines_count` and nodes = N read from it, returns the int32 node workspace, whose
    element 1 is the number of kept vertices K' (still on the device).  No host synchronisation."""
    H, W, ld, NR, K = _simplify_args(ids, outlines)
    t = _simplify_tolerance(tolerance)
    nodes = int(nodes)
    assert ws.is_cuda and ws.dtype == torch.int32 and ws.is_contiguous()
    nws, nbytes = _simplify_workspace(H, W, K, nodes, ids.device)
    with _rec("outline_simplify_run", 0, ws.numel() * 4 + 8 * K + nbytes):
        call("catseg_outline_simplify_run", outlines["ring_offset"].data_ptr(), NR, outlines["vertices"].data_ptr(), K,
             H, W, t, ws.data_ptr(), ws.numel() * 4, nodes, nws.data_ptr(), nbytes, _stream())
    return nws


def simplify_outlines_write(ids, outlines, nws, nodes, out):
    """Write third of `simplify_outlines` (catseg_outline_simplify_write): with the node workspace `nws` of
    `simplify_outlines_run` for the same nodes, fills `out`, a dict of device tensors "ring_offset" (capacity + 1,)
    int32, "ring_value" (capacity,) int32, "ring_area2" (capacity,) int64, "ring_hole" (capacity,) uint8 and
    "vertices" (vertex capacity, 2) int32: rings below min(NR, capacity) and vertices below the vertex capacity;
    nothing is stored beyond either.  No host synchronisation."""
    what = "simplify_outlines"
    H, W, ld, NR, K = _simplify_args(ids, outlines)
    nodes = int(nodes)
    assert nws.is_cuda and nws.dtype == torch.int32 and nws.is_contiguous()
    for k, dt in _OUTLINE_KEYS + (("ring_hole", torch.uint8),):
        t = out[k]
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise ValueError(f"{what}: out[{k!r}] must be a contiguous {dt} CUDA tensor")
    off, val, a2, hole, vert = (out[k] for k in ("ring_offset", "ring_value", "ring_area2", "ring_hole", "vertices"))
    cap = val.numel()
    if (off.dim() != 1 or val.dim() != 1 or tuple(off.shape) != (cap + 1,) or tuple(a2.shape) != (cap,)
            or tuple(hole.shape) != (cap,)):
        raise ValueError(f"{what}: ring_offset must have one element more than ring_value, ring_area2 and ring_hole")
    if vert.dim() != 2 or vert.shape[1] != 2:
        raise ValueError(f"{what}: vertices must be (capacity, 2), got {tuple(vert.shape)}")
    with _rec("outline_simplify_write", 0, nws.numel() * 4 + 17 * cap + 8 * vert.shape[0]):
        call("catseg_outline_simplify_write", nws.data_ptr(), nws.numel() * 4, H, W, K, nodes, NR,
             outlines["ring_value"].data_ptr(), outlines["ring_area2"].data_ptr(), off.data_ptr(),
             val.data_ptr() or None, a2.data_ptr() or None, hole.data_ptr() or None, cap, vert.data_ptr() or None,
             vert.shape[0], _stream())
    return out


def simplify_outlines(ids, outlines, tolerance):
    """The rings of `region_outlines(ids)` simplified by Douglas-Peucker with `tolerance` (pixels, 0 .. 16384) on the
    device, arc by arc (catseg_outline_simplify_*; DESIGN.md section 4, "Outline simplification"): the boundary
    between two regions is one arc between two junctions (vertices where at least 3 boundary edges meet, and the
    map's corners), so both neighbours keep the same vertices and no sliver or gap opens between them.  Junctions are
    always kept, also where they lie inside a straight edge of a ring (a T-junction), so a ring can gain vertices
    over its source.  ids: the 2-D int32 CUDA map (H, W <= 16384), possibly a row-strided view; outlines: the dict
    `region_outlines` returned for it.  Returns a dict of device tensors, allocated exactly: the same NR rings in the
    same order, "ring_offset" (NR + 1,) int32, "ring_value" (NR,) int32 (copied), "ring_area2" (NR,) int64 (the
    shoelace sum of the kept vertices; may be 0 or change sign), "ring_hole" (NR,) uint8 (1 where the source ring's
    ring_area2 < 0) and "vertices" (K', 2) int32.  A ring may end with 1 or 2 vertices.  Crossings at large
    tolerances are not prevented, and areas are not preserved.

    Two synchronising 4-byte reads (N, then K') size the buffers.  Not registered as a torch.ops.catseg.* custom op:
    the output sizes depend on the data."""
    H, W, ld, NR, K = _simplify_args(ids, outlines)
    _simplify_tolerance(tolerance)
    ws = simplify_outlines_count(ids, outlines)
    N = int(ws[0].item())
    nws = simplify_outlines_run(ids, outlines, ws, N, tolerance)
    K2 = int(nws[1].item())
    dev = ids.device
    out = {"ring_offset": torch.empty(NR + 1, dtype=torch.int32, device=dev),
           "ring_value": torch.empty(NR, dtype=torch.int32, device=dev),
           "ring_area2": torch.empty(NR, dtype=torch.int64, device=dev),
           "ring_hole": torch.empty(NR, dtype=torch.uint8, device=dev),
           "vertices": torch.empty(K2, 2, dtype=torch.int32, device=dev)}
    return simplify_outlines_write(ids, outlines, nws, N, out)


TRAIN_INPUT_MAX_LABELS = 4096


def _train_input_args(src, meta, B, desc_words=C.sizeof(L.TrainImageDesc) // 4):
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.data_ptr() % 16 == 0
    assert meta.is_cuda and meta.dtype == torch.int32 and meta.is_contiguous() and meta.data_ptr() % 8 == 0
    assert B > 0 and meta.numel() >= B * desc_words


def train_crop_select(src, meta, cand_off, B, n_cand, n_labels, ignore_label, max_area, workspace, crops):
    """The category-area rule over every image's candidates (catseg_train_crop_select): `src` the packed
    uint8 pixels, `meta` the packed int32 descriptors (at word 0), candidates (at word cand_off) and tables
    as cat_seg.data.train_input.plan_batch lays them out; crops (B, 4) int32 receives each image's window.
    `workspace`: B * (n_cand + 1) int32, zero before its first use."""
    _train_input_args(src, meta, B)
    if n_labels > TRAIN_INPUT_MAX_LABELS:
        raise ValueError(f"train_crop_select: n_labels {n_labels} > {TRAIN_INPUT_MAX_LABELS} (the LDS histogram)")
    assert crops.is_cuda and crops.dtype == torch.int32 and crops.is_contiguous() and crops.numel() >= 4 * B
    assert workspace.is_cuda and workspace.dtype == torch.int32 and workspace.numel() >= B * (n_cand + 1)
    assert cand_off >= 0 and cand_off + B * n_cand * 4 <= meta.numel()
    with _rec("train_crop_select", 0, 0):
        call("catseg_train_crop_select", src.data_ptr(), meta.data_ptr(), meta.data_ptr(),
             meta.data_ptr() + 4 * cand_off, B, n_cand, int(n_labels), int(ignore_label), float(max_area),
             workspace.data_ptr(), crops.data_ptr(), _stream())
    return crops


def train_augment(src, meta, B, images, targets, ignore_label, crops=None):
    """Resize + crop + colour + flip + pad of a packed batch in one launch (catseg_train_augment):
    images (B, 3, S, S) uint8 and targets (B, S, S) int64, contiguous; `crops` the (B, 4) int32 record of
    train_crop_select when the descriptors select from it."""
    _train_input_args(src, meta, B)
    S = images.shape[-1]
    assert images.is_cuda and images.dtype == torch.uint8 and images.is_contiguous() and tuple(images.shape) == (B, 3, S, S)
    assert targets.is_cuda and targets.dtype == torch.int64 and targets.is_contiguous() and tuple(targets.shape) == (B, S, S)
    assert crops is None or (crops.is_cuda and crops.dtype == torch.int32 and crops.is_contiguous()
                             and crops.numel() >= 4 * B)
    with _rec("train_augment", 0, B * S * S * 11):
        call("catseg_train_augment", src.data_ptr(), meta.data_ptr(), meta.data_ptr(), _p(crops), B, S,
             int(ignore_label), images.data_ptr(), targets.data_ptr(), _stream())
    return images, targets
