"""Training-side HIP kernels (include/catseg_hip_train.h) against torch fp64 autograd of the
reference ops (cat_seg/modeling/transformer/model.py, cat_seg/cat_seg_model.py).

Gate: max |hip - ref| <= 1e-4 * max |ref| for every gradient (fp32 kernels vs fp64), 1e-5 for the conv
forward, 1e-6 for elementwise results and the class / pixel sums, the same bits for copies.

The first half runs every entry point at the training step's shapes; the second ("modes and edge shapes")
runs the modes the model calls but the first half does not (acc_dx = 0, dgamma = None, acc_param = 1,
beta = 1, alpha != 1, y = None, out aliasing x) and the shapes at which a kernel takes another path: the
LayerNorm / l2-normalize widths of every VPL instantiation, more rows than the LayerNorm grid has waves,
more slices than gn_param_kernel has threads, maps narrower than the conv kernels' 16-pixel slab, the
64-row and 32-class block edges of the attention backwards, windows other than 12 x 12, one-entry
pooled grids, and a head conv larger than its capped grid.  Overwritten outputs start as NaN
(nan_out), accumulated ones from a non-zero value.  Strides, padding and writes outside the output
are tests/test_gpu_train_poison.py's subject.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import poison  # noqa: E402
from cat_seg import _lib as L  # noqa: E402
from cat_seg import ops, train_ops as TO  # noqa: E402
from oracle import catseg_oracle as O  # noqa: E402

DEV = "cuda"


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def nan_out(*shape, device=DEV):
    """An fp32 output its call is documented to overwrite completely (beta = 0), prefilled with NaN: an
    element the kernel leaves unwritten cannot pass on what an earlier test left in the allocator's block."""
    return poison.filled(tuple(shape), torch.float32, device)


def nan_like(t):
    return poison.filled(tuple(t.shape), t.dtype, t.device)


def close(a, b, tol=1e-4):
    assert not torch.isnan(a).any(), f"{int(torch.isnan(a).sum())} NaN element(s) in the result"
    e = rel(a, b)
    assert e <= tol, f"rel err {e:.3e} > {tol}"


def g(*shape, seed=0, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=gen, dtype=torch.float64) * scale


def dev(t):
    return t.float().to(DEV).contiguous()


@pytest.mark.parametrize("M,N,K", [(300, 132, 68), (96, 512, 40000), (2304, 768, 171), (5, 4, 8)])
def test_gemm_ex_layouts(M, N, K):
    A = g(M, K, seed=1)
    B = g(K, N, seed=2)
    ref = A @ B
    for a_t in (False, True):
        for b_t in (False, True):
            Ad = dev(A.t() if a_t else A)              # a_t: stored [K][M] (m-contiguous)
            Bd = dev(B.t() if b_t else B)              # b_t: stored [N][K] (k-contiguous)
            a_sm, a_sk = (1, M) if a_t else (K, 1)
            b_sk, b_sn = (1, K) if b_t else (N, 1)
            if (a_t and M % 4) or (not a_t and K % 4) or (b_t and K % 4) or (not b_t and N % 4):
                continue
            out = torch.full((M, N), 3.0, device=DEV)
            TO.gemm_ex(Ad, a_sm, a_sk, Bd, b_sk, b_sn, out, M=M, N=N, K=K, alpha=0.5, beta=1)
            close(out, 0.5 * ref + 3.0)


@pytest.mark.parametrize("terms,tol", [(0, 2e-6), (6, 2e-6), (3, 3e-5)])
@pytest.mark.parametrize("M,N,K", [(300, 132, 68), (128, 384, 20000), (7, 12, 100)])
def test_gemm_ex_split_bf16_forms(terms, tol, M, N, K):
    """The product forms of catseg_gemm_ex (tuning knob gemm_ex_terms): exact-f32 MFMA, the six-pair
    split-bf16 form (automatic for K >= 8192: fp32-class error) and the three-pair form (~2^-17),
    in every operand layout, against fp64 at fp32-scale gates."""
    A = g(M, K, seed=11)
    B = g(K, N, seed=12)
    ref = A @ B
    L.tune("gemm_ex_terms", terms)
    try:
        for a_t in (False, True):
            for b_t in (False, True):
                if (a_t and M % 4) or (not a_t and K % 4) or (b_t and K % 4) or (not b_t and N % 4):
                    continue
                a_sm, a_sk = (1, M) if a_t else (K, 1)
                b_sk, b_sn = (1, K) if b_t else (N, 1)
                out = nan_out(M, N, device=DEV)
                TO.gemm_ex(dev(A.t() if a_t else A), a_sm, a_sk, dev(B.t() if b_t else B), b_sk, b_sn, out,
                           M=M, N=N, K=K)
                close(out, ref, tol)
    finally:
        L.tune("gemm_ex_terms", -1)


@pytest.mark.parametrize("act,fn", [(L.ACT_GELU, F.gelu), (L.ACT_RELU, F.relu),
                                    (L.ACT_QUICKGELU, lambda t: t * torch.sigmoid(1.702 * t))])
def test_gemm_ex_activation_backward_epilogue(act, fn):
    """dU = (dY . W2) * act'(U) in the GEMM's epilogue (the MLP backward's fused form) vs fp64 autograd,
    in place (the epilogue writes over U) and into a fresh buffer."""
    M, N, K = 1000, 512, 128
    dY, W2, U = g(M, K, seed=40), g(K, N, seed=41) / math.sqrt(K), g(M, N, seed=42, scale=2)
    ur = U.clone().requires_grad_(True)
    fn(ur).backward(dY @ W2)
    out = TO.mm(dev(dY), dev(W2), act_u=dev(U), act=act)
    close(out, ur.grad)
    Ud = dev(U)
    TO.mm(dev(dY), dev(W2), out=Ud, act_u=Ud, act=act)
    close(Ud, ur.grad)


@pytest.mark.parametrize("rows,cols,ld", [(5000, 132, 132),      # 16-byte loads, 33 vectors in a 64-wide block
                                          (5000, 130, 130),      # scalar path (cols % 4 != 0)
                                          (3001, 96, 100),       # strided rows, vectors
                                          (300000, 32, 32),      # 2048 chunks, 8 vectors x 32 row lanes
                                          (77, 3072, 3072),      # 12 column blocks, one chunk per 64 rows
                                          (9, 1, 1)])
def test_colsum(rows, cols, ld):
    x = g(rows, ld, seed=3)
    out = torch.ones(cols, device=DEV)
    TO.colsum(dev(x), out, rows=rows, cols=cols, ld=ld, beta=1, alpha=2.0)
    ref = x[:, :cols].double().sum(0)
    close(out, 2 * ref.float() + 1)


@pytest.mark.parametrize("cols", [128, 768])
def test_layernorm_backward(cols):
    x = g(777, cols, seed=4)
    w = 1 + 0.1 * g(cols, seed=5)
    b = 0.1 * g(cols, seed=6)
    dy = g(777, cols, seed=7)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    F.layer_norm(xr, (cols,), wr, br, 1e-5).backward(dy)
    dx = dev(torch.ones_like(x))
    dg = torch.zeros(cols, device=DEV)
    db = torch.zeros(cols, device=DEV)
    TO.layernorm_backward(dev(x), dev(w), dev(dy), dx, acc_dx=True, dgamma=dg, dbeta=db)
    close(dx, xr.grad + 1)
    close(dg, wr.grad)
    close(db, br.grad)


@pytest.mark.parametrize("act,fn", [(L.ACT_GELU, F.gelu), (L.ACT_RELU, F.relu),
                                    (L.ACT_QUICKGELU, lambda t: t * torch.sigmoid(1.702 * t))])
def test_act_forward_backward(act, fn):
    u = g(4096, seed=8, scale=3)
    dy = g(4096, seed=9)
    ur = u.clone().requires_grad_(True)
    a = fn(ur)
    a.backward(dy)
    close(TO.act_forward(dev(u), act), a, 1e-6)
    close(TO.act_backward(dev(u), dev(dy), act), ur.grad, 1e-6)


@pytest.mark.parametrize("S,H,W,C,cpg", [(6, 12, 10, 64, 16),    # one pixel chunk
                                         (3, 40, 37, 32, 16),    # 3 chunks of 512 pixels, the last ragged
                                         (2, 24, 24, 128, 16),   # 4.5 chunks of 128 pixels
                                         (4, 9, 7, 16, 4)])      # one group of 4 channels per quad
def test_groupnorm_relu_stats_and_backward(S, H, W, C, cpg):
    x = g(S, C, H, W, seed=10) * 2 + 0.5
    gm = 1 + 0.2 * g(C, seed=11)
    bt = 0.3 * g(C, seed=12)
    dy = g(S, C, H, W, seed=13)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gm, bt))
    F.relu(F.group_norm(xr, C // cpg, gr, br, 1e-5)).backward(dy)
    xn = dev(x.permute(0, 2, 3, 1))
    mean = nan_out(S * C // cpg, device=DEV)
    rstd = nan_like(mean)
    TO.groupnorm_stats_rows(xn, S, H * W, C, cpg, mean, rstd)
    xs = x.reshape(S, C // cpg, -1)
    close(mean, xs.mean(-1).reshape(-1), 1e-5)
    close(rstd, (1 / torch.sqrt(xs.var(-1, unbiased=False) + 1e-5)).reshape(-1), 1e-5)
    dx = nan_like(xn)
    dg = torch.zeros(C, device=DEV)
    db = torch.zeros(C, device=DEV)
    TO.groupnorm_relu_backward(xn, dev(dy.permute(0, 2, 3, 1)), dx, S=S, HW=H * W, C_=C, cpg=cpg, mean=mean, rstd=rstd,
                               gamma=dev(gm), beta=dev(bt), dgamma=dg, dbeta=db)
    close(dx, xr.grad.permute(0, 2, 3, 1))
    close(dg, gr.grad)
    close(db, br.grad)


def test_sum_classes_and_pixels():
    B, T, HW, C = 3, 7, 25, 64
    x = g(B * T * HW, 96, seed=14)
    xr = x[:, :C].reshape(B, T, HW, C)
    out = torch.ones(B * HW, C, device=DEV)
    TO.sum_classes(dev(x), out, B=B, T=T, HW=HW, C_=C, beta=1)
    close(out, xr.sum(1).reshape(B * HW, C) + 1, 1e-6)
    out2 = nan_out(T, C, device=DEV)
    TO.sum_pixels(dev(x), out2, B=B, T=T, HW=HW, C_=C)
    close(out2, xr.sum((0, 2)), 1e-6)


def test_avgpool_and_upsample_ac_backward():
    S, H, W, C = 5, 24, 24, 16
    x = g(S, C, H, W, seed=15)
    xr = x.clone().requires_grad_(True)
    xp = F.avg_pool2d(xr, 2)
    y = F.interpolate(xp, size=(H, W), mode="bilinear", align_corners=True)
    dy = g(S, C, H, W, seed=16)
    y.backward(dy)
    # upsample backward to the pooled grid, then the pool backward
    dyn = dev(dy.permute(0, 2, 3, 1))
    dxp = nan_out(S * 12 * 12, C, device=DEV)
    TO.upsample_ac_backward_rows(dyn, dxp, S=S, H=H, W=W, C_=C, Hp=12, Wp=12)
    dx = torch.ones(S * H * W, C, device=DEV)
    TO.avgpool_backward_rows(dxp, dx, S=S, H=H, W=W, C_=C, pool=(2, 2), beta=1)
    close(dx, xr.grad.permute(0, 2, 3, 1).reshape(-1, C) + 1)


def test_l2normalize_backward():
    x = g(300, 96, seed=17)
    dy = g(300, 96, seed=18)
    xr = x.clone().requires_grad_(True)
    F.normalize(xr, dim=-1).backward(dy)
    dx = torch.zeros(300, 96, device=DEV)
    TO.l2normalize_backward(dev(x), dev(dy), dx, rows=300, cols=96)
    close(dx, xr.grad)


@pytest.mark.parametrize("k", [2, 4])
def test_convtranspose_backward_via_gather(k):
    S, h, cin, cout = 3, 6, 32, 16
    x = g(S, cin, h, h, seed=19)
    w = g(cin, cout, k, k, seed=20) * 0.2
    b = g(cout, seed=21)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.conv_transpose2d(xr, wr, br, stride=k)
    dy = g(*y.shape, seed=22)
    y.backward(dy)
    G = nan_out(S * h * h, k * k * cout, device=DEV)
    TO.convt_gather(dev(dy.permute(0, 2, 3, 1)).reshape(-1, cout), G, S=S, hin=h, win=h, k=k, cout=cout)
    Wg = dev(w.permute(2, 3, 1, 0).reshape(k * k * cout, cin))      # [(ky, kx, co)][ci]
    X = dev(x.permute(0, 2, 3, 1).reshape(-1, cin))
    dX = TO.mm(G, Wg)
    close(dX, xr.grad.permute(0, 2, 3, 1).reshape(-1, cin))
    dWg = TO.mm(G.t(), X)
    close(dWg.reshape(k, k, cout, cin).permute(3, 2, 0, 1), wr.grad)
    db = nan_out(cout, device=DEV)
    TO.colsum(G, db, rows=S * h * h * k * k, cols=cout, ld=cout)
    close(db, br.grad)


def _window_ref(q, k, v, H, W, ws, shift, nh):
    """WindowAttention core (model.py:86-114 without the projections) over rows [S*H*W][D], the
    roll / partition / reverse of SwinTransformerBlock.forward (model.py:185-216)."""
    S = q.shape[0] // (H * W)
    D = q.shape[1]

    def part(t):
        t = t.reshape(S, H, W, D)
        if shift:
            t = torch.roll(t, (-shift, -shift), (1, 2))
        return O.window_partition(t, ws).reshape(-1, ws * ws, nh, D // nh).permute(0, 2, 1, 3)

    qw, kw, vw = part(q), part(k), part(v)
    hd = D // nh
    a = (qw * hd ** -0.5) @ kw.transpose(-2, -1)
    if shift:
        m = O.shift_mask(H, W, ws, shift).to(a.dtype)
        nw = m.shape[0]
        a = (a.view(-1, nw, nh, ws * ws, ws * ws) + m.unsqueeze(1).unsqueeze(0)).view(-1, nh, ws * ws, ws * ws)
    a = a.softmax(-1)
    o = (a @ vw).transpose(1, 2).reshape(-1, ws, ws, D)
    o = O.window_reverse(o, ws, H, W)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(S * H * W, D)


def _window_attention_backward_case(S, H, W, ws, nh, shift):
    D = nh * 32
    R = S * H * W
    qkv = g(R, 3 * D, seed=23)
    dout = g(R, D, seed=24)
    qr, kr, vr = (qkv[:, i * D:(i + 1) * D].clone().requires_grad_(True) for i in range(3))
    o = _window_ref(qr, kr, vr, H, W, ws, shift, nh)
    o.backward(dout)
    # the forward kernel's own output feeds D_q = dO . O
    qkvd = dev(qkv)
    od = nan_out(R, D, device=DEV)
    ops.attention(qkvd[:, :D], qkvd[:, D:2 * D], qkvd[:, 2 * D:], od, n_seq=S * (H // ws) * (W // ws), seq_len=ws * ws,
                  n_heads=nh, head_dim=D // nh, scale=(D // nh) ** -0.5, mode=1, img_hw=(H, W), window=ws, shift=shift)
    close(od, o, 1e-5)
    dqkv = nan_out(R, 3 * D, device=DEV)
    TO.window_attention_backward(qkvd, od, dev(dout), dqkv, S=S, img_hw=(H, W), window=ws, shift=shift, n_heads=nh,
                                 head_dim=D // nh, scale=(D // nh) ** -0.5)
    close(dqkv[:, :D], qr.grad)
    close(dqkv[:, D:2 * D], kr.grad)
    close(dqkv[:, 2 * D:], vr.grad)


@pytest.mark.parametrize("shift", [0, 6])
def test_window_attention_backward(shift):
    _window_attention_backward_case(3, 24, 24, 12, 4, shift)


@pytest.mark.parametrize("shift", ["0", "1", "ws-1"])
@pytest.mark.parametrize("S,H,W,ws,nh", [(2, 8, 4, 4, 1),        # one 16-token tile; the map one window wide
                                         (1, 16, 8, 8, 2),       # four tiles, two windows, two heads
                                         (1, 24, 12, 12, 4)])    # the nine tiles of WNMAX on a 2 x 1 window grid
def test_window_attention_backward_windows(S, H, W, ws, nh, shift):
    """Windows other than 12 x 12 on the square 24 x 24 map, with the smallest and the largest shift.  The
    forward kernel takes every one of these shapes, so `o` is its own output, as in the test above."""
    _window_attention_backward_case(S, H, W, ws, nh, {"0": 0, "1": 1, "ws-1": ws - 1}[shift])


def close_dqkv(dqkv, grads, width, one_key=False):
    """dq, dk and dv each against its own reference under `close`.
    one_key: the softmax (or the linear attention's normaliser) runs over a single key, so the output is v
    whatever q and k are: the reference's dq and dk are zero (dense) or a residue of the normaliser's eps
    (linear, ~1e-9), while an fp32 kernel forms them as the difference of two O(1) dot products (dP - D) and
    is left with their rounding, ~1e-7 of the operands whatever the result.  A gate relative to max |dq ref|
    has no scale there (measured on the MI355X: |dq| up to 3.8e-7 against a reference of exactly 0 for the dense
    kernel at L = 1; an error of 8.4 max |dq ref|, with dq ref ~ 6e-10, for the linear one at T = 1, n_pad = 0),
    so these cases compare the whole gradient dq | dk | dv with the whole reference under the same
    1e-4 * max |ref|."""
    if one_key:
        close(dqkv, torch.cat(list(grads), 1))
        return
    for i, ref in enumerate(grads):
        close(dqkv[:, i * width:(i + 1) * width], ref)


def _dense_attention_backward_case(n_seq, L_, nh, causal):
    hd = 64
    W = nh * hd
    R = n_seq * L_
    qkv = g(R, 3 * W, seed=40)
    dout = g(R, W, seed=41)
    qr, kr, vr = (qkv[:, i * W:(i + 1) * W].clone().requires_grad_(True) for i in range(3))

    def heads(t):
        return t.reshape(n_seq, L_, nh, hd).permute(0, 2, 1, 3)

    s = (heads(qr) * hd ** -0.5) @ heads(kr).transpose(-2, -1)
    if causal:
        s = s + torch.full((L_, L_), float("-inf"), dtype=s.dtype).triu_(1)
    o = (s.softmax(-1) @ heads(vr)).permute(0, 2, 1, 3).reshape(R, W)
    o.backward(dout)
    qkvd = dev(qkv)
    od = nan_out(R, W, device=DEV)
    ops.attention(qkvd[:, :W], qkvd[:, W:2 * W], qkvd[:, 2 * W:], od, n_seq=n_seq, seq_len=L_, n_heads=nh,
                  head_dim=hd, scale=hd ** -0.5, causal=causal)
    close(od, o, 1e-5)
    dqkv = nan_out(R, 3 * W, device=DEV)
    TO.attention_backward(qkvd, od, dev(dout), dqkv, n_seq=n_seq, seq_len=L_, n_heads=nh, head_dim=hd,
                          scale=hd ** -0.5, causal=causal)
    close_dqkv(dqkv, (qr.grad, kr.grad, vr.grad), W, one_key=L_ == 1)


@pytest.mark.parametrize("n_seq,L_,nh,causal", [(2, 577, 3, False), (5, 14, 2, True), (1, 77, 2, True),
                                                 (3, 50, 1, False)])
def test_dense_attention_backward(n_seq, L_, nh, causal):
    """CLIP nn.MultiheadAttention core (model_vpt.py:202-206; causal triu -inf mask, model_vpt.py:400-406)."""
    _dense_attention_backward_case(n_seq, L_, nh, causal)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L_", [1, 64, 65, 128])
def test_dense_attention_backward_block_edges(L_, causal):
    """One token (see close_dqkv), one full 64-row block, a block and a row, two full blocks."""
    _dense_attention_backward_case(2, L_, 2, causal)


def _linear_attention_backward_case(B, T, HW, n_pad):
    nh, D = 4, 128
    hd = D // nh
    R = B * T * HW
    qkv = g(R, 3 * D, seed=25)
    kv_pad = g(2, D, seed=26)
    dy = g(R, D, seed=27)
    qr, kr, vr = (qkv[:, i * D:(i + 1) * D].clone().requires_grad_(True) for i in range(3))
    kp, vp = (kv_pad[i].clone().requires_grad_(True) for i in range(2))

    def seq(t, pad):      # rows (b, t, p) -> (b*p, T + n_pad, nh, hd)
        t = t.reshape(B, T, HW, D).permute(0, 2, 1, 3)
        if n_pad:
            t = torch.cat([t, pad.reshape(1, 1, 1, D).expand(B, HW, n_pad, D)], 2)
        return t.reshape(B * HW, T + n_pad, nh, hd)

    out = O.linear_attention(seq(qr, kp), seq(kr, kp), seq(vr, vp))[:, :T]
    out = out.reshape(B, HW, T, D).permute(0, 2, 1, 3).reshape(R, D)
    out.backward(dy)
    dqkv = nan_out(R, 3 * D, device=DEV)
    dkp = nan_out(D, device=DEV)
    dvp = nan_out(D, device=DEV)
    kw = dict(k_pad=dev(kv_pad[0]), v_pad=dev(kv_pad[1]), dk_pad=dkp, dv_pad=dvp) if n_pad else {}
    TO.linear_attention_backward(dev(qkv), dev(dy), dqkv, B=B, T=T, HW=HW, n_heads=nh, head_dim=hd, n_pad=n_pad, **kw)
    close_dqkv(dqkv, (qr.grad, kr.grad, vr.grad), D, one_key=T + n_pad == 1)
    if n_pad:
        close(dkp, kp.grad)
        close(dvp, vp.grad)


@pytest.mark.parametrize("T,n_pad", [(20, 236), (171, 85), (256, 0)])
def test_linear_attention_backward(T, n_pad):
    _linear_attention_backward_case(2, T, 9, n_pad)


@pytest.mark.parametrize("n_pad", [0, 1])
@pytest.mark.parametrize("T", [1, 32, 33])
def test_linear_attention_backward_chunk_edges(T, n_pad):
    """One class (alone, n_pad = 0, it is the only key: see close_dqkv), one full chunk of LCH = 32 classes, one
    chunk and a class; one pixel, one padding token."""
    _linear_attention_backward_case(1, T, 1, n_pad)


@pytest.mark.parametrize("cin,cout,k,relu,S", [(96, 64, 3, False, 3), (64, 32, 3, True, 3), (1, 128, 7, False, 3),
                                               (128, 16, 3, True, 3), (20, 8, 3, False, 3),
                                               (3, 16, 3, False, 3),      # scalar (cin % 4 != 0) 192-row weight tiles
                                               (32, 32, 3, True, 24),     # weight gradient split over 11 pixel ranges
                                               (96, 64, 3, False, 40)])   # 256 x 32 and 128 x 64 tiles, split-K
def test_conv2d_forward_dgrad_wgrad(cin, cout, k, relu, S):
    H, W = 24, 20
    x = g(S, cin, H, W, seed=28)
    w = g(cout, cin, k, k, seed=29) / math.sqrt(cin * k * k)
    b = g(cout, seed=30)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(xr, wr, br, padding=k // 2)
    if relu:
        y = F.relu(y)
    dy = g(*y.shape, seed=31)
    y.backward(dy)
    xn = dev(x.permute(0, 2, 3, 1).reshape(-1, cin))
    wt = dev(w.permute(2, 3, 1, 0).reshape(k * k * cin, cout))         # [(tap, ci)][co]
    yd = nan_out(S * H * W, cout, device=DEV)
    TO.conv2d(xn, wt, yd, S=S, H=H, W=W, cin=cin, cout=cout, ksize=k, bias=dev(b), act=L.ACT_RELU if relu else 0)
    close(yd, y.permute(0, 2, 3, 1).reshape(-1, cout), 1e-5)
    dyn = dev(dy.permute(0, 2, 3, 1).reshape(-1, cout))
    if relu:
        dyn = TO.act_backward(yd, dyn, L.ACT_RELU)
    dw = nan_out(k * k * cin, cout, device=DEV)
    TO.conv2d_wgrad(xn, dyn, dw, S=S, H=H, W=W, cin=cin, cout=cout, ksize=k)
    close(dw.reshape(k, k, cin, cout).permute(3, 2, 0, 1), wr.grad)
    if cin % 4 == 0:
        # data gradient: conv of dY with the flipped, transposed weight [(tap, co)][ci]
        wf = dev(w.flip(2, 3).permute(2, 3, 0, 1).reshape(k * k * cout, cin))
        dx = nan_out(S * H * W, cin, device=DEV)
        TO.conv2d(dyn, wf, dx, S=S, H=H, W=W, cin=cout, cout=cin, ksize=k)
        close(dx, xr.grad.permute(0, 2, 3, 1).reshape(-1, cin))


@pytest.mark.parametrize("max_norm", [0.0, 0.01, 1e6])
def test_adamw_matches_torch(max_norm):
    """cat_seg.optim.AdamW (catseg_adamw_step) vs torch.optim.AdamW behind the reference's
    FullModelGradientClippingOptimizer (train_net.py:228-253), 4 steps, three parameter groups."""
    from cat_seg.optim import AdamW
    gen = torch.Generator().manual_seed(50)
    shapes = [(128, 256), (5000,), (3, 4, 5), (1,), (4097,), (4096,), (8193,)]   # one chunk exactly; two and an element
    base = [torch.randn(*s, generator=gen) for s in shapes]
    grads = [[torch.randn(*s, generator=gen) for s in shapes] for _ in range(4)]
    mine = [b.clone().cuda().requires_grad_(True) for b in base]
    ref = [b.clone().cuda().requires_grad_(True) for b in base]

    def groups(ps):
        return [{"params": ps[:2], "lr": 2e-4, "weight_decay": 1e-4}, {"params": ps[2:4], "lr": 2e-6,
                "weight_decay": 0.0}, {"params": ps[4:], "lr": 1e-3, "weight_decay": 0.05}]

    o1 = AdamW(groups(mine), 2e-4, max_grad_norm=max_norm)
    o2 = torch.optim.AdamW(groups(ref), 2e-4)
    for st in range(4):
        for p, q, gr in zip(mine, ref, grads[st]):
            p.grad = gr.cuda()
            q.grad = gr.cuda()
        o1.step()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ref, max_norm)
        o2.step()
        for p, q in zip(mine, ref):
            assert (p - q).abs().max().item() <= 1e-6 * q.abs().max().item() + 1e-7
            assert (p.grad - q.grad).abs().max().item() <= 1e-6 * q.grad.abs().max().item()
    if max_norm > 0:
        tot = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g.cuda()) for g in grads[-1]]))
        assert abs(o1.last_grad_norm[0].item() - tot.item()) <= 1e-5 * tot.item()
    # the state layout is torch's: the two optimizers' state dicts load into each other
    sd = o1.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    o2.load_state_dict(sd)


def test_head_conv_backward():
    S, H, W, C = 5, 32, 24, 32
    x = g(S, C, H, W, seed=32)
    w = g(1, C, 3, 3, seed=33) / math.sqrt(9 * C)
    xr, wr = (t.clone().requires_grad_(True) for t in (x, w))
    y = F.conv2d(xr, wr, padding=1)
    dl = g(*y.shape, seed=34)
    y.backward(dl)
    dx = nan_out(S * H * W, C, device=DEV)
    dw = nan_out(9, C, device=DEV)
    TO.head_conv_backward(dev(x.permute(0, 2, 3, 1)), dev(dl), dev(w[0].permute(1, 2, 0).reshape(9, C)), dx, dw,
                          S=S, H=H, W=W, C_=C)
    close(dx, xr.grad.permute(0, 2, 3, 1).reshape(-1, C))
    close(dw, wr.grad[0].permute(1, 2, 0).reshape(9, C))


# ============================================================================= modes and edge shapes
# Every mode the model calls (cat_seg/training.py) and every shape at which a kernel takes another path.
# Overwritten outputs start as NaN, accumulated ones from a non-zero value.

@pytest.mark.parametrize("rows", [1, 5, 4099])          # one row; two workgroups; past the 4 x LN_WG_MAX waves of the grid
@pytest.mark.parametrize("cols", [64, 256, 512, 1024])  # VPL 1, 4, 8, 16 (2 and 12 are the test above)
def test_layernorm_backward_modes(cols, rows):
    """acc_dx 0 / 1, with the parameter gradients (overwritten) and without them (dgamma = None)."""
    x = g(rows, cols, seed=60) * 2 + 0.3
    w = 1 + 0.1 * g(cols, seed=61)
    b = 0.1 * g(cols, seed=62)
    dy = g(rows, cols, seed=63)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    F.layer_norm(xr, (cols,), wr, br, 1e-5).backward(dy)
    xd, wd, dyd = dev(x), dev(w), dev(dy)
    for acc_dx in (False, True):
        for params in (True, False):
            dx = dev(torch.ones_like(x)) if acc_dx else nan_out(rows, cols)
            dg, db = (nan_out(cols), nan_out(cols)) if params else (None, None)
            TO.layernorm_backward(xd, wd, dyd, dx, acc_dx=acc_dx, dgamma=dg, dbeta=db)
            close(dx, xr.grad + 1 if acc_dx else xr.grad)
            if params:
                close(dg, wr.grad)
                close(db, br.grad)


@pytest.mark.parametrize("cols", [64, 768])
def test_layernorm_backward_accumulates_one_row(cols):
    """acc_param = 1 on a single row (the pad token's LayerNorm) into the dgamma / dbeta of a previous call."""
    x = g(6, cols, seed=64)
    w = 1 + 0.1 * g(cols, seed=65)
    dy = g(6, cols, seed=66)
    grads = []
    for rows in (slice(0, 5), slice(5, 6)):
        xr, wr, br = (t.clone().requires_grad_(True) for t in (x[rows], w, torch.zeros_like(w)))
        F.layer_norm(xr, (cols,), wr, br, 1e-5).backward(dy[rows])
        grads.append((xr.grad, wr.grad, br.grad))
    dg, db = nan_out(cols), nan_out(cols)
    dx5, dx1 = nan_out(5, cols), nan_out(1, cols)
    TO.layernorm_backward(dev(x[:5]), dev(w), dev(dy[:5]), dx5, dgamma=dg, dbeta=db)
    TO.layernorm_backward(dev(x[5:]), dev(w), dev(dy[5:]), dx1, dgamma=dg, dbeta=db, acc_param=True)
    close(dx5, grads[0][0])
    close(dx1, grads[1][0])
    close(dg, grads[0][1] + grads[1][1])
    close(db, grads[0][2] + grads[1][2])


@pytest.mark.parametrize("acc_param", [False, True])
@pytest.mark.parametrize("S,HW,C,cpg", [(300, 4, 16, 4),       # more slices than gn_param_kernel has threads
                                        (2, 17, 1024, 16),      # C / 4 = 256 quads: one pixel per pass, two chunks
                                        (3, 5, 4, 4)])          # one quad, one group
def test_groupnorm_relu_edge_shapes(S, HW, C, cpg, acc_param):
    x = g(S, C, HW, 1, seed=67) * 2 + 0.5
    gm = 1 + 0.2 * g(C, seed=68)
    bt = 0.3 * g(C, seed=69)
    dy = g(S, C, HW, 1, seed=70)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gm, bt))
    F.relu(F.group_norm(xr, C // cpg, gr, br, 1e-5)).backward(dy)
    xn = dev(x.permute(0, 2, 3, 1))
    mean = nan_out(S * C // cpg)
    rstd = nan_like(mean)
    TO.groupnorm_stats_rows(xn, S, HW, C, cpg, mean, rstd)
    xs = x.reshape(S, C // cpg, -1)
    close(mean, xs.mean(-1).reshape(-1), 1e-5)
    close(rstd, (1 / torch.sqrt(xs.var(-1, unbiased=False) + 1e-5)).reshape(-1), 1e-5)
    dx = nan_like(xn)
    dg = torch.full((C,), 2.0, device=DEV) if acc_param else nan_out(C)
    db = torch.full((C,), -3.0, device=DEV) if acc_param else nan_out(C)
    TO.groupnorm_relu_backward(xn, dev(dy.permute(0, 2, 3, 1)), dx, S=S, HW=HW, C_=C, cpg=cpg, mean=mean, rstd=rstd,
                               gamma=dev(gm), beta=dev(bt), dgamma=dg, dbeta=db, acc_param=acc_param)
    close(dx, xr.grad.permute(0, 2, 3, 1))
    close(dg, gr.grad + 2 if acc_param else gr.grad)
    close(db, br.grad - 3 if acc_param else br.grad)


@pytest.mark.parametrize("beta", [0, 1])
def test_sum_classes_one_pixel(beta):
    """HW = 1 (the text guidance's repeat over classes), accumulating and into NaN."""
    B, T, C = 3, 7, 64
    x = g(B * T, C, seed=71)
    out = torch.ones(B, C, device=DEV) if beta else nan_out(B, C)
    TO.sum_classes(dev(x), out, B=B, T=T, HW=1, C_=C, beta=beta)
    close(out, x.reshape(B, T, C).sum(1) + beta, 1e-6)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("HW", [1, 3, 5])       # fewer pixels than the 4 row lanes, and one more
@pytest.mark.parametrize("C", [4, 70])          # one column block mostly idle; two blocks, the second ragged
def test_sum_pixels_edge_shapes(C, HW, beta):
    B, T = 3, 7
    x = g(B * T * HW, C, seed=72)
    out = torch.ones(T, C, device=DEV) if beta else nan_out(T, C)
    TO.sum_pixels(dev(x), out, B=B, T=T, HW=HW, C_=C, beta=beta)
    close(out, x.reshape(B, T, HW, C).sum((0, 2)) + beta, 1e-6)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("H,W,pool", [(25, 23, (2, 2)),      # ragged: the last row and column are dropped
                                      (12, 12, (3, 4)),      # a window that is not square
                                      (6, 6, (6, 6)),        # the whole map in one window
                                      (5, 5, (1, 1))])       # the identity
def test_avgpool_backward_shapes(H, W, pool, beta):
    """nn.AvgPool2d backward; the border a ragged map drops gets zero gradient, as F.avg_pool2d gives."""
    S, C = 2, 8
    xr = g(S, C, H, W, seed=73).requires_grad_(True)
    xp = F.avg_pool2d(xr, pool)
    dxp = g(*xp.shape, seed=74)
    xp.backward(dxp)
    dx = torch.ones(S * H * W, C, device=DEV) if beta else nan_out(S * H * W, C)
    TO.avgpool_backward_rows(dev(dxp.permute(0, 2, 3, 1)).reshape(-1, C), dx, S=S, H=H, W=W, C_=C, pool=pool, beta=beta)
    close(dx, xr.grad.permute(0, 2, 3, 1).reshape(-1, C) + beta)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("H,W,Hp,Wp", [(24, 20, 12, 10), (7, 5, 3, 2),
                                       (6, 6, 1, 1),        # a one-entry coarse grid: every fine row feeds row 0
                                       (5, 9, 1, 4),        # one coarse row, four columns
                                       (4, 4, 4, 4),        # the identity
                                       (3, 3, 5, 5),        # the "coarse" grid is the finer one
                                       (1, 1, 1, 1)])
def test_upsample_ac_backward_shapes(H, W, Hp, Wp, beta):
    """bilinear(align_corners=True) backward against the fp64 autograd of F.interpolate."""
    S, C = 2, 8
    xp = g(S, C, Hp, Wp, seed=75).requires_grad_(True)
    y = F.interpolate(xp, size=(H, W), mode="bilinear", align_corners=True)
    dy = g(*y.shape, seed=76)
    y.backward(dy)
    dxp = torch.ones(S * Hp * Wp, C, device=DEV) if beta else nan_out(S * Hp * Wp, C)
    TO.upsample_ac_backward_rows(dev(dy.permute(0, 2, 3, 1)), dxp, S=S, H=H, W=W, C_=C, Hp=Hp, Wp=Wp, beta=beta)
    close(dxp, xp.grad.permute(0, 2, 3, 1).reshape(-1, C) + beta)


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", [96, 200, 512, 768, 1000, 1024])     # VPL 2, 4, 8, 12, 16 (ragged), 16
def test_l2normalize_backward_widths(cols, rows):
    x = g(rows, cols, seed=77)
    dy = g(rows, cols, seed=78)
    xr = x.clone().requires_grad_(True)
    F.normalize(xr, dim=-1).backward(dy)
    dx = torch.ones(rows, cols, device=DEV)
    TO.l2normalize_backward(dev(x), dev(dy), dx, rows=rows, cols=cols, beta=1)
    close(dx, xr.grad + 1)


def test_l2normalize_backward_zero_row():
    """|x| <= eps: y = x / eps, so dx = dy / eps (the header's formula with y = 0)."""
    rows, cols, eps = 3, 96, 1e-12
    x = g(rows, cols, seed=79)
    x[1] = 0
    dy = g(rows, cols, seed=80)
    xr = x.clone().requires_grad_(True)
    F.normalize(xr, dim=-1).backward(dy)
    dx = nan_out(rows, cols)
    TO.l2normalize_backward(dev(x), dev(dy), dx, rows=rows, cols=cols, eps=eps)
    close(dx[1], dy[1] / eps)
    close(dx[0], xr.grad[0])
    close(dx[2], xr.grad[2])


@pytest.mark.parametrize("n", [4, 1028, 2 ** 20 + 4])       # one vector; one past a workgroup; one past 1024 workgroups
def test_axpby(n):
    x, y = g(n, seed=81), g(n, seed=82)
    xd, yd = dev(x), dev(y)
    out = nan_out(n)
    TO.axpby(xd, yd, out, alpha=0.75, beta=-1.5)
    close(out, 0.75 * x - 1.5 * y, 1e-6)
    out = nan_out(n)
    TO.axpby(xd, None, out, alpha=-2.5)
    close(out, -2.5 * x, 1e-6)
    TO.axpby(xd, yd, xd, alpha=0.5, beta=3.0)      # out is x: axpby(dXp, dout, dXp) of the pad token's backward
    close(xd, 0.5 * x + 3.0 * y, 1e-6)


@pytest.mark.parametrize("n", [1, 257, 70000])
def test_add_dev_scalar(n):
    """One fp32 add per element: the same bits as torch's."""
    x = g(n, seed=83).float()
    s = torch.tensor([0.3721], dtype=torch.float32)
    xd = x.to(DEV)
    TO.add_dev_scalar(xd, s.to(DEV))
    assert torch.equal(xd.cpu(), x + s)


@pytest.mark.parametrize("cols", [5, 512])
def test_scatter_rows(cols):
    """A copy: the named rows hold the input's bits, every other row keeps what it held."""
    idx = torch.tensor([7, 0, 11, 3, 19, 4], dtype=torch.int32)
    x = g(len(idx), cols, seed=84).float()
    out = nan_out(20, cols)
    TO.scatter_rows(x.to(DEV), idx.to(DEV), out)
    got = out.cpu()
    poison.check_bit_identical(got[idx.long()], x, "scatter_rows")
    rest = torch.ones(20, dtype=torch.bool)
    rest[idx.long()] = False
    assert poison.holds_fill(got[rest]).all(), "scatter_rows: a row that idx does not name was written"


@pytest.mark.parametrize("k", [2, 4])
def test_convt_gather_is_a_copy(k):
    """catseg_convt_gather on a 3 x 5 map (not square): g[(s, y, x)][(ky, kx, co)] = dout[s][y k + ky][x k + kx][co]."""
    S, hin, win, cout = 2, 3, 5, 8
    dout = g(S, hin * k, win * k, cout, seed=85).float()
    G = nan_out(S * hin * win, k * k * cout)
    TO.convt_gather(dout.to(DEV).reshape(-1, cout), G, S=S, hin=hin, win=win, k=k, cout=cout)
    want = dout.reshape(S, hin, k, win, k, cout).permute(0, 1, 3, 2, 4, 5).reshape(S * hin * win, k * k * cout)
    poison.check_bit_identical(G.cpu(), want.contiguous(), "convt_gather")


@pytest.mark.parametrize("k", [1, 3, 5, 7])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (5, 3), (7, 33)])       # maps narrower than the 16-pixel slab, and 2 slabs + 1
@pytest.mark.parametrize("cin,cout", [(20, 8), (3, 16), (64, 32)])       # vector / scalar cin; the data gradient of the
def test_conv2d_small_maps(cin, cout, H, W, k):                          # last on the 128 x 64 tile
    """Forward, data gradient and weight gradient on small maps with every kernel size, overwriting (into NaN)
    and as alpha = 0.5, beta = 1 (forward and weight gradient)."""
    S = 2
    x = g(S, cin, H, W, seed=86)
    w = g(cout, cin, k, k, seed=87) / math.sqrt(cin * k * k)
    b = g(cout, seed=88)
    xr, wr = (t.clone().requires_grad_(True) for t in (x, w))
    y = F.conv2d(xr, wr, b, padding=k // 2)
    dy = g(*y.shape, seed=89)
    y.backward(dy)
    yref = y.detach().permute(0, 2, 3, 1).reshape(-1, cout)
    xn = dev(x.permute(0, 2, 3, 1).reshape(-1, cin))
    wt = dev(w.permute(2, 3, 1, 0).reshape(k * k * cin, cout))         # [(tap, ci)][co]
    kw = dict(S=S, H=H, W=W, cin=cin, cout=cout, ksize=k)
    yd = nan_out(S * H * W, cout)
    TO.conv2d(xn, wt, yd, bias=dev(b), **kw)
    close(yd, yref, 1e-5)
    y0 = g(S * H * W, cout, seed=90)
    yd = dev(y0)
    TO.conv2d(xn, wt, yd, bias=dev(b), alpha=0.5, beta=1, **kw)
    close(yd, 0.5 * yref + y0, 1e-5)
    dyn = dev(dy.permute(0, 2, 3, 1).reshape(-1, cout))
    wref = wr.grad.permute(2, 3, 1, 0).reshape(k * k * cin, cout)
    dw = nan_out(k * k * cin, cout)
    TO.conv2d_wgrad(xn, dyn, dw, **kw)
    close(dw, wref)
    w0 = g(k * k * cin, cout, seed=91)
    dw = dev(w0)
    TO.conv2d_wgrad(xn, dyn, dw, alpha=0.5, beta=1, **kw)
    close(dw, 0.5 * wref + w0)
    if cin % 4 == 0:
        wf = dev(w.flip(2, 3).permute(2, 3, 0, 1).reshape(k * k * cout, cin))
        dx = nan_out(S * H * W, cin)
        TO.conv2d(dyn, wf, dx, S=S, H=H, W=W, cin=cout, cout=cin, ksize=k)
        close(dx, xr.grad.permute(0, 2, 3, 1).reshape(-1, cin))


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("H,W", [(5, 7), (24, 24), (32, 32)])      # pixels per thread: one; three, the last ragged; four
def test_corr_embed_backward_input(H, W, D, k):
    """The data gradient of corr_embed's Conv2d(1, D, k) against the autograd of F.conv2d."""
    S = 3
    corr = g(S, 1, H, W, seed=92).requires_grad_(True)
    w = g(D, 1, k, k, seed=93) / k
    dX = g(S, D, H, W, seed=94)
    F.conv2d(corr, w, padding=k // 2).backward(dX)
    dcorr = nan_out(S, H * W)
    TO.corr_embed_backward_input(dev(dX.permute(0, 2, 3, 1)).reshape(-1, D), dev(w), dcorr, S=S, H=H, W=W)
    close(dcorr, corr.grad.reshape(S, H * W))


def _head_conv_formula(x, dl, w):
    """The head conv's backward written out (any device): x (S, H, W, C), dl (S, H, W), w (9, C), tap t = (ky, kx) of
    y[p] = sum_t x[p + (ky - 1, kx - 1)] . w[t].  Returns dx (S, H, W, C) and dw (9, C)."""
    S, H, W, C = x.shape
    dlp = F.pad(dl, (1, 1, 1, 1))
    dx = torch.zeros_like(x)
    dw = torch.zeros_like(w)
    for t in range(9):
        ky, kx = t // 3, t % 3
        d = dlp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W].unsqueeze(-1)       # dl[q - (ky - 1, kx - 1)]
        dx += d * w[t]
        dw[t] = (d * x).sum((0, 1, 2))
    return dx, dw


@pytest.mark.parametrize("H,W", [(1, 1), (3, 7)])
@pytest.mark.parametrize("C", [4, 16, 64])
def test_head_conv_backward_channels(C, H, W):
    S = 5
    x = g(S, C, H, W, seed=95)
    w = g(1, C, 3, 3, seed=96) / math.sqrt(9 * C)
    xr, wr = (t.clone().requires_grad_(True) for t in (x, w))
    y = F.conv2d(xr, wr, padding=1)
    dl = g(*y.shape, seed=97)
    y.backward(dl)
    dx = nan_out(S * H * W, C)
    dw = nan_out(9, C)
    wt = w[0].permute(1, 2, 0).reshape(9, C)
    TO.head_conv_backward(dev(x.permute(0, 2, 3, 1)), dev(dl), dev(wt), dx, dw, S=S, H=H, W=W, C_=C)
    close(dx, xr.grad.permute(0, 2, 3, 1).reshape(-1, C))
    close(dw, wr.grad[0].permute(1, 2, 0).reshape(9, C))
    # the written-out formula the large case below is checked against agrees with autograd
    fx, fw = _head_conv_formula(x.permute(0, 2, 3, 1), dl[:, 0], wt)
    assert rel(fx.reshape(-1, C), xr.grad.permute(0, 2, 3, 1).reshape(-1, C)) < 1e-12
    assert rel(fw, wr.grad[0].permute(1, 2, 0).reshape(9, C)) < 1e-12


def test_head_conv_backward_grid_stride():
    """S H W C / 4 = 4 305 920 items on the HC_WG x 256 x 16 = 4 194 304 a capped grid covers in 16 visits per
    thread: the grid-stride loop makes a 17th.  The fp64 reference is the written-out formula on the device."""
    S, H, W, C = 5, 232, 232, 64
    gen = torch.Generator().manual_seed(98)
    x = torch.randn(S, H, W, C, generator=gen)
    dl = torch.randn(S, H, W, generator=gen)
    wt = torch.randn(9, C, generator=gen) / math.sqrt(9 * C)
    xd, dld, wd = x.to(DEV), dl.to(DEV), wt.to(DEV)
    dx = nan_out(S * H * W, C)
    dw = nan_out(9, C)
    TO.head_conv_backward(xd, dld, wd, dx, dw, S=S, H=H, W=W, C_=C)
    rx, rw = _head_conv_formula(xd.double(), dld.double(), wd.double())
    assert not torch.isnan(dx).any() and not torch.isnan(dw).any()
    ex = ((dx.double() - rx.reshape(-1, C)).abs().max() / rx.abs().max()).item()
    ew = ((dw.double() - rw).abs().max() / rw.abs().max()).item()
    assert ex <= 1e-4 and ew <= 1e-4, (ex, ew)
