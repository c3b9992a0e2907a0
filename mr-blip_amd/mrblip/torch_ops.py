"""The hot-path kernels as PyTorch custom operators: ``torch.ops.mrblip.*`` (``torch.library.custom_op`` + ``register_fake`` +
``register_autograd``), for callers that want the MI355X kernels inside an ordinary autograd graph — e.g. a maintainer of the reference
swapping ``nn.LayerNorm`` / ``T5LayerNorm`` / ``nn.Linear`` / the attention core / ``CrossEntropyLoss`` one module at a time before moving
to the whole-step engine.

The train step itself (mrblip/engine.py) does NOT go through these: it drives the same C-ABI entry points (mrblip/ops.py) with a
hand-written backward over pre-planned workspaces, because per-op autograd bookkeeping (one Python node, one output allocation and one
saved-tensor set per kernel) costs more than the 12-token decoder's kernels themselves.  These operators are the same kernels behind
the standard PyTorch extension point:

  mrblip::linear(x, w, bias?) -> y               bf16 [M,K] x bf16 [N,K]^T (+ fp32 bias) -> bf16 [M,N], fp32 accumulation; K, N % 64 == 0
  mrblip::layer_norm(x, gamma, beta, eps) -> y   fp32 [M,D] -> bf16 (eva_vit.py / Qformer.py LayerNorm under autocast)
  mrblip::rms_norm(x, weight, eps) -> y          fp32 [M,D] -> bf16 (modeling_t5.py:239-262 T5LayerNorm; weight frozen on this path)
  mrblip::attention(q, k, v, scale, bias_lut?, kmask?, causal) -> o     bf16 [B,S,H,D], D <= 64 for the backward
  mrblip::cross_entropy(logits, labels) -> loss  fp32 [R,V], int32 [R] (-100 = ignore) -> mean over valid rows, fp32 [1]
  mrblip::adamw_(p, g, m, v, hyper, ...)         in-place fused AdamW over flat fp32 buffers
  mrblip::grad_norm(g) -> (norm, nonfinite)      flat fp32 gradient -> (fp32 [1] global L2 norm, fp64-accumulated and bit-reproducible;
                                                 int32 [1] count of inf / nan values, norm = +inf when non-zero); no host synchronisation
  mrblip::gemm_(a, w, out, bias?, residual?, act, tile_cfg)   the raw fused GEMM, writing ``out`` in place
  mrblip::crop_resize_u8(src, boxes, out_size, frames_per_clip) -> dst   uint8 [.., 3, H, W] -> [.., 3, out, out]: one crop box per clip
                                                 (CPU int [n_clips, 4] of i, j, h, w) + bicubic resize; input augmentation, no autograd

  mrblip::decode_self_attention(kv_src, kv_dst, qkv, out, lut, layer, heads, pos, pos_dev?, parents?, scale)   one decoder layer's
                                                 single-query self-attention against the row-major K / V cache of an incremental decode:
                                                 re-orders by parents, appends the new position, writes kv_dst and out in place; no autograd

Every operator has a fake (meta) implementation, so FakeTensor tracing / torch.compile graph capture see shapes and dtypes without
running a kernel.  CUDA (= HIP) tensors only: there is no CPU fallback, by design.
"""
from typing import Optional, Tuple

import torch
from torch.library import custom_op

from . import ops

bf16, f32 = torch.bfloat16, torch.float32


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------ raw GEMM (in place)
@custom_op("mrblip::gemm_", mutates_args=("out",), device_types="cuda")
def gemm_(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
          act: int = 0, tile_cfg: int = 0) -> None:
    ops.gemm(a, w, out, bias=bias, residual=residual, act=act, tile_cfg=tile_cfg)


@gemm_.register_fake
def _(a, w, out, bias=None, residual=None, act=0, tile_cfg=0):
    return None


# ------------------------------------------------------------------------------------------------ linear
@custom_op("mrblip::linear", mutates_args=(), device_types="cuda")
def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    out = torch.empty(x.shape[0], w.shape[0], dtype=bf16, device=x.device)
    ops.gemm(_c(x), _c(w), out, bias=None if bias is None else bias.float())
    return out


@linear.register_fake
def _(x, w, bias=None):
    return x.new_empty(x.shape[0], w.shape[0])


@custom_op("mrblip::linear_backward", mutates_args=(), device_types="cuda")
def linear_backward(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, need_dw: bool, need_db: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    dy = _c(dy)
    dx = torch.empty_like(x)
    ops.gemm(dy, _c(w.t()), dx)                               # dX = dY W        (contraction over N: N % 64 == 0)
    dw = torch.zeros(w.shape if need_dw else (0,), dtype=f32, device=x.device)
    if need_dw:                                               # dW = dY^T X      (contraction over M, zero padded to a multiple of 64)
        M = x.shape[0]
        Mp = (M + 63) // 64 * 64
        dyt = torch.zeros(dy.shape[1], Mp, dtype=bf16, device=x.device)
        xt = torch.zeros(x.shape[1], Mp, dtype=bf16, device=x.device)
        dyt[:, :M] = dy.t()
        xt[:, :M] = x.t()
        ops.gemm(dyt, xt, dw)
    db = dy.float().sum(0) if need_db else torch.zeros(0, dtype=f32, device=x.device)
    return dx, dw, db


@linear_backward.register_fake
def _(dy, x, w, need_dw, need_db):
    return torch.empty_like(x), x.new_empty(w.shape if need_dw else (0,), dtype=f32), x.new_empty((w.shape[0],) if need_db else (0,), dtype=f32)


def _linear_setup(ctx, inputs, output):
    x, w, bias = inputs
    ctx.save_for_backward(x, w)
    ctx.has_bias = bias is not None


def _linear_bwd(ctx, dy):
    x, w = ctx.saved_tensors
    need_dw, need_db = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
    dx, dw, db = linear_backward(dy, x, w, need_dw, need_db)
    return dx, (dw.to(w.dtype) if need_dw else None), (db if need_db else None)


linear.register_autograd(_linear_bwd, setup_context=_linear_setup)


# ------------------------------------------------------------------------------------------------ norms
@custom_op("mrblip::layer_norm", mutates_args=(), device_types="cuda")
def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    out = torch.empty(x.shape, dtype=bf16, device=x.device)
    ops.layernorm_fwd(_c(x), gamma, beta, eps, out_bf16=out)
    return out


@layer_norm.register_fake
def _(x, gamma, beta, eps):
    return x.new_empty(x.shape, dtype=bf16)


@custom_op("mrblip::layer_norm_backward", mutates_args=(), device_types="cuda")
def layer_norm_backward(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    dx = torch.empty_like(x)
    dg, db = torch.zeros_like(gamma), torch.zeros_like(gamma)
    ops.layernorm_bwd(_c(dy.float()), _c(x), gamma, eps, dx, dgamma=dg, dbeta=db)
    return dx, dg, db


@layer_norm_backward.register_fake
def _(dy, x, gamma, eps):
    return torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)


def _ln_setup(ctx, inputs, output):
    x, gamma, beta, eps = inputs
    ctx.save_for_backward(x, gamma)
    ctx.eps = eps


def _ln_bwd(ctx, dy):
    x, gamma = ctx.saved_tensors
    dx, dg, db = layer_norm_backward(dy, x, gamma, ctx.eps)
    return dx, dg, db, None


layer_norm.register_autograd(_ln_bwd, setup_context=_ln_setup)


@custom_op("mrblip::rms_norm", mutates_args=(), device_types="cuda")
def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    out = torch.empty(x.shape, dtype=bf16, device=x.device)
    ops.rmsnorm_fwd(_c(x), weight, eps, out_bf16=out)
    return out


@rms_norm.register_fake
def _(x, weight, eps):
    return x.new_empty(x.shape, dtype=bf16)


@custom_op("mrblip::rms_norm_backward", mutates_args=(), device_types="cuda")
def rms_norm_backward(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    dx = torch.empty_like(x)
    ops.rmsnorm_bwd(_c(dy.float()), _c(x), weight, eps, dx)
    return dx


@rms_norm_backward.register_fake
def _(dy, x, weight, eps):
    return torch.empty_like(x)


def _rms_setup(ctx, inputs, output):
    x, weight, eps = inputs
    ctx.save_for_backward(x, weight)
    ctx.eps = eps


def _rms_bwd(ctx, dy):
    x, weight = ctx.saved_tensors
    if ctx.needs_input_grad[1]:
        raise RuntimeError("mrblip::rms_norm: the T5 norm weights are frozen on the Mr. BLIP path; no weight gradient kernel exists")
    return rms_norm_backward(dy, x, weight, ctx.eps), None, None


rms_norm.register_autograd(_rms_bwd, setup_context=_rms_setup)


# ------------------------------------------------------------------------------------------------ attention
@custom_op("mrblip::attention_forward", mutates_args=(), device_types="cuda")
def attention_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, bias_lut: Optional[torch.Tensor] = None,
                      kmask: Optional[torch.Tensor] = None, causal: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    q, k, v = _c(q), _c(k), _c(v)
    B, Sq, H, D = q.shape
    o = torch.empty_like(q)
    lse = torch.zeros(B, H, ops.rup32(Sq), dtype=f32, device=q.device)
    ops.attention_fwd(q, k, ops.head_transpose(v), o, lse, scale=scale, bias_lut=bias_lut, kmask=kmask, causal=causal)
    return o, lse


@attention_forward.register_fake
def _(q, k, v, scale, bias_lut=None, kmask=None, causal=False):
    B, Sq, H, D = q.shape
    return torch.empty_like(q), q.new_empty(B, H, (Sq + 31) // 32 * 32, dtype=f32)


@custom_op("mrblip::attention_backward", mutates_args=(), device_types="cuda")
def attention_backward(do: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, o: torch.Tensor, lse: torch.Tensor, scale: float,
                       bias_lut: Optional[torch.Tensor] = None, kmask: Optional[torch.Tensor] = None,
                       causal: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    do, q, k, v, o = _c(do.to(bf16)), _c(q), _c(k), _c(v), _c(o)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    ops.attention_bwd(q, k, v, o, do, ops.head_transpose(k), ops.head_transpose(q), ops.head_transpose(do), lse, torch.zeros_like(lse),
                      dq, dk, dv, scale=scale, bias_lut=bias_lut, kmask=kmask, causal=causal)
    return dq, dk, dv


@attention_backward.register_fake
def _(do, q, k, v, o, lse, scale, bias_lut=None, kmask=None, causal=False):
    return torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)


def _attn_setup(ctx, inputs, output):
    q, k, v, scale, bias_lut, kmask, causal = inputs
    o, lse = output
    ctx.save_for_backward(q, k, v, o, lse, bias_lut, kmask)
    ctx.scale, ctx.causal = scale, causal


def _attn_bwd(ctx, do, dlse):
    q, k, v, o, lse, bias_lut, kmask = ctx.saved_tensors
    dq, dk, dv = attention_backward(do, q, k, v, o, lse, ctx.scale, bias_lut, kmask, ctx.causal)
    return dq, dk, dv, None, None, None, None


attention_forward.register_autograd(_attn_bwd, setup_context=_attn_setup)


def attention(q, k, v, scale: float, bias_lut=None, kmask=None, causal: bool = False) -> torch.Tensor:
    """softmax(q k^T * scale + bias) v over [B,S,H,D] bf16 tensors.  bias_lut: fp32 [H,257] relative-position bias by
    clamp(key - query, -128, 128) + 128 (T5); kmask: int32 [B, rup32(Sk)], 1 = attend."""
    return torch.ops.mrblip.attention_forward(q, k, v, scale, bias_lut, kmask, causal)[0]


# ------------------------------------------------------------------------------------------------ loss, optimizer
@custom_op("mrblip::cross_entropy_forward", mutates_args=(), device_types="cuda")
def cross_entropy_forward(logits: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    logits = _c(logits)
    n_valid = int((labels != -100).sum())
    loss = torch.zeros(1, dtype=f32, device=logits.device)
    dlogits = torch.empty(logits.shape, dtype=bf16, device=logits.device)
    ops.cross_entropy(logits, _c(labels.to(torch.int32)), 1.0 / max(n_valid, 1), loss, dlogits)
    return loss, dlogits


@cross_entropy_forward.register_fake
def _(logits, labels):
    return logits.new_empty(1, dtype=f32), logits.new_empty(logits.shape, dtype=bf16)


def _ce_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _ce_bwd(ctx, dloss, _unused):
    (dlogits,) = ctx.saved_tensors
    return dlogits.float() * dloss, None


cross_entropy_forward.register_autograd(_ce_bwd, setup_context=_ce_setup)


def cross_entropy(logits, labels) -> torch.Tensor:
    """mean CE over rows whose label is not -100 (modeling_t5.py:1788-1792: CrossEntropyLoss(ignore_index=-100))"""
    return torch.ops.mrblip.cross_entropy_forward(logits, labels)[0]


@custom_op("mrblip::adamw_", mutates_args=("p", "m", "v"), device_types="cuda")
def adamw_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, hyper: torch.Tensor, beta1: float = 0.9, beta2: float = 0.999,
           eps: float = 1e-8, weight_decay: float = 0.0) -> None:
    """hyper: fp32 [4] on the device = (lr, 1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t), grad_scale)"""
    ops.adamw(p, g, m, v, hyper, beta1, beta2, eps, weight_decay)


@adamw_.register_fake
def _(p, g, m, v, hyper, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    return None


@custom_op("mrblip::grad_norm", mutates_args=(), device_types="cuda")
def grad_norm(g: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """ops.grad_norm: the global L2 norm of a flat fp32 gradient and its count of non-finite values (csrc/optim.hip).  No gradient."""
    norm, bad = ops.grad_norm(_c(g))
    return norm.clone(), bad.clone()


@grad_norm.register_fake
def _(g):
    return g.new_empty(1, dtype=f32), g.new_empty(1, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ input augmentation
@custom_op("mrblip::crop_resize_u8", mutates_args=(), device_types="cuda")
def crop_resize_u8(src: torch.Tensor, boxes: torch.Tensor, out_size: int, frames_per_clip: int = 0) -> torch.Tensor:
    """src: uint8 [n_clips, T, 3, H, W], or [F, 3, H, W] with frames_per_clip > 0; boxes: CPU int [n_clips, 4] (host values: they travel
    in the kernel arguments).  No gradient: the frames are data."""
    return ops.crop_resize_u8(_c(src), boxes, out_size, frames_per_clip=frames_per_clip or None)


@crop_resize_u8.register_fake
def _(src, boxes, out_size, frames_per_clip=0):
    return src.new_empty(tuple(src.shape[:-2]) + (out_size, out_size))


# ------------------------------------------------------------------------------------------------ incremental decode
@custom_op("mrblip::decode_self_attention", mutates_args=("kv_dst", "out"), device_types="cuda")
def decode_self_attention(kv_src: torch.Tensor, kv_dst: torch.Tensor, qkv: torch.Tensor, out: torch.Tensor, lut: torch.Tensor, layer: int,
                          heads: int, pos: int = 0, pos_dev: Optional[torch.Tensor] = None, parents: Optional[torch.Tensor] = None,
                          scale: float = 1.0) -> None:
    """ops.decode_self_attention: caches bf16 [2, layers, R, Lmax, heads * D]; with ``parents`` (int32 [R]) kv_dst is the other cache buffer,
    without it kv_dst must be kv_src's storage.  ``pos_dev`` (int32 [1]) replaces the host position ``pos``.  No gradient: inference only."""
    ops.decode_self_attention(kv_src, kv_dst, qkv, out, lut, layer, heads, pos=None if pos_dev is not None else pos, pos_dev=pos_dev,
                              parents=parents, scale=scale)


@decode_self_attention.register_fake
def _(kv_src, kv_dst, qkv, out, lut, layer, heads, pos=0, pos_dev=None, parents=None, scale=1.0):
    return None


OPS = ("gemm_", "linear", "linear_backward", "layer_norm", "layer_norm_backward", "rms_norm", "rms_norm_backward", "attention_forward",
       "attention_backward", "cross_entropy_forward", "adamw_", "crop_resize_u8", "decode_self_attention", "grad_norm")
