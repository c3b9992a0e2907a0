"""MrBlipEngine — the MI355X-native train step of Mr. BLIP / Chrono: ViT-g frame encoding -> ln_vision -> Q-Former ->
t5_proj (-> 32->1 mean pool) -> frame/timestamp interleave -> Flan-T5 encoder/decoder with LoRA -> CE loss, and the
hand-written backward (dX through T5, t5_proj, Q-Former; dW for LoRA A/B, t5_proj, ln_vision), all as launches of
the gfx950 kernels in libmrblip_hip.so over static workspaces: the dependency chain on the caller's stream, the next clip's frozen-ViT
forward on a look-ahead stream, weight-gradient / transposition work on a gradient side stream.  (Nothing synchronises or allocates
after the first step, so the chain could be captured in a hipGraph — measured to buy nothing: the pre-queued eager stream already runs
dependent launches 2.3 us apart, tools/graph_gap_probe.py.)

Follows the behaviour of ``BLIP2_MR.forward_mr`` (blip2_mr.py:433-570) and the modules it calls (eva_vit.py:324-340,
Qformer.py:804-965, modeling_t5.py:1734-1893, peft LoRA r=8).  Residual streams are fp32, GEMM/attention operands bf16,
accumulation fp32 (the reference's GPU path is fp16/bf16 autocast with fp32 residuals).
Frozen: ViT, Q-Former, query_tokens, T5 base weights.  Trainable: LoRA A/B, t5_proj.{weight,bias}, ln_vision.{weight,bias}
(SURVEY.md §3.1).
"""
from __future__ import annotations

import contextlib
import math
import os
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import ops
from .prompt import EncoderLayout, bias_lut

bf16, f32, f16 = torch.bfloat16, torch.float32, torch.float16


def pad64(n: int) -> int:
    return (n + 63) // 64 * 64


# experiment knobs: tile configs of the T5 ENCODER's GEMMs (M = B * S_enc rows), forward "qkv,o,wi,wo" / backward dX "wo,wi,o,qkv" (0 = auto)
_ENC_FWD_CFG = (tuple(int(x) for x in os.environ.get("MRB_ENC_FWD_CFG", "0,0,0,0").split(",")) + (0, 0, 0, 0))[:4]
_ENC_BWD_CFG = (tuple(int(x) for x in os.environ.get("MRB_ENC_BWD_CFG", "0,0,0,0").split(",")) + (0, 0, 0, 0))[:4]

# tile configs of the ViT qkv / proj / fc2 / fc1 GEMMs (0 = the library's own choice); MRB_VIT_CFG="q,p,f2,f1" overrides for experiments
_VIT_CFG = (tuple(int(x) for x in os.environ.get("MRB_VIT_CFG", "0,0,0,0").split(",")) + (0, 0, 0, 0))[:4]
# round 6: CU reserve PER ViT GEMM (qkv, proj, fc2, fc1) while the ViT runs as the look-ahead, -1 = the look-ahead's reserve.  The 4-wave kernel is
# persistent, one 256 x 256 tile per CU and round: 60 frames are 61 row tiles, so qkv = 1037, proj / fc2 = 366, fc1 = 1464 tiles, i.e. 6 / 2 / 8
# rounds on the 192 CUs a reserve of 64 leaves — but 5 rounds on 208 CUs (qkv) and 7 on 216 (fc1), and still 2 on 184 (proj / fc2).
_VIT_RSV = (tuple(int(x) for x in os.environ.get("MRB_VIT_RESERVE_BY_GEMM", "-1,-1,-1,-1").split(",")) + (-1, -1, -1, -1))[:4]


@dataclass
class EngineConfig:
    # ViT (eva_vit.py:415-428)
    img: int = 224
    patch: int = 14
    vit_dim: int = 1408
    vit_depth: int = 39
    vit_heads: int = 16
    vit_mlp: int = 6144
    # Q-Former (bert-base-uncased + blip2.py:46-61)
    qf_dim: int = 768
    qf_heads: int = 12
    qf_inter: int = 3072
    qf_layers: int = 12
    qf_cross_freq: int = 2
    num_query: int = 32
    qf_dropout: float = 0.1
    # T5 (google/flan-t5-xl)
    d_model: int = 2048
    d_kv: int = 64
    t5_heads: int = 32
    d_ff: int = 5120
    t5_layers: int = 24
    t5_dec_layers: int = 24
    vocab: int = 32128
    t5_eps: float = 1e-6
    t5_dropout: float = 0.1
    # LoRA (blip2_mr.py:193-200)
    lora_r: int = 8
    lora_alpha: float = 8.0
    lora_dropout: float = 0.05
    # peft draws one lora_dropout mask per ADAPTER (each LoRA Linear owns its nn.Dropout: blip2_mr.py:193-200 -> peft lora_dropout
    # ModuleDict).  False (default): the adapters of a fused projection group (q/k/v, wi_0/wi_1, cross k/v) share ONE mask of their
    # common input — same marginal distribution, one launch per group; True: a distinct mask per adapter, as peft, at the price of
    # per-adapter thin launches (measured: DESIGN.md §4).
    lora_mask_per_adapter: bool = False
    mean_pool: bool = False
    # Operand type of the frozen ViT's GEMMs and attention (round 4).  The reference's GPU arithmetic there is fp16 autocast over fp16
    # weights (blip2_mr.py:446; eva_vit.py:397-412, 439-441).  "fp16" runs the ViT on IEEE fp16 operands (v_mfma_f32_32x32x16_f16: 3 more
    # mantissa bits than bf16); "bf16" (default) as rounds 1-3; "auto" = fp16 where the fp16 kernels apply (every ViT GEMM on the 4-wave
    # 256x256 kernel, attention on the row-major-V form: head_dim in (64, 96], > 32 tokens — the real ViT-g/14), bf16 otherwise.
    # MEASURED (round 4, one box, alternating runs; profiles/r04_vit_fp16_vs_bf16.txt): the ViT output's error against the reference's fp32
    # run drops 8x (C1 6.1e-3 -> 7.7e-4, C2 5.2e-3 -> 6.9e-4) but the logits only 5-8 % (C2 9.4e-3 -> 8.9e-3: the Q-Former and T5 towers
    # dominate), while the step gets SLOWER: 73.0 vs 71.6 ms, fc1 275 vs 261 us exclusive — at the same MFMA rate the fp16 multipliers
    # draw more power and the chip, which runs every GEMM at its 1400 W cap, clocks lower.  Hence bf16 stays the default.
    # The residual stream is fp32 either way; ln_vision's output, which feeds the Q-Former, stays bf16 (the Q-Former's BACKWARD needs
    # bf16's exponent range for its gradient operands — the reference needs a GradScaler for the same reason: DESIGN.md §7).
    vit_operands: str = "bf16"

    @staticmethod
    def flan_t5_xl_qvh(**kw):
        return EngineConfig(**kw)

    @staticmethod
    def tiny(**kw):
        base = dict(img=56, vit_dim=96, vit_depth=2, vit_heads=4, vit_mlp=418, qf_dim=64, qf_heads=4, qf_inter=128, qf_layers=4,
                    num_query=8, d_model=64, d_kv=16, t5_heads=4, d_ff=128, t5_layers=2, t5_dec_layers=2)
        base.update(kw)
        return EngineConfig(**base)


# tile configuration of the Q-Former's cross K / V input-gradient GEMM [F * 257, 1408] x [1408, 1536]^T (0 = auto = the 4-wave 256x256 form;
# 14 = its 256x192 form: N = 1408 is 5.5 tiles of 256 but 7.3 of 192)
_QF_KV_BWD_CFG = int(os.environ.get("MRB_QF_KV_BWD_CFG", "0"))


class StateDictSource:
    """Weights by reference state-dict key (plain HF names or peft names for T5)."""

    def __init__(self, sd: Dict[str, torch.Tensor]):
        self.sd = sd

    def get(self, key: str, shape=None) -> torch.Tensor:
        if key in self.sd:
            return self.sd[key]
        for pre in ("t5_model.", "answerer_model."):      # (peft wraps both T5s of the video-QA variants the same way)
            if key.startswith(pre):
                k2 = pre + "base_model.model." + key[len(pre):]
                if k2 in self.sd:
                    return self.sd[k2]
                k3 = k2.replace(".weight", ".base_layer.weight")
                if k3 in self.sd:
                    return self.sd[k3]
        raise KeyError(key)

    def has(self, key: str) -> bool:
        try:
            self.get(key)
            return True
        except KeyError:
            return False


class RandomSource:
    """Seeded N(0, std) weights generated directly on the device (benchmark: no checkpoints in the container)."""

    def __init__(self, device, seed: int = 1234, std: float = 0.02):
        self.g = torch.Generator(device=device).manual_seed(seed)
        self.device, self.std = device, std

    def get(self, key: str, shape) -> torch.Tensor:
        leaf = key.rsplit(".", 1)[-1]
        lower = key.lower()
        if leaf == "weight" and ("norm" in lower or "ln_" in lower) and len(shape) == 1:
            return torch.ones(shape, device=self.device)
        if leaf in ("bias", "q_bias", "v_bias"):
            return torch.zeros(shape, device=self.device)
        return torch.randn(shape, device=self.device, generator=self.g) * self.std

    def has(self, key: str) -> bool:
        return True


@dataclass
class Adapter:
    name: str          # e.g. encoder.block.0.layer.0.SelfAttention.q
    in_dim: int
    out: int
    row0: int
    col0: int
    site: int
    A: torch.Tensor = None     # fp32 [8, in] view into the flat trainable buffer
    Bt: torch.Tensor = None    # fp32 [8, out]  (B transposed)
    dA: torch.Tensor = None
    dBt: torch.Tensor = None
    a_off: int = 0
    bt_off: int = 0


@dataclass
class LoraGroup:
    W: torch.Tensor            # bf16 [N, Kp]
    Wt: torch.Tensor           # bf16 [K, Np]  (for dX)
    N: int
    K: int
    adapters: List[Adapter] = field(default_factory=list)
    wext: torch.Tensor = None  # bf16 [N, 64] view: B (K-extension operand of the forward GEMM)
    acat: torch.Tensor = None  # bf16 [8*nad, K]: scale * A stacked ("down" operand)
    bblk: torch.Tensor = None  # bf16 [8*nad, N]: scale * B^T block-diagonal (operand of g = dy @ B)
    acatt: torch.Tensor = None  # bf16 [K, 64]: (scale * A)^T, K-extension operand of the dX GEMM
    site: int = 0              # lora_dropout site (one mask per group input)
    w_off: int = -1            # encoder groups: element offset of W in the engine's enc_w_arena
    wt_off: int = -1           # ... and of Wt in enc_wt_arena


def _with_attention_split(fn):
    """Run a decoder entry point with the engine's cross-block key-split workspace registered for the cross attention (csrc/attention.hip F_XS;
    thread-local on the C side), and unregister it afterwards: a direct ops.attention_* caller must never inherit a pointer into this engine."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **kw):
        if self.xs_ws is None:
            return fn(self, *a, **kw)
        ops.attention_split_workspace(self.xs_ws, self.xs_split)
        try:
            return fn(self, *a, **kw)
        finally:
            ops.attention_split_workspace(None)
    return wrapped


class MrBlipEngine:
    @torch.no_grad()
    def __init__(self, cfg: EngineConfig, src, device, lora_init: Optional[Callable] = None, seed: Optional[int] = 42,
                 t5_prefix: str = "t5_model.", share_towers: Optional["MrBlipEngine"] = None):
        """seed: dropout stream of THIS rank (the reference seeds every RNG with run.seed + rank, train.py:57-65); None = derive it
        from torch's current seed, which train.py's setup_seeds has already offset by the rank.
        t5_prefix / share_towers (round 6, video-QA): the ANSWERER of the two-stage path is a second T5 with its own LoRA under the keys
        ``answerer_model.*`` (blip2_mr.py:152-161, 206-236) over the SAME frozen ViT / Q-Former as the localizer: share_towers = the
        localizer's engine, whose packed ViT / Q-Former operands (and Q-Former dropout call sites) this engine then uses instead of
        packing its own copies; t5_proj / ln_vision are read from ``src`` again (nothing trains them in QA: blip2_mr.py:325-363 runs
        the frame path under no_grad)."""
        if seed is None:
            seed = int(torch.initial_seed()) & 0x7FFFFFFF
        self.cfg, self.dev = cfg, device
        self.ws: Dict[str, torch.Tensor] = {}
        self.enc_t_saved: Dict[int, bool] = {}    # encoder layer -> Q^T / K^T were written by the forward's qkv GEMM
        self.dec_t_saved: Dict[int, bool] = {}    # decoder layer -> Q^T / K^T of its self-attention were written by the forward's fused projection
        # round 4: workspace of the cross-block key split of the decoder's cross attention (csrc/attention.hip F_XS): tickets (zero) + partials
        # (40 MB: up to 4 clips x 32 heads x 8 chunks of partials)
        self.xs_ws = torch.zeros(10 * 1024 * 1024, dtype=torch.int32, device=self.dev) if os.environ.get("MRB_ATTN_XS", "1") == "1" else None
        self.xs_split = int(os.environ.get("MRB_ATTN_XS_N", "0"))
        self.dec_tc_saved: Dict[int, bool] = {}   # ... and the cross-attention's Q^T
        self._store: Dict[str, torch.Tensor] = {}
        self.ws_allocation_log: List[tuple] = []
        self.training = True
        self.seed = torch.tensor([seed & 0x7FFFFFFF], dtype=torch.int32, device=device)
        self.hyper = torch.tensor([0.0, 1.0, 1.0, 1.0], dtype=f32, device=device)
        self.opt_step = 0
        self.probe = None
        self.vit_chunk = 1 << 20  # frames per ViT pass (chunking measured slower on MI355X: fewer tiles per launch; kept as a knob)
        self._site = 100
        inner = cfg.t5_heads * cfg.d_kv
        for nm, v in (("d_model", cfg.d_model), ("t5 inner", inner), ("d_ff", cfg.d_ff), ("qf_dim", cfg.qf_dim), ("qf_inter", cfg.qf_inter)):
            assert v % 64 == 0, f"{nm} must be a multiple of 64 (got {v})"
        assert cfg.vit_dim % 8 == 0 and (cfg.vit_dim // cfg.vit_heads) % 8 == 0 and cfg.vit_dim // cfg.vit_heads <= 96
        self.t5_prefix = t5_prefix
        if share_towers is None:
            self._build_vit(src)
            self._build_qformer(src)
        else:
            o = share_towers
            assert o.cfg.vit_dim == cfg.vit_dim and o.cfg.qf_dim == cfg.qf_dim and o.cfg.img == cfg.img and o.dev == self.dev
            self.vit_kpad, self.vit_fp, self.vit_dtype, self.vit = o.vit_kpad, o.vit_fp, o.vit_dtype, o.vit
            self.qf, self.ln_vision_eps, self.qf_emb_site = o.qf, o.ln_vision_eps, o.qf_emb_site
            self._site = o._site_after_towers
        self._site_after_towers = self._site
        self._build_t5(src, lora_init)

    # ------------------------------------------------------------------------------------------ utilities
    def buf(self, name: str, shape, dtype, zero: bool = True) -> torch.Tensor:
        """Named workspace of the step.  CAPACITY based: the backing store of a name is allocated once (zero-filled) for the largest
        size asked for so far — times ``ws_headroom``, which the caller raises before the first step when it knows that later steps
        will be longer (``reserve``) — and every request gets a contiguous VIEW of its leading elements.  The sequence length of the
        T5 encoder follows the query's token count (blip2_mr.py:572-824), so S changes on nearly every step of a real run: no
        allocation, no zero-fill and no host synchronisation happens after the longest shape has been seen.

        Why views are safe for the zero-padded operands: padding is either COLUMN padding at fixed positions of a row (K padded to
        64, the 8 n_adapter columns of the [M, 64] LoRA activations: never written, so they stay at their initial zeros whatever the
        row count), or it is written by the producing kernel itself on every call (head_transpose writes the whole [DP, Spad] tile
        with zeros outside the tensor, and so does the fused decoder projection for the head-transposed copies it emits: csrc/decproj.hip;
        pad_mask builds a fresh mask), or it is never read (LSE / Delta / keep-bit rows past Sq)."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for v in shape:
            n *= v
        store = self._store.get(name)
        if store is None or store.dtype != dtype or store.numel() < n:
            cap = max(n, int(n * self.ws_headroom)) if store is None else max(n, int(store.numel() * 1.25))
            store = torch.zeros(cap, dtype=dtype, device=self.dev)
            self._store[name] = store
            self.ws_allocations += 1
            self.ws_allocation_log.append((name, cap))
            # the zero fill runs on the CURRENT stream, but workspaces are shared by the engine's streams (gradient side stream,
            # ViT look-ahead stream): a buffer created on the main stream and first written on a side stream could be zeroed AFTER
            # that write (seen as a wrong first-step loss when two ranks shared one GPU); and a store that is REPLACED may still be
            # read by queued kernels.  (Re)allocation happens once per buffer (first step / a new longest shape), so simply let
            # everything finish before anything else is enqueued.
            torch.cuda.synchronize(self.dev)
        t = self.ws.get(name)
        if t is None or tuple(t.shape) != shape or t.dtype != dtype or t.untyped_storage().data_ptr() != store.untyped_storage().data_ptr():
            t = store[:n].view(shape)
            self.ws[name] = t
        return t

    ws_headroom = 1.0      # over-allocation factor of workspaces created from now on (see reserve)
    ws_allocations = 0     # (re)allocations so far: constant after warm-up, also over a stream of different sequence lengths

    def reserve(self, S: int, S_max: int, Ld: int = 1, Ld_max: int = 1):
        """Call before the first step (whose encoder / decoder lengths are S / Ld) when later steps can be as long as S_max / Ld_max:
        every workspace the first step creates is over-allocated so that the longest step fits.  Workspaces grow with S (rows), a
        few with S^2 (attention keep bits) or S * Ld (cross-attention) — one factor covers them all; it multiplies ~3 GB of
        activations of the QVH step by ~1.2 (max_txt_len 200 against a 40-token query), against 288 GB of HBM."""
        rs = max(1.0, (S_max + 31) // 32 * 32 / max(S, 1))
        rl = max(1.0, (Ld_max + 31) // 32 * 32 / max((Ld + 31) // 32 * 32, 1)) if Ld_max > Ld else 1.0
        self.ws_headroom = max(self.ws_headroom, rs * rs, rs * rl) * 1.01

    def h2d(self, t: torch.Tensor, dtype=None) -> torch.Tensor:
        """small host tensor -> device WITHOUT stalling the host on the stream (a pageable copy makes the host wait until the stream
        reaches it, i.e. until everything enqueued so far has run): pinned staging buffer + non_blocking copy"""
        if t.is_cuda:
            return t if dtype is None else t.to(dtype)
        if dtype is not None:
            t = t.to(dtype)
        return t.contiguous().pin_memory().to(self.dev, non_blocking=True)

    def new_site(self) -> int:
        self._site += 1
        return self._site

    def drop(self, site: int, p: float):
        return ops.Dropout(self.seed, site, p) if (self.training and p > 0) else None

    # Frame-sharded mode (dist.FrameShard.attach): the ranks of a shard group share ONE dropout seed (the T5 is replicated and must draw the
    # same masks everywhere), but each rank's LOCAL frames start at row 0 of its Q-Former buffers — with the shared seed the ranks would
    # draw identical Q-Former masks for different frames.  The Q-Former's call-site ids are therefore salted per rank (0 outside that mode).
    qf_site_salt = 0

    def qdrop(self, site: int, p: float):
        return self.drop(site + self.qf_site_salt, p)

    def _w(self, w: torch.Tensor, n_pad: Optional[int] = None, dtype=bf16) -> torch.Tensor:
        """fp32 [N,K] -> bf16 (or fp16) [Np, pad64(K)] zero padded"""
        N, K = w.shape
        Np = n_pad or N
        out = torch.zeros(Np, pad64(K), dtype=dtype, device=self.dev)
        out[:N, :K] = w.to(self.dev)
        return out

    def _v(self, v: torch.Tensor, n_pad: Optional[int] = None) -> torch.Tensor:
        out = torch.zeros(n_pad or v.numel(), dtype=f32, device=self.dev)
        out[: v.numel()] = v.to(self.dev).float().reshape(-1)
        return out

    @staticmethod
    def v4(t2d: torch.Tensor, B: int, S: int, H: int, D: int, col0: int = 0) -> torch.Tensor:
        """[B*S, ld] buffer -> strided [B,S,H,D] view of columns col0 .. col0+H*D"""
        ld = t2d.stride(0)
        return torch.as_strided(t2d, (B, S, H, D), (S * ld, ld, D, 1), t2d.storage_offset() + col0)

    # ------------------------------------------------------------------------------------------ ViT (frozen)
    def _build_vit(self, src):
        c = self.cfg
        D, P = c.vit_dim, c.patch
        p = "visual_encoder."
        self.vit_kpad = pad64(3 * P * P)
        self.vit_fp = pad64(c.vit_mlp)
        hd, T = D // c.vit_heads, (c.img // P) ** 2 + 1
        fp16_ok = 64 < hd <= 96 and T > 32 and self.vit_rowv
        assert c.vit_operands in ("auto", "fp16", "bf16"), c.vit_operands
        if c.vit_operands == "fp16" and not fp16_ok:
            raise ValueError(f"vit_operands='fp16' needs the row-major-V attention form (head_dim in (64, 96], > 32 tokens): got head_dim {hd}, {T} tokens")
        want16 = c.vit_operands != "bf16" or os.environ.get("MRB_VIT_FP16", "0") == "1"      # (MRB_VIT_FP16=1: A/B switch of the bench)
        self.vit_dtype = f16 if (want16 and fp16_ok) else bf16
        vt = self.vit_dtype
        _w0 = self._w
        self._w = lambda w, n_pad=None: _w0(w, n_pad, vt)     # (the ViT's packed GEMM operands only; restored below)
        self.vit = dict(
            pe_w=self._w(src.get(p + "patch_embed.proj.weight", (D, 3, P, P)).reshape(D, -1)),
            pe_b=self._v(src.get(p + "patch_embed.proj.bias", (D,))),
            cls=self._v(src.get(p + "cls_token", (1, 1, D))),
            pos=src.get(p + "pos_embed", (1, (c.img // P) ** 2 + 1, D)).to(self.dev).float().reshape(-1, D).contiguous(),
            blocks=[],
        )
        for i in range(c.vit_depth):
            q = p + f"blocks.{i}."
            qb, vb = src.get(q + "attn.q_bias", (D,)), src.get(q + "attn.v_bias", (D,))
            self.vit["blocks"].append(dict(
                n1w=self._v(src.get(q + "norm1.weight", (D,))), n1b=self._v(src.get(q + "norm1.bias", (D,))),
                qkv_w=self._w(src.get(q + "attn.qkv.weight", (3 * D, D))),
                qkv_b=self._v(torch.cat([qb.float().cpu(), torch.zeros(D), vb.float().cpu()])),
                proj_w=self._w(src.get(q + "attn.proj.weight", (D, D))), proj_b=self._v(src.get(q + "attn.proj.bias", (D,))),
                n2w=self._v(src.get(q + "norm2.weight", (D,))), n2b=self._v(src.get(q + "norm2.bias", (D,))),
                fc1_w=self._w(src.get(q + "mlp.fc1.weight", (c.vit_mlp, D)), self.vit_fp), fc1_b=self._v(src.get(q + "mlp.fc1.bias", (c.vit_mlp,)), self.vit_fp),
                fc2_w=self._w(src.get(q + "mlp.fc2.weight", (D, c.vit_mlp))), fc2_b=self._v(src.get(q + "mlp.fc2.bias", (D,))),
            ))
        del self._w   # back to the class method (bf16)

    @torch.no_grad()
    def vit_forward(self, video: torch.Tensor, n_blocks: Optional[int] = None, slot: int = 0, blocks: Optional[tuple] = None) -> torch.Tensor:
        """video fp32 [F,3,IMG,IMG] -> fp32 [F*(NP+1), D] (no final norm, eva_vit.py:324-340).  No activations are kept (the ViT is
        frozen and its output needs no gradient).  Frames are independent through the ViT; ``vit_chunk`` optionally processes them in
        groups (measured on MI355X: one pass over all frames is fastest — larger GEMMs beat Infinity-Cache residency)."""
        c = self.cfg
        F_ = video.shape[0]
        T = (c.img // c.patch) ** 2 + 1
        x_all = self.buf("vit_x" if slot == 0 else f"vit_x{slot}", (F_ * T, c.vit_dim), f32, zero=False)
        chunk = max(1, min(F_, self.vit_chunk))
        for f0 in range(0, F_, chunk):
            f1 = min(F_, f0 + chunk)
            self._vit_chunk(video[f0:f1], x_all[f0 * T: f1 * T], n_blocks, blocks)
        return x_all

    def _vit_chunk(self, video: torch.Tensor, x: torch.Tensor, n_blocks: Optional[int], blocks: Optional[tuple] = None):
        """blocks = (b0, b1): run only transformer blocks b0..b1-1 on the residual stream already in ``x`` (b0 > 0 skips the patch
        embedding) — the look-ahead runs a prefix of the ViT beside the decoder and the next step finishes it."""
        c, v = self.cfg, self.vit
        F_ = video.shape[0]
        G = c.img // c.patch
        NP, D, H = G * G, c.vit_dim, c.vit_heads
        hd = D // H
        T = NP + 1
        M = F_ * T
        tag = f"_{F_}"
        b0, b1 = blocks if blocks is not None else (0, c.vit_depth if n_blocks is None else n_blocks)
        vt_ = self.vit_dtype   # bf16, or IEEE fp16 (cfg.vit_operands)
        if b0 == 0:
            patches = self.buf("vit_patches" + tag, (F_ * NP, self.vit_kpad), vt_, zero=False)
            ops.patchify(video, patches, c.patch)
            pe = self.buf("vit_pe" + tag, (F_ * NP, D), f32, zero=False)
            ops.gemm(patches, v["pe_w"], pe, bias=v["pe_b"])
            ops.vit_assemble(pe, v["cls"], v["pos"], x.view(F_, T, D))
        h = self.buf("vit_h" + tag, (M, pad64(D)), vt_)
        qkv = self.buf("vit_qkv" + tag, (M, 3 * D), vt_, zero=False)
        o = self.buf("vit_o" + tag, (M, pad64(D)), vt_)
        f = self.buf("vit_f" + tag, (M, self.vit_fp), vt_, zero=False)
        vt = self.buf("vit_vt" + tag, (F_, H, ops.rup32(hd), ops.rup32(T)), bf16) if vt_ == bf16 else None
        q4, k4, v4 = self.v4(qkv, F_, T, H, hd, 0), self.v4(qkv, F_, T, H, hd, D), self.v4(qkv, F_, T, H, hd, 2 * D)
        o4 = self.v4(o, F_, T, H, hd)
        scale = hd ** -0.5
        probe = getattr(self, "probe", None)
        ctx_rsv = getattr(ops._tls, "cu_reserve", 0)
        rsv = [(r if (r >= 0 and ctx_rsv > 0) else None) for r in _VIT_RSV]     # (only beside another stream: an exclusive ViT pass keeps the whole chip)
        for blk in v["blocks"][b0:b1]:
            ops.layernorm_fwd(x, blk["n1w"], blk["n1b"], 1e-6, out_bf16=h)
            ops.gemm(h, blk["qkv_w"], qkv, bias=blk["qkv_b"], tile_cfg=_VIT_CFG[0], cu_reserve=rsv[0])
            if self.vit_rowv and hd > 64 and T > 32:   # V read row-major from the qkv buffer (LDS transpose reads): no V^T copy
                ops.attention_fwd_rowv(q4, k4, v4, o4, None, scale=scale)
            else:
                ops.head_transpose(v4, out=vt)
                ops.attention_fwd(q4, k4, vt, o4, None, scale=scale)
            ops.gemm(o, blk["proj_w"], x, bias=blk["proj_b"], residual=x, tile_cfg=_VIT_CFG[1], cu_reserve=rsv[1])
            ops.layernorm_fwd(x, blk["n2w"], blk["n2b"], 1e-6, out_bf16=h)
            if probe is not None:  # HIP events around the dominant kernel's launch (bench.py roofline.achieved)
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            ops.gemm(h, blk["fc1_w"], f, bias=blk["fc1_b"], act=1, tile_cfg=_VIT_CFG[3], cu_reserve=rsv[3])
            if probe is not None:
                ev[1].record()
                probe.append(ev)
            ops.gemm(f, blk["fc2_w"], x, bias=blk["fc2_b"], residual=x, tile_cfg=_VIT_CFG[2], cu_reserve=rsv[2])

    # ------------------------------------------------------------------------------------------ Q-Former (frozen weights, dX needed)
    def _build_qformer(self, src):
        c = self.cfg
        D, Dv, I = c.qf_dim, c.vit_dim, c.qf_inter
        p = "Qformer.bert."
        g = lambda k, s: src.get(p + k, s)  # noqa: E731
        self.qf = dict(
            query=src.get("query_tokens", (1, c.num_query, D)).to(self.dev).float().reshape(c.num_query, D).contiguous(),
            emb_w=self._v(g("embeddings.LayerNorm.weight", (D,))), emb_b=self._v(g("embeddings.LayerNorm.bias", (D,))),
            layers=[],
        )

        def att(pref, kv_dim):
            qw, kw, vw = g(pref + "self.query.weight", (D, D)), g(pref + "self.key.weight", (D, kv_dim)), g(pref + "self.value.weight", (D, kv_dim))
            qb, kb, vb = g(pref + "self.query.bias", (D,)), g(pref + "self.key.bias", (D,)), g(pref + "self.value.bias", (D,))
            ow = g(pref + "output.dense.weight", (D, D))
            d = dict(ob=self._v(g(pref + "output.dense.bias", (D,))), ow=self._w(ow), owt=self._w(ow.t()),
                     lnw=self._v(g(pref + "output.LayerNorm.weight", (D,))), lnb=self._v(g(pref + "output.LayerNorm.bias", (D,))),
                     sites=(self.new_site(), self.new_site()))
            if kv_dim == D:  # self-attention: fused q,k,v
                w = torch.cat([qw, kw, vw]).float()
                d.update(qkv_w=self._w(w), qkv_wt=self._w(w.t()), qkv_b=self._v(torch.cat([qb, kb, vb])))
            else:
                w = torch.cat([kw, vw]).float()
                d.update(q_w=self._w(qw), q_wt=self._w(qw.t()), q_b=self._v(qb), kv_w=self._w(w), kv_wt=self._w(w.t()), kv_b=self._v(torch.cat([kb, vb])))
            return d

        self.ln_vision_eps = 1e-5
        for i in range(c.qf_layers):
            l = f"encoder.layer.{i}."
            iw, ow = g(l + "intermediate_query.dense.weight", (I, D)), g(l + "output_query.dense.weight", (D, I))
            self.qf["layers"].append(dict(
                self=att(l + "attention.", D),
                cross=att(l + "crossattention.", Dv) if i % c.qf_cross_freq == 0 else None,
                iw=self._w(iw), iwt=self._w(iw.t()), ib=self._v(g(l + "intermediate_query.dense.bias", (I,))),
                ow=self._w(ow), owt=self._w(ow.t()), ob=self._v(g(l + "output_query.dense.bias", (D,))),
                lnw=self._v(g(l + "output_query.LayerNorm.weight", (D,))), lnb=self._v(g(l + "output_query.LayerNorm.bias", (D,))),
                site=self.new_site(),
            ))
        self.qf_emb_site = self.new_site()

    @torch.no_grad()
    def qformer_forward(self, img: torch.Tensor, F_: int) -> torch.Tensor:
        """img: bf16 [F*Tv, pad64(Dv)] (ln_vision output).  Returns the bf16 [F*nq, pad64(D)] last hidden state; keeps what
        the backward needs in the workspace."""
        c = self.cfg
        D, H, nq, I = c.qf_dim, c.qf_heads, c.num_query, c.qf_inter
        hd = D // H
        Mq = F_ * nq
        Tv = img.shape[0] // F_
        eps, pdrop = 1e-12, c.qf_dropout
        scale = 1.0 / math.sqrt(hd)
        q_exp = self.buf("qf_qexp", (Mq, D), f32, zero=False)
        q_exp.view(F_, nq, D).copy_(self.qf["query"])
        x = self.buf("qf_x0", (Mq, D), f32, zero=False)
        ops.layernorm_fwd(q_exp, self.qf["emb_w"], self.qf["emb_b"], eps, out_f32=x)
        xb = self.buf("qf_xb0", (Mq, pad64(D)), bf16)
        ops.cast_dropout(x, out_bf16=xb, out_f32=x, drop=self.qdrop(self.qf_emb_site, pdrop))
        if self._qf_fused_ok():
            return self._qformer_forward_fused(img, F_, x)
        vt_s = self.buf("qf_vt_s", (F_, H, ops.rup32(hd), ops.rup32(nq)), bf16)
        vt_c = self.buf("qf_vt_c", (F_, H, ops.rup32(hd), ops.rup32(Tv)), bf16)
        t_ok = self.tout_ok(hd, F_, nq, 4)
        want_t = bool(self.gemm_tout_sites & 8)   # the transposed Q / K copies of the forward are kept for the backward (eval / generate pay a few MB for them)
        self.qf_t_saved = t_ok and want_t
        # Round 4: the cross-attention K / V projections of the image tokens ([F * 257, 1408] x [1408, 1536] per cross layer: the only big
        # GEMMs of the Q-Former, 70 us each) depend on nothing but ``img``: they (and their V^T copies) are issued on the side stream at
        # entry and run beside the chain of small query-side kernels, each cross layer waits for its own event.  This phase runs with the
        # chip to itself (the look-ahead ViT starts behind the encoder forward), so what is hidden here comes off the step 1:1.
        kv_ready = {}
        self.qf_kt_saved = False
        if self.qf_kv_side and self.grad_side_stream_enabled:
            st, ev0 = self._grad_stream(), torch.cuda.Event()
            ev0.record()
            with torch.cuda.stream(st):
                st.wait_event(ev0)
                for i, L in enumerate(self.qf["layers"]):
                    if L["cross"] is None:
                        continue
                    C_ = L["cross"]
                    kv = self.buf(f"qf{i}_kvc", (F_ * Tv, 2 * D), bf16, zero=False)
                    vt_i = self.buf(f"qf{i}_vt_c", (F_, H, ops.rup32(hd), ops.rup32(Tv)), bf16)
                    ops.gemm(img, C_["kv_w"], kv, bias=C_["kv_b"])
                    ops.head_transpose(self.v4(kv, F_, Tv, H, hd, D), out=vt_i)
                    ev = torch.cuda.Event()
                    ev.record()
                    kv_ready[i] = (kv, vt_i, ev)
                if want_t and self.qf_kt_fwd and getattr(self, "_qf_backward_follows", False):
                    # round 6: the cross-attention K^T copies of the BACKWARD are written here, behind every layer's K / V^T (nothing of the forward
                    # waits for them), instead of by six launches on the backward's dependent chain; the backward waits for ONE event
                    for i, (kv, _, _) in kv_ready.items():
                        ops.head_transpose(self.v4(kv, F_, Tv, H, hd, 0), out=self.buf(f"qf{i}_kt_c", (F_, H, ops.rup32(hd), ops.rup32(Tv)), bf16))
                    self._qf_kt_event = torch.cuda.Event()
                    self._qf_kt_event.record()
                    self.qf_kt_saved = True
        # the query chain's GEMMs are 10-40 us each and every weight is touched once: each launch carries prefetch workgroups for the NEXT
        # launch's weights (see enc_prefetch; stand-alone o 13.3 -> 11.2, fc2 37.9 -> 28.8 us on cold weights)
        chain = []
        for L in self.qf["layers"]:
            chain += [L["self"]["qkv_w"], L["self"]["ow"]] + ([L["cross"]["q_w"], L["cross"]["ow"]] if L["cross"] is not None else []) + [L["iw"], L["ow"]]
        nxt_w = {id(a): b for a, b in zip(chain, chain[1:])}

        def pf(w):
            n = nxt_w.get(id(w)) if self.qf_prefetch else None
            if n is not None:
                ops.gemm_prefetch(n, n_blocks=16 if n.numel() < 2**20 else 32)
        for i, L in enumerate(self.qf["layers"]):
            S_ = L["self"]
            qkv = self.buf(f"qf{i}_qkv", (Mq, 3 * D), bf16, zero=False)
            q4, k4, v4 = self.v4(qkv, F_, nq, H, hd, 0), self.v4(qkv, F_, nq, H, hd, D), self.v4(qkv, F_, nq, H, hd, 2 * D)
            if t_ok:   # the projection writes V^T for this layer's attention and Q^T / K^T for its backward
                keep = want_t and i > 0   # (layer 0's self-attention has no backward: it only feeds the frozen query tokens)
                qt_i = self.buf(f"qf{i}_qt_s", (F_, H, 64, ops.rup32(nq)), bf16) if keep else None
                kt_i = self.buf(f"qf{i}_kt_s", (F_, H, 64, ops.rup32(nq)), bf16) if keep else None
                pf(S_["qkv_w"])
                ops.gemm(xb, S_["qkv_w"], qkv, bias=S_["qkv_b"], tout=(qt_i, kt_i, vt_s), t_rows=nq)
            else:
                pf(S_["qkv_w"])
                ops.gemm(xb, S_["qkv_w"], qkv, bias=S_["qkv_b"])
                ops.head_transpose(v4, out=vt_s)
            o = self.buf(f"qf{i}_o", (Mq, pad64(D)), bf16)
            lse = self.buf(f"qf{i}_lse", (F_, H, ops.rup32(nq)), f32)
            ops.attention_fwd(q4, k4, vt_s, self.v4(o, F_, nq, H, hd), lse, scale=scale, drop=self.qdrop(S_["sites"][0], pdrop))
            y = self.buf(f"qf{i}_y", (Mq, D), f32, zero=False)
            pf(S_["ow"])
            ops.gemm(o, S_["ow"], y, bias=S_["ob"], residual=x, drop=self.qdrop(S_["sites"][1], pdrop))
            x = self.buf(f"qf{i}_x1", (Mq, D), f32, zero=False)
            xb = self.buf(f"qf{i}_x1b", (Mq, pad64(D)), bf16)
            ops.layernorm_fwd(y, S_["lnw"], S_["lnb"], eps, out_bf16=xb, out_f32=x)
            if L["cross"] is not None:
                C_ = L["cross"]
                qc = self.buf(f"qf{i}_qc", (Mq, D), bf16, zero=False)
                pf(C_["q_w"])
                if t_ok and want_t:   # ... and the cross-attention's Q^T
                    ops.gemm(xb, C_["q_w"], qc, bias=C_["q_b"], tout=(self.buf(f"qf{i}_qt_c", (F_, H, 64, ops.rup32(nq)), bf16),), t_rows=nq)
                else:
                    ops.gemm(xb, C_["q_w"], qc, bias=C_["q_b"])
                if i in kv_ready:
                    kv, vt_c, ev = kv_ready[i]
                    torch.cuda.current_stream().wait_event(ev)
                    k4 = self.v4(kv, F_, Tv, H, hd, 0)
                else:
                    kv = self.buf(f"qf{i}_kvc", (F_ * Tv, 2 * D), bf16, zero=False)
                    ops.gemm(img, C_["kv_w"], kv, bias=C_["kv_b"])
                    k4, v4 = self.v4(kv, F_, Tv, H, hd, 0), self.v4(kv, F_, Tv, H, hd, D)
                    ops.head_transpose(v4, out=vt_c)
                oc = self.buf(f"qf{i}_oc", (Mq, pad64(D)), bf16)
                lsec = self.buf(f"qf{i}_lsec", (F_, H, ops.rup32(nq)), f32)
                ops.attention_fwd(self.v4(qc, F_, nq, H, hd), k4, vt_c, self.v4(oc, F_, nq, H, hd), lsec, scale=scale, drop=self.qdrop(C_["sites"][0], pdrop))
                y2 = self.buf(f"qf{i}_y2", (Mq, D), f32, zero=False)
                pf(C_["ow"])
                ops.gemm(oc, C_["ow"], y2, bias=C_["ob"], residual=x, drop=self.qdrop(C_["sites"][1], pdrop))
                x = self.buf(f"qf{i}_x2", (Mq, D), f32, zero=False)
                xb = self.buf(f"qf{i}_x2b", (Mq, pad64(D)), bf16)
                ops.layernorm_fwd(y2, C_["lnw"], C_["lnb"], eps, out_bf16=xb, out_f32=x)
            hact = self.buf(f"qf{i}_hact", (Mq, pad64(I)), bf16, zero=False)
            hpre = self.buf(f"qf{i}_hpre", (Mq, pad64(I)), bf16, zero=False)
            pf(L["iw"])
            ops.gemm(xb, L["iw"], hact, bias=L["ib"], act=1, out2=hpre)
            y3 = self.buf(f"qf{i}_y3", (Mq, D), f32, zero=False)
            pf(L["ow"])
            ops.gemm(hact, L["ow"], y3, bias=L["ob"], residual=x, drop=self.qdrop(L["site"], pdrop))
            x = self.buf(f"qf{i}_x3", (Mq, D), f32, zero=False)
            xb = self.buf(f"qf{i}_x3b", (Mq, pad64(D)), bf16)
            ops.layernorm_fwd(y3, L["lnw"], L["lnb"], eps, out_bf16=xb, out_f32=x)
        self._qf_last_f32 = x
        return xb

    # Round 6: one launch per Q-Former layer (csrc/qformer.hip: a workgroup owns one frame's 32 query tokens through the whole layer) instead
    # of the chain of 7 / 11 launches above.  BERT-base geometry only (the real Q-Former).  Built, parity-tested against the chain
    # (tests/test_qformer_fused_gpu.py) and MEASURED SLOWER — off by default (MRB_QF_FUSED=1 selects it): every workgroup has to pull the
    # layer's 14-17 MB of weights through ONE CU, and one CU draws ~43 GB/s through LDS-DMA with 48 KB in flight (27 GB/s with fragment-shaped
    # register loads), whatever the number of frames — 4.8 ms per 12-layer forward on 60 CUs against 2.0 ms for the chain on the whole chip;
    # in the step, with the look-ahead's head leg widened to fill the other 196 CUs, 66.1 ms against 65.6 (profiles/r06_qformer_fused.txt).
    qf_fused = os.environ.get("MRB_QF_FUSED", "0") == "1"

    def _qf_fused_ok(self) -> bool:
        c = self.cfg
        return bool(self.qf_fused and c.qf_dim == 768 and c.qf_heads == 12 and c.num_query == 32 and c.qf_inter == 3072)

    @torch.no_grad()
    def _qformer_forward_fused(self, img: torch.Tensor, F_: int, x: torch.Tensor) -> torch.Tensor:
        """x: fp32 [F * nq, D], the (dropped) embedding LayerNorm output.  The cross-attention K / V projections of the image tokens — the
        Q-Former's only big GEMMs — and their V^T copies are issued first, on the side stream when there is one (each cross layer waits for
        its own event); then one fused launch per layer on F_ CUs."""
        c = self.cfg
        D, H, nq, I = c.qf_dim, c.qf_heads, c.num_query, c.qf_inter
        hd = D // H
        Mq = F_ * nq
        Tv = img.shape[0] // F_
        Tvp = ops.rup32(Tv)
        pdrop = c.qf_dropout if self.training else 0.0
        self.qf_t_saved = False
        kv_of = {}

        def kv_jobs():
            for i, L in enumerate(self.qf["layers"]):
                if L["cross"] is None:
                    continue
                C_ = L["cross"]
                kv = self.buf(f"qf{i}_kvc", (F_ * Tv, 2 * D), bf16, zero=False)
                vt_i = self.buf(f"qf{i}_vt_c", (F_, H, ops.rup32(hd), Tvp), bf16)
                ops.gemm(img, C_["kv_w"], kv, bias=C_["kv_b"])
                ops.head_transpose(self.v4(kv, F_, Tv, H, hd, D), out=vt_i)
                ev = None
                if side:
                    ev = torch.cuda.Event()
                    ev.record()
                kv_of[i] = (kv, vt_i, ev)

        side = self.qf_kv_side and self.grad_side_stream_enabled
        if side:
            st, ev0 = self._grad_stream(), torch.cuda.Event()
            ev0.record()
            with torch.cuda.stream(st):
                st.wait_event(ev0)
                kv_jobs()
        else:
            kv_jobs()
        n_layers = len(self.qf["layers"])
        xb = None
        for i, L in enumerate(self.qf["layers"]):
            S_, C_ = L["self"], L["cross"]
            last = i == n_layers - 1
            x_out = self.buf(f"qf{i}_x3", (Mq, D), f32, zero=False)
            xb = self.buf(f"qf{i}_x3b", (Mq, pad64(D)), bf16) if last else None
            o = self.buf(f"qf{i}_o", (Mq, pad64(D)), bf16)
            fields = dict(qkv_w=S_["qkv_w"], so_w=S_["ow"], i_w=L["iw"], o_w=L["ow"], qkv_b=S_["qkv_b"], so_b=S_["ob"], s_lnw=S_["lnw"], s_lnb=S_["lnb"],
                          i_b=L["ib"], o_b=L["ob"], o_lnw=L["lnw"], o_lnb=L["lnb"], x_in=x, x_out=x_out, xb_out=xb, ldxb=pad64(D),
                          qkv=self.buf(f"qf{i}_qkv", (Mq, 3 * D), bf16, zero=False), o=o, ldo=o.stride(0),
                          lse=self.buf(f"qf{i}_lse", (F_, H, ops.rup32(nq)), f32), y=self.buf(f"qf{i}_y", (Mq, D), f32, zero=False),
                          hpre=self.buf(f"qf{i}_hpre", (Mq, pad64(I)), bf16, zero=False), y3=self.buf(f"qf{i}_y3", (Mq, D), f32, zero=False),
                          F=F_, Tv=Tv, Tvp=Tvp, has_cross=int(C_ is not None))
            sites = [S_["sites"][0], S_["sites"][1], 0, 0, L["site"]]
            if C_ is not None:
                kv, vt_i, ev = kv_of[i]
                if ev is not None:
                    torch.cuda.current_stream().wait_event(ev)
                oc = self.buf(f"qf{i}_oc", (Mq, pad64(D)), bf16)
                fields.update(cq_w=C_["q_w"], co_w=C_["ow"], cq_b=C_["q_b"], co_b=C_["ob"], c_lnw=C_["lnw"], c_lnb=C_["lnb"],
                              qc=self.buf(f"qf{i}_qc", (Mq, D), bf16, zero=False), oc=oc,
                              lsec=self.buf(f"qf{i}_lsec", (F_, H, ops.rup32(nq)), f32), y2=self.buf(f"qf{i}_y2", (Mq, D), f32, zero=False), kv=kv, vt=vt_i)
                sites[2], sites[3] = C_["sites"][0], C_["sites"][1]
            ops.qformer_layer_fwd(fields, seed=self.seed if pdrop > 0 else None, p_drop=pdrop, sites=[s_ + self.qf_site_salt for s_ in sites], eps=1e-12)
            x = x_out
        self._qf_last_f32 = x
        return xb

    @torch.no_grad()
    def qformer_backward(self, dx: torch.Tensor, img: torch.Tensor, F_: int) -> torch.Tensor:
        """dx: fp32 [F*nq, D] grad of the last hidden state.  Returns fp32 d(img) [F*Tv, Dv] (grad of ln_vision's output)."""
        c = self.cfg
        D, H, nq, I, Dv = c.qf_dim, c.qf_heads, c.num_query, c.qf_inter, c.vit_dim
        hd = D // H
        Mq = F_ * nq
        Tv = img.shape[0] // F_
        eps, pdrop = 1e-12, c.qf_dropout
        scale = 1.0 / math.sqrt(hd)
        dimg = self.buf("qf_dimg", (F_ * Tv, Dv), f32, zero=False)
        # Round 6 (MRB_QF_KV_BWD_MERGE): the image-token gradient of the cross-attention K / V projections of ALL cross layers as ONE product
        # [dKV_0 | dKV_1 | ...] x [Wkv_0 | Wkv_1 | ...]^T over K = layers x 2 D (6 x 1536 = 9216) at the end of the backward, instead of one
        # [F Tv x Dv x 2 D] GEMM per cross layer that read-modify-writes the 87 MB fp32 accumulator (6 x 172 us in the QVH step): nothing but
        # ln_vision's backward reads d(img), and it runs after the last layer either way.
        cross_ids = [j for j, L_ in enumerate(self.qf["layers"]) if L_["cross"] is not None]
        merge_kv = self.qf_kv_bwd_merge and len(cross_ids) > 1
        if merge_kv:
            pw = self.qf["layers"][cross_ids[0]]["cross"]["kv_wt"].shape[1]       # pad64(2 D)
            if self.qf.get("kv_wt_all") is None:
                self.qf["kv_wt_all"] = torch.cat([self.qf["layers"][j]["cross"]["kv_wt"] for j in cross_ids], dim=1).contiguous()
            dkv_all = self.buf("qf_dkvc_all", (F_ * Tv, len(cross_ids) * pw), bf16)
        else:
            dimg.zero_()
        dy = self.buf("qf_dy", (Mq, D), f32, zero=False)
        dyb = self.buf("qf_dyb", (Mq, pad64(D)), bf16)
        dh = self.buf("qf_dh", (Mq, pad64(I)), bf16, zero=False)
        dhp = self.buf("qf_dhp", (Mq, pad64(I)), bf16, zero=False)
        do = self.buf("qf_do", (Mq, D), bf16, zero=False)
        dqkv = self.buf("qf_dqkv", (Mq, 3 * D), bf16, zero=False)
        dqc = self.buf("qf_dqc", (Mq, D), bf16, zero=False)
        dkv = self.buf("qf_dkvc", (F_ * Tv, 2 * D), bf16, zero=False)
        delta = self.buf("qf_delta", (F_, H, ops.rup32(nq)), f32)
        rq, rt = ops.rup32(nq), ops.rup32(Tv)
        kt_s, qt_s, dot_s = (self.buf(n, (F_, H, ops.rup32(hd), rq), bf16) for n in ("qf_kt_s", "qf_qt_s", "qf_dot_s"))
        kt_c = self.buf("qf_kt_c", (F_, H, ops.rup32(hd), rt), bf16)
        cur = dx
        if getattr(self, "qf_kt_saved", False):
            torch.cuda.current_stream().wait_event(self._qf_kt_event)
        for i in reversed(range(len(self.qf["layers"]))):
            L = self.qf["layers"][i]
            nxt = self.buf(f"qf_dx_{i % 2}", (Mq, D), f32, zero=False)
            # FFN: x3 = LN(y3), y3 = x2 + drop(dense(gelu(dense_i(x2b))))
            self._qf_ln_bwd(cur, self.ws[f"qf{i}_y3"], L["lnw"], eps, dy, dyb, self.qdrop(L["site"], pdrop))
            if self.qf_gelu_bwd_fused:   # round 6: dh = (dy W) * gelu'(hpre) from the GEMM's epilogue (act = 2 reads the saved pre-activation): the same bits, 12 launches fewer
                ops.gemm(dyb, L["owt"], dhp, out2=self.ws[f"qf{i}_hpre"], act=2)
            else:
                ops.gemm(dyb, L["owt"], dh)
                ops.gelu_bwd(dh, self.ws[f"qf{i}_hpre"], dhp)
            ops.gemm(dhp, L["iwt"], nxt, residual=dy)
            cur = nxt
            if L["cross"] is not None:
                C_ = L["cross"]
                nxt = self.buf(f"qf_dxc_{i % 2}", (Mq, D), f32, zero=False)
                self._qf_ln_bwd(cur, self.ws[f"qf{i}_y2"], C_["lnw"], eps, dy, dyb, self.qdrop(C_["sites"][1], pdrop))
                t_saved = getattr(self, "qf_t_saved", False) and self.tout_ok(hd, F_, nq, 8)
                if t_saved:
                    ops.gemm(dyb, C_["owt"], do, tout=(dot_s,), t_rows=nq)
                else:
                    ops.gemm(dyb, C_["owt"], do)
                qc, kv, oc = self.ws[f"qf{i}_qc"], self.ws[f"qf{i}_kvc"], self.ws[f"qf{i}_oc"]
                q4, k4, v4 = self.v4(qc, F_, nq, H, hd), self.v4(kv, F_, Tv, H, hd, 0), self.v4(kv, F_, Tv, H, hd, D)
                do4 = self.v4(do, F_, nq, H, hd)
                kt_x = kt_c
                if getattr(self, "qf_kt_saved", False):
                    kt_x = self.ws[f"qf{i}_kt_c"]
                else:
                    ops.head_transpose(k4, out=kt_c)
                qt_x = qt_s
                if t_saved:
                    qt_x = self.ws[f"qf{i}_qt_c"]
                else:
                    ops.head_transpose(q4, out=qt_s)
                    ops.head_transpose(do4, out=dot_s)
                dkv_i, c0 = (dkv_all, cross_ids.index(i) * pw) if merge_kv else (dkv, 0)
                ops.attention_bwd(q4, k4, v4, self.v4(oc, F_, nq, H, hd), do4, kt_x, qt_x, dot_s, self.ws[f"qf{i}_lsec"], delta,
                                  self.v4(dqc, F_, nq, H, hd), self.v4(dkv_i, F_, Tv, H, hd, c0), self.v4(dkv_i, F_, Tv, H, hd, c0 + D),
                                  scale=scale, drop=self.qdrop(C_["sites"][0], pdrop))
                if not merge_kv:
                    ops.gemm(dkv, C_["kv_wt"], dimg, residual=dimg, tile_cfg=_QF_KV_BWD_CFG)
                if i > 0:
                    ops.gemm(dqc, C_["q_wt"], nxt, residual=dy)
                    cur = nxt
            if i == 0:
                break  # layer 0's self-attention only feeds the frozen query tokens
            S_ = L["self"]
            nxt = self.buf(f"qf_dxs_{i % 2}", (Mq, D), f32, zero=False)
            self._qf_ln_bwd(cur, self.ws[f"qf{i}_y"], S_["lnw"], eps, dy, dyb, self.qdrop(S_["sites"][1], pdrop))
            t_saved = getattr(self, "qf_t_saved", False) and self.tout_ok(hd, F_, nq, 8)
            if t_saved:
                ops.gemm(dyb, S_["owt"], do, tout=(dot_s,), t_rows=nq)
            else:
                ops.gemm(dyb, S_["owt"], do)
            qkv, o = self.ws[f"qf{i}_qkv"], self.ws[f"qf{i}_o"]
            q4, k4, v4 = self.v4(qkv, F_, nq, H, hd, 0), self.v4(qkv, F_, nq, H, hd, D), self.v4(qkv, F_, nq, H, hd, 2 * D)
            do4 = self.v4(do, F_, nq, H, hd)
            kt_x, qt_x = kt_s, qt_s
            if t_saved:
                kt_x, qt_x = self.ws[f"qf{i}_kt_s"], self.ws[f"qf{i}_qt_s"]
            else:
                ops.head_transpose(k4, out=kt_s)
                ops.head_transpose(q4, out=qt_s)
                ops.head_transpose(do4, out=dot_s)
            ops.attention_bwd(q4, k4, v4, self.v4(o, F_, nq, H, hd), do4, kt_x, qt_x, dot_s, self.ws[f"qf{i}_lse"], delta,
                              self.v4(dqkv, F_, nq, H, hd, 0), self.v4(dqkv, F_, nq, H, hd, D), self.v4(dqkv, F_, nq, H, hd, 2 * D),
                              scale=scale, drop=self.qdrop(S_["sites"][0], pdrop))
            ops.gemm(dqkv, S_["qkv_wt"], nxt, residual=dy)
            cur = nxt
        if merge_kv:
            ops.gemm(dkv_all, self.qf["kv_wt_all"], dimg, tile_cfg=_QF_KV_BWD_CFG)
        return dimg

    qf_kv_bwd_merge = os.environ.get("MRB_QF_KV_BWD_MERGE", "1") == "1"
    # round 6: LayerNorm backward + the dropout-backward cast of its result (the next GEMM's operand) in ONE launch: 29 launches per step off
    # the Q-Former backward's dependent chain, the same bits (MRB_QF_LN_BWD_CAST=0: two launches)
    qf_ln_bwd_cast = os.environ.get("MRB_QF_LN_BWD_CAST", "1") == "1"
    qf_gelu_bwd_fused = os.environ.get("MRB_QF_GELU_BWD_FUSED", "1") == "1"
    qf_kt_fwd = os.environ.get("MRB_QF_KT_FWD", "1") == "1"   # cross-attention K^T for the backward written by the forward's side stream (0: by the backward chain)

    def _qf_ln_bwd(self, cur, y, lnw, eps, dy, dyb, drop):
        if self.qf_ln_bwd_cast:
            ops.layernorm_bwd(cur, y, lnw, eps, dy, out_bf16=dyb, out_drop=drop)
        else:
            ops.layernorm_bwd(cur, y, lnw, eps, dy)
            ops.cast_dropout(dy, out_bf16=dyb, drop=drop)

    # ------------------------------------------------------------------------------------------ T5 + LoRA, t5_proj, ln_vision
    def _build_t5(self, src, lora_init):
        c = self.cfg
        d, inner, ff, V = c.d_model, c.t5_heads * c.d_kv, c.d_ff, c.vocab
        r = c.lora_r
        self.lora_scale = c.lora_alpha / c.lora_r
        t = self.t5_prefix
        groups: List[LoraGroup] = []
        adapters: List[Adapter] = []

        def W(name, shape):
            return src.get(t + name + ".weight", shape).float()

        def group(names, in_dim, outs):
            w = torch.cat([W(n, (o, in_dim)) for n, o in zip(names, outs)])
            N = w.shape[0]
            g = LoraGroup(W=self._w(w), Wt=self._w(w.t()), N=N, K=in_dim, site=self.new_site())
            row = 0
            for j, (n, o) in enumerate(zip(names, outs)):
                a = Adapter(name=n, in_dim=in_dim, out=o, row0=row, col0=8 * j, site=self.new_site())
                g.adapters.append(a)
                adapters.append(a)
                row += o
            groups.append(g)
            return g

        self.t5 = dict(enc=[], dec=[])
        self.emb = src.get(t + "shared.weight", (V, d)).to(self.dev).float().contiguous()
        for i in range(c.t5_layers):
            b = f"encoder.block.{i}."
            self.t5["enc"].append(dict(
                ln0=self._v(src.get(t + b + "layer.0.layer_norm.weight", (d,))),
                qkv=group([b + "layer.0.SelfAttention." + x for x in "qkv"], d, [inner] * 3),
                o=group([b + "layer.0.SelfAttention.o"], inner, [d]),
                ln1=self._v(src.get(t + b + "layer.1.layer_norm.weight", (d,))),
                wi=group([b + "layer.1.DenseReluDense.wi_0", b + "layer.1.DenseReluDense.wi_1"], d, [ff, ff]),
                wo=group([b + "layer.1.DenseReluDense.wo"], ff, [d]),
                sites=[self.new_site() for _ in range(4)],
            ))
        for i in range(c.t5_dec_layers):
            b = f"decoder.block.{i}."
            self.t5["dec"].append(dict(
                ln0=self._v(src.get(t + b + "layer.0.layer_norm.weight", (d,))),
                qkv=group([b + "layer.0.SelfAttention." + x for x in "qkv"], d, [inner] * 3),
                o=group([b + "layer.0.SelfAttention.o"], inner, [d]),
                ln1=self._v(src.get(t + b + "layer.1.layer_norm.weight", (d,))),
                cq=group([b + "layer.1.EncDecAttention.q"], d, [inner]),
                ckv=group([b + "layer.1.EncDecAttention.k", b + "layer.1.EncDecAttention.v"], d, [inner] * 2),
                co=group([b + "layer.1.EncDecAttention.o"], inner, [d]),
                ln2=self._v(src.get(t + b + "layer.2.layer_norm.weight", (d,))),
                wi=group([b + "layer.2.DenseReluDense.wi_0", b + "layer.2.DenseReluDense.wi_1"], d, [ff, ff]),
                wo=group([b + "layer.2.DenseReluDense.wo"], ff, [d]),
                sites=[self.new_site() for _ in range(6)],
            ))
        self.t5["enc_final"] = self._v(src.get(t + "encoder.final_layer_norm.weight", (d,)))
        # the encoder's forward weights in one arena, in the order the forward reads them: a GEMM's prefetch workgroups (enc_prefetch)
        # pull a contiguous range — the weights of the next launches — through the memory-side cache
        eorder = [L[k] for L in self.t5["enc"] for k in ("qkv", "o", "wi", "wo")]
        self.enc_w_arena = torch.empty(sum(g.W.numel() for g in eorder), dtype=bf16, device=self.dev)
        off = 0
        for g in eorder:
            v = self.enc_w_arena[off: off + g.W.numel()].view_as(g.W)
            v.copy_(g.W)
            g.W, g.w_off = v, off
            off += v.numel()
        # ... and the transposed copies the backward's dX GEMMs read, in the backward's order
        border = [L[k] for L in reversed(self.t5["enc"]) for k in ("wo", "wi", "o", "qkv")]
        self.enc_wt_arena = torch.empty(sum(g.Wt.numel() for g in border), dtype=bf16, device=self.dev)
        off = 0
        for g in border:
            v = self.enc_wt_arena[off: off + g.Wt.numel()].view_as(g.Wt)
            v.copy_(g.Wt)
            g.Wt, g.wt_off = v, off
            off += v.numel()
        self.t5["dec_final"] = self._v(src.get(t + "decoder.final_layer_norm.weight", (d,)))
        self.t5["lm"] = group(["lm_head"], d, [V])
        self.t5["sites"] = [self.new_site() for _ in range(4)]
        nb = 32
        self.lut_enc = bias_lut(src.get(t + "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", (nb, c.t5_heads)).cpu(), True).to(self.dev)
        self.lut_dec = bias_lut(src.get(t + "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", (nb, c.t5_heads)).cpu(), False).to(self.dev)

        # ---- flat trainable buffer: [LoRA A, Bt ...] [t5_proj.weight] | [t5_proj.bias, ln_vision.weight, ln_vision.bias]
        Dq, Dv = c.qf_dim, c.vit_dim
        n_lora = sum(r * (a.in_dim + a.out) for a in adapters)
        n_decay = n_lora + d * Dq
        n_total = n_decay + d + 2 * Dv
        self.flat = torch.zeros(n_total, dtype=f32, device=self.dev)
        self.grad = torch.zeros_like(self.flat)
        self.adam_m = torch.zeros_like(self.flat)
        self.adam_v = torch.zeros_like(self.flat)
        self.n_decay = n_decay
        self.n_lora = n_lora   # [0, n_lora): every LoRA A / B^T gradient — complete when the T5 encoder backward has been issued
        off = 0
        desc = []
        n_wext_rows = sum(g.N for g in groups)
        self.wext_all = torch.zeros(n_wext_rows, 64, dtype=bf16, device=self.dev)
        n_acat = sum(8 * len(g.adapters) * g.K for g in groups)
        n_bblk = sum(8 * len(g.adapters) * g.N for g in groups)
        self.acat_all = torch.zeros(n_acat, dtype=bf16, device=self.dev)
        self.bblk_all = torch.zeros(n_bblk, dtype=bf16, device=self.dev)
        self.acatt_all = torch.zeros(sum(g.K for g in groups), 64, dtype=bf16, device=self.dev)
        gen = torch.Generator(device="cpu").manual_seed(4321)
        for g in groups:      # the flat trainable buffer in creation order (the layout checkpoints and named_parameters see)
            for j, a in enumerate(g.adapters):
                a.a_off, a.bt_off = off, off + r * a.in_dim
                a.A = self.flat[a.a_off: a.a_off + r * a.in_dim].view(r, a.in_dim)
                a.Bt = self.flat[a.bt_off: a.bt_off + r * a.out].view(r, a.out)
                a.dA = self.grad[a.a_off: a.a_off + r * a.in_dim].view(r, a.in_dim)
                a.dBt = self.grad[a.bt_off: a.bt_off + r * a.out].view(r, a.out)
                off += r * (a.in_dim + a.out)
                ka, kb = t + "base_model.model." + a.name + ".lora_A.default.weight", t + "base_model.model." + a.name + ".lora_B.default.weight"
                if isinstance(src, StateDictSource) and ka in src.sd:
                    a.A.copy_(src.sd[ka])
                    a.Bt.copy_(src.sd[kb].t())
                elif lora_init is not None:
                    lora_init(a, gen)
                else:  # peft default: A kaiming-uniform(a=sqrt(5)), B zeros
                    bound = 1.0 / math.sqrt(a.in_dim)
                    a.A.copy_((torch.rand(r, a.in_dim, generator=gen) * 2 - 1) * bound)
        # the bf16 operand copies (acat / wext / bblk / acatt) in PACKING order: the decoder's cross-attention K / V groups last and next to
        # each other, layer by layer — their operands then form ONE stacked operand each, which the batched projection of all layers' cross
        # K / V (round 4: one thin product + one GEMM instead of 24 + 24) addresses with a per-layer stride
        ckv_groups = [L["ckv"] for L in self.t5["dec"]]
        pack = [g for g in groups if not any(g is x for x in ckv_groups)] + ckv_groups
        wrow = aoff = boff = trow = 0
        for g in pack:
            nad = len(g.adapters)
            g.wext = self.wext_all[wrow: wrow + g.N]
            g.acat = self.acat_all[aoff: aoff + 8 * nad * g.K].view(8 * nad, g.K)
            g.bblk = self.bblk_all[boff: boff + 8 * nad * g.N].view(8 * nad, g.N)
            g.acatt = self.acatt_all[trow: trow + g.K]
            for j, a in enumerate(g.adapters):
                desc.append([a.a_off, a.bt_off, a.in_dim, a.out, aoff + 8 * j * g.K, (wrow + a.row0) * 64 + a.col0,
                             boff + 8 * j * g.N + a.row0, g.N, trow * 64 + 8 * j, 0])
            wrow += g.N
            aoff += 8 * nad * g.K
            boff += 8 * nad * g.N
            trow += g.K
        self._stack_cross_kv(ckv_groups)
        self.adapters, self.groups = adapters, groups
        self.lora_desc = torch.tensor(desc, dtype=torch.int64, device=self.dev)
        # t5_proj / ln_vision (trainable)
        self.proj_w = self.flat[off: off + d * Dq].view(d, Dq)
        self.dproj_w = self.grad[off: off + d * Dq].view(d, Dq)
        off += d * Dq
        assert off == n_decay
        self.proj_b, self.dproj_b = self.flat[off: off + d], self.grad[off: off + d]
        off += d
        self.lnv_w, self.dlnv_w = self.flat[off: off + Dv], self.grad[off: off + Dv]
        off += Dv
        self.lnv_b, self.dlnv_b = self.flat[off: off + Dv], self.grad[off: off + Dv]
        self.proj_w.copy_(src.get("t5_proj.weight", (d, Dq)))
        self.proj_b.copy_(src.get("t5_proj.bias", (d,)))
        self.lnv_w.copy_(src.get("ln_vision.weight", (Dv,)))
        self.lnv_b.copy_(src.get("ln_vision.bias", (Dv,)))
        self.proj_wb = torch.zeros(d, pad64(Dq), dtype=bf16, device=self.dev)      # bf16 operand copies, refreshed per step
        self.proj_wtb = torch.zeros(Dq, pad64(d), dtype=bf16, device=self.dev)
        self.refresh_trainable()

    def transpose2d(self, src: torch.Tensor, C: int, dst: torch.Tensor, drop=None):
        """bf16 src[R, :C] (row stride src.stride(0)) -> dst[C, Rp] = src^T, zero padded to dst.shape[1] (multiple of 32)."""
        R = src.shape[0]
        hd = 64 if C % 64 == 0 else 32
        assert C % hd == 0 and dst.shape[0] == C and dst.shape[1] % 32 == 0 and dst.shape[1] >= R
        v = torch.as_strided(src, (1, R, C // hd, hd), (0, src.stride(0), hd, 1), src.storage_offset())
        ops.head_transpose(v, out=dst.view(1, C // hd, hd, dst.shape[1]), spad=dst.shape[1], drop=drop)

    @torch.no_grad()
    def refresh_trainable(self):
        """Re-derive the bf16 operand copies of the trainable tensors (after init / optimizer step / checkpoint load)."""
        c = self.cfg
        ops.lora_pack(self.flat, self.acat_all, self.wext_all, self.bblk_all, self.acatt_all, self.lora_desc, len(self.adapters), self.lora_scale)
        if getattr(self, "enc_qkv_wc", None) is not None:   # [W | B] of the encoder's qkv groups (enc_qkv_w4): refresh the B columns
            K = self.enc_qkv_wc.shape[2] - 64
            self.enc_qkv_wc[:, :, K:].copy_(self.wext_all.index_select(0, self._enc_qkv_rows).view(self.enc_qkv_wc.shape[0], -1, 64))
        if getattr(self, "enc_wi_wc", None) is not None:    # ... and of its wi groups (enc_wi_w4)
            K = self.enc_wi_wc.shape[2] - 64
            self.enc_wi_wc[:, :, K:].copy_(self.wext_all.index_select(0, self._enc_wi_rows).view(self.enc_wi_wc.shape[0], -1, 64))
        ops.cast_dropout(self.proj_w, out_bf16=self.proj_wb)
        self.transpose2d(self.proj_wb, c.qf_dim, self.proj_wtb)

    def _stack_cross_kv(self, ckv_groups):
        """The frozen weights of all decoder layers' EncDecAttention.k / .v as ONE operand [L * 2 * inner, Kp] (and one transposed operand
        [d, L * 2 * inner] for the backward); the per-layer groups keep working as views.  modeling_t5.py:561-599 computes these projections
        layer by layer inside the decoder; they depend only on the encoder output."""
        self.ckv_all = None
        if not ckv_groups:
            return
        g0 = ckv_groups[0]
        Lc, N, Kp, K = len(ckv_groups), g0.N, g0.W.shape[1], g0.K
        if any(g.N != N or g.K != K or g.W.shape[1] != Kp or len(g.adapters) != 2 for g in ckv_groups):
            return
        sites = [g.site for g in ckv_groups]
        stride = sites[1] - sites[0] if Lc > 1 else 0
        if any(sites[i] != sites[0] + i * stride for i in range(Lc)) or stride < 0:
            return
        W = torch.empty(Lc * N, Kp, dtype=bf16, device=self.dev)
        Wt = torch.zeros(g0.Wt.shape[0], pad64(Lc * N), dtype=bf16, device=self.dev)
        for i, g in enumerate(ckv_groups):
            W[i * N:(i + 1) * N].copy_(g.W)
            Wt[:, i * N:(i + 1) * N].copy_(g.Wt[:, :N])
            g.W, g.Wt = W[i * N:(i + 1) * N], Wt[:, i * N:(i + 1) * N]
        a0, w0, b0 = ckv_groups[0].acat, ckv_groups[0].wext, ckv_groups[0].bblk
        R = a0.shape[0]
        self.ckv_all = dict(W=W, Wt=Wt, L=Lc, N=N, K=K, R=R, site0=sites[0], site_stride=stride,
                            acat=torch.as_strided(a0, (Lc * R, K), (K, 1), a0.storage_offset()),          # [L * 16, K]
                            wext=torch.as_strided(w0, (Lc * N, 64), (64, 1), w0.storage_offset()),        # [L * N, 64]
                            bblk=torch.as_strided(b0, (Lc * R, N), (N, 1), b0.storage_offset()))          # [L * 16, N]
        for i, g in enumerate(ckv_groups):   # the views of the stacked operands ARE the groups' operands (contiguous packing)
            assert g.acat.data_ptr() == self.ckv_all["acat"][i * R].data_ptr() and g.wext.data_ptr() == self.ckv_all["wext"][i * N].data_ptr()

    # ---- LoRA-group forward / backward -------------------------------------------------------------------------
    # Round 4: each T5 layer's weights are read once per pass, so every GEMM finds them in HBM; the [2012 x N] tile GEMMs run 10-25 % slower
    # on cold weights than on a re-used set (tools/prefetch_bench.py).  The qkv GEMM of an encoder layer starts extra workgroups that read
    # the o and wi weights, the wi GEMM the wo weights and the next layer's qkv weights (csrc/gemm.hip pf_blocks).  MRB_ENC_PREFETCH=0: off.
    enc_prefetch = tuple(int(x) for x in (os.environ.get("MRB_ENC_PREFETCH", "32,128,32") + ",,").split(",")[:3] if x)   # workgroups per host launch (qkv, o, wi; 0: none)
    enc_prefetch_ext = os.environ.get("MRB_ENC_PREFETCH_EXT", "0") == "1"   # (measured: no difference)
    enc_pf_plan = int(os.environ.get("MRB_ENC_PF_PLAN", "1"))   # which launch carries which range (see t5_encoder_forward)
    enc_prefetch_min_rows = int(os.environ.get("MRB_ENC_PREFETCH_MIN_ROWS", "1024"))   # a shorter host launch ends before its prefetch does

    def enc_pf(self, groups, M: int, host: int = 0):
        """(tensor, bytes, workgroups) covering the arena range of `groups` (adjacent in the arena), or None"""
        nb = self.enc_prefetch[min(host, len(self.enc_prefetch) - 1)] if self.enc_prefetch else 0
        if not nb or M < self.enc_prefetch_min_rows or not groups:
            return None
        a, b = groups[0].w_off, groups[-1].w_off + groups[-1].W.numel()
        # (second range: the groups' LoRA "up" operands — the K extension's W side, adjacent rows of wext_all)
        e0, e1 = groups[0].wext.storage_offset(), groups[-1].wext.storage_offset() + groups[-1].wext.numel()
        return (self.enc_w_arena[a:b], (b - a) * 2, nb, self.wext_all.view(-1)[e0:e1] if self.enc_prefetch_ext else None)

    # Round 4: the LoRA "down" product of a tall input (the T5 encoder's 2012 rows) rides in the GEMM that consumes it.  MRB_GEMM_THIN=0: a launch
    # of its own (lora_thin_kernel), as before; same bits either way.
    gemm_thin_enabled = os.environ.get("MRB_GEMM_THIN", "1") == "1"
    gemm_thin_min_rows = 512      # (= LORA_THIN_MIN_M: below it lora_rows takes the row kernel, whose summation order differs)
    enc_bwd_prefetch = int(os.environ.get("MRB_ENC_BWD_PREFETCH", "0"))   # the same for the backward's dX GEMMs (transposed weights)

    def enc_pf_bwd(self, groups, M: int):
        if not self.enc_bwd_prefetch or M < self.enc_prefetch_min_rows or not groups:
            return None
        a, b = groups[0].wt_off, groups[-1].wt_off + groups[-1].Wt.numel()
        return (self.enc_wt_arena[a:b], (b - a) * 2, self.enc_bwd_prefetch)

    def lg_fwd(self, g: LoraGroup, x: torch.Tensor, u: torch.Tensor, out: torch.Tensor, u_ready: bool = False, **kw):
        """out = x W^T + u B^T with u = dropout(x) (scale*A)^T:  the rank-8 "down" product is the row kernel of csrc/lora.hip (or was
        already produced by the fused RMSNorm launch: u_ready), the "up" product rides in the main GEMM as a 64-wide K extension."""
        tout, t_rows = kw.pop("tout", None), kw.pop("t_rows", 0)   # head-transposed copies: only the fused decoder kernel writes them (-> True)
        pf = kw.pop("prefetch", None)       # (tensor, bytes, workgroups): rides in the tile GEMM below (a hint: the other paths drop it)
        per_adapter = self.cfg.lora_mask_per_adapter and len(g.adapters) > 1 and self.training and self.cfg.lora_dropout > 0
        if per_adapter:   # peft-faithful: u_j = dropout_j(x) (s A_j)^T with adapter j's own mask (its own call-site id)
            assert not u_ready
            for j, a in enumerate(g.adapters):
                self.lora_thin(x, g.acat[8 * j: 8 * j + 8], u[:, 8 * j:], g.K, drop=self.drop(a.site, self.cfg.lora_dropout))
            ops.gemm(x, g.W, out, aext=u, wext=g.wext, **kw)
            return
        if not u_ready and self._dec_proj_ok(g, x.shape[0], kw, 16 if kw.get("gated") else self.dec_proj_max_rows):
            # <= 16 decoder rows: LoRA "down", main product, "up" product and epilogue in ONE launch (csrc/decproj.hip)
            t_ok = tout is not None and out.dtype == bf16 and not kw.get("gated")
            ops.dec_proj(x, g.W, g.acat, g.wext, u, out, g.K, residual=kw.get("residual"), out2=kw.get("out2"), gated=bool(kw.get("gated")),
                         in_drop=self.drop(g.site, self.cfg.lora_dropout), out_drop=kw.get("drop"), tout=tout if t_ok else None, t_rows=t_rows)
            return t_ok
        ks = self.k_splits_for(x.shape[0], g.N, g.K, out)
        if ks > 1 and not u_ready and kw.get("residual", None) is not None and not kw.get("gated") and kw.get("out2") is None:
            # 12-token decoder rows: a [M x 2048] output has 64 tiles of the skinny kernel; ks blocks per tile share K and add their
            # partial products atomically into `out`, which the LoRA "down" launch pre-initialises with the residual on its way
            res = kw.pop("residual")
            ops.lora_rows(x, g.acat, u, g.K, drop=self.drop(g.site, self.cfg.lora_dropout), init_dst=out, init_src=res)
            ops.gemm(x, g.W, out, aext=u, wext=g.wext, k_splits=ks, **kw)
            return
        thin = None
        if not u_ready:
            if self.gemm_thin_enabled and self.gemm_thin_min_rows <= x.shape[0] <= self.lora_rows_max_m and g.K % 32 == 0 and g.acat.shape[0] <= 32:
                # the GEMM's first workgroups compute u while its tiles run (csrc/gemm.hip thin role): no launch for the "down" product
                thin = (g.acat, g.K, self.drop(g.site, self.cfg.lora_dropout))
            else:
                self.lora_thin(x, g.acat, u, g.K, drop=self.drop(g.site, self.cfg.lora_dropout))
        if thin is not None:
            kw["thin"] = thin
        if pf is not None:
            ops.gemm_prefetch(pf[0], n_blocks=pf[2], nbytes=pf[1], t2=pf[3] if len(pf) > 3 else None)
        if tout is not None and out.dtype == bf16 and not kw.get("gated") and x.shape[0] > 64 and self.gemm_tout_enabled:
            ops.gemm(x, g.W, out, aext=u, wext=g.wext, tout=tout, t_rows=t_rows, **kw)   # tile GEMM: head-transposed copies from its epilogue
            return True
        ops.gemm(x, g.W, out, aext=u, wext=g.wext, **kw)

    # Opt-in (MRB_KSPLIT=1).  Measured on the QVH step: 76.6 vs 77.0 ms — the decoder chain is not what bounds the step once the
    # frozen-ViT look-ahead runs beside it — and the fp32 atomics make the summation order, hence the last bits, run-dependent.
    ksplit_enabled = os.environ.get("MRB_KSPLIT", "0") == "1"
    # Round 3: the adapted projections of the decoder's <= 16 rows as ONE launch each (forward: [RMSNorm +] LoRA down + GEMM + LoRA up +
    # epilogue; backward: g = dy B + the dX GEMM with its masked rank-8 term) instead of two.  MRB_DEC_PROJ=0 restores the two-launch path.
    # Round 4: the tile GEMMs that produce q / k / v (and the backward's dO) also write the head-transposed copies the attention kernels read
    # (csrc/gemm.hip GemmArgs.tout): no head_transpose launches in the T5 encoder and the Q-Former's self / query paths.  MRB_GEMM_TOUT=0
    # restores the transpose launches.
    qf_prefetch = os.environ.get("MRB_QF_PREFETCH", "1") == "1"   # Q-Former forward: every GEMM carries the next one's weight prefetch
    qf_kv_side = os.environ.get("MRB_QF_KV_SIDE", "1") == "1"   # Q-Former cross K / V projections on the side stream beside the query chain
    gemm_tout_enabled = os.environ.get("MRB_GEMM_TOUT", "1") == "1"

    gemm_tout_sites = int(os.environ.get("MRB_TOUT_SITES", "15"))   # bit mask for A/B: 1 T5 encoder fwd (+ stacked cross K/V), 2 encoder bwd, 4 Q-Former fwd, 8 Q-Former bwd

    def tout_ok(self, hd: int, B: int, rows: int, site: int = 1) -> bool:
        """heads of 64, and one clip or clips of a multiple of 32 rows (a wave's 32-row slab then lies inside one clip)"""
        return self.gemm_tout_enabled and bool(self.gemm_tout_sites & site) and hd == 64 and (B == 1 or rows % 32 == 0)

    dec_proj_enabled = os.environ.get("MRB_DEC_PROJ", "1") == "1"
    dec_tout_enabled = os.environ.get("MRB_DEC_TOUT", "1") == "1"   # ... which also write the head-transposed copies the attention kernels read (0: head_transpose launches)

    dec_proj_norm_split = os.environ.get("MRB_DEC_PROJ_NORM_SPLIT", "1") == "1"
    dec_proj_max_rows = int(os.environ.get("MRB_DEC_PROJ_ROWS", "80"))   # ... up to this many rows for the projections without a fused RMSNorm / gating

    def _dec_proj_ok(self, g: "LoraGroup", M: int, kw: dict, max_rows: int = 16) -> bool:
        if not self.dec_proj_enabled or M > max_rows or g.acat is None or g.acat.shape[0] > 32:
            return False
        if self.cfg.lora_mask_per_adapter and len(g.adapters) > 1 and self.training and self.cfg.lora_dropout > 0:
            return False
        if kw.get("bias") is not None or kw.get("act", 0) or kw.get("k_splits", 0):
            return False
        n_out = g.W.shape[0] // 2 if kw.get("gated") else g.W.shape[0]
        # (lm_head, 32128 output columns, stays on the skinny GEMM: 35 vs 43 us — its 1004 blocks re-read the LoRA rows 1004 times)
        return n_out % 16 == 0 and g.K % 32 == 0 and n_out <= 16384

    def k_splits_for(self, M: int, N: int, K: int, out: torch.Tensor) -> int:
        """K split of the skinny GEMM (csrc/gemm.hip): only for <= 32 rows, fp32 output, few output tiles and a long enough K"""
        if not self.ksplit_enabled or M > 32 or out.dtype != f32 or N > 4096 or K < 1024:
            return 1
        tiles = (N + 31) // 32
        ks = max(1, min(8, 256 // tiles, K // 256))
        return ks if ks > 1 else 1

    # rows of the tall operand up to which the thin LoRA products take the row kernel of csrc/lora.hip (decoder: 8-12 rows -> 10 us
    # instead of 12-22 us, and the RMSNorm fusion saves a launch); taller inputs (encoder, M = 2012 / 8048) keep the MFMA skinny
    # kernel: there every CU re-stages the thin vectors (same lines from the same L2 channels) and the row kernel is no faster
    # (tools/lora_rows_bench.py: 15.7 vs 12.6 us at M = 2012, 47 vs 15 us at M = 8048).
    # Round 3: the threshold went from 256 to 2100 rows — in the QVH step (M = 2012) the row kernel + the fused RMSNorm launch are 0.2 ms
    # per step AHEAD (74.0 vs 74.2 ms, 48 launches fewer, the normalised rows are not re-read) although each launch alone is slower than
    # the skinny kernel (15.7 vs 12.6 us); from M = 3992 (ActivityNet) on the skinny kernel stays.
    # Round 3, later: mrblip_lora_rows itself switches to the matrix-core thin kernel from 512 rows on (csrc/lora.hip lora_thin_kernel:
    # 16 rows per block, the 8 waves split K, operands straight from global memory into 16x16x32 fragments; 7 / 14 / 21 us where the row
    # kernel took 8-16 / 20 / 30), and the fused RMSNorm launch becomes norm + thin product there — the QVH step went 72.55 -> 71.36 ms —
    # so the row entry point now serves every M; MRB_LORA_ROWS_MAX_M restores a threshold above which the MFMA skinny GEMM is used.
    lora_rows_max_m = int(os.environ.get("MRB_LORA_ROWS_MAX_M", str(1 << 30)))

    def lora_thin(self, x, a, u, K, drop=None, seg=None, init_dst=None, init_src=None):
        """u[:, :R] = dropout(x)[:, :K] @ a^T for a thin a ([R <= 32, K])"""
        if x.shape[0] <= self.lora_rows_max_m:
            ops.lora_rows(x, a, u, K, drop=drop, seg=seg, init_dst=init_dst, init_src=init_src)
        elif drop is not None:
            ops.lora_down(x, a, u, K, drop=drop)
        else:
            ops.gemm(x, a, u, tile_cfg=3, K=K)

    def norm_lg_fwd(self, x: torch.Tensor, ln: torch.Tensor, g: LoraGroup, xn: torch.Tensor, u: torch.Tensor, out: torch.Tensor, **kw):
        """T5 RMSNorm + the LoRA "down" product of its output in ONE launch, then the main GEMM (q/k/v, wi_0/wi_1, EncDecAttention.q)"""
        tout, t_rows = kw.pop("tout", None), kw.pop("t_rows", 0)
        per_adapter = self.cfg.lora_mask_per_adapter and len(g.adapters) > 1 and self.training and self.cfg.lora_dropout > 0
        if g.K <= 2048 and self._dec_proj_ok(g, x.shape[0], kw):   # <= 16 decoder rows: norm, LoRA and projection in one launch
            t_ok = tout is not None and out.dtype == bf16 and not kw.get("gated")
            ops.dec_proj(xn, g.W, g.acat, g.wext, u, out, g.K, x32=x, gamma=ln, eps=self.cfg.t5_eps, residual=kw.get("residual"),
                         out2=kw.get("out2"), gated=bool(kw.get("gated")), in_drop=self.drop(g.site, self.cfg.lora_dropout), out_drop=kw.get("drop"),
                         tout=tout if t_ok else None, t_rows=t_rows)
            return t_ok
        if (16 < x.shape[0] <= self.dec_proj_max_rows and not kw.get("gated") and self.dec_proj_norm_split
                and self._dec_proj_ok(g, x.shape[0], kw, self.dec_proj_max_rows)):
            # 17..80 rows (a short encoder): the fused kernel cannot hold that many normalised rows in LDS — plain RMSNorm, then the
            # one-launch projection on its output (instead of fused norm + LoRA-down and a tile GEMM with one or two 64-row tiles)
            ops.rmsnorm_fwd(x, ln, self.cfg.t5_eps, out_bf16=xn)
            kw["tout"], kw["t_rows"] = tout, t_rows
            return self.lg_fwd(g, xn, u, out, **kw)
        kw["tout"], kw["t_rows"] = tout, t_rows
        thin_in_gemm = self.gemm_thin_enabled and self.gemm_thin_min_rows <= x.shape[0] <= self.lora_rows_max_m and g.K % 32 == 0 and not per_adapter
        if self.fuse_norm_lora and x.shape[0] <= self.lora_rows_max_m and not per_adapter and not thin_in_gemm:
            ops.rmsnorm_lora_fwd(x, ln, self.cfg.t5_eps, xn, g.acat, u, drop=self.drop(g.site, self.cfg.lora_dropout))
            return self.lg_fwd(g, xn, u, out, u_ready=True, **kw)
        ops.rmsnorm_fwd(x, ln, self.cfg.t5_eps, out_bf16=xn)
        return self.lg_fwd(g, xn, u, out, **kw)

    fuse_norm_lora = os.environ.get("MRB_FUSE_NORM_LORA", "1") == "1"

    # Round 5: the weight-gradient launches of several LoRA groups go out as ONE launch (ops.lora_grads_batched: the same blocks, the same
    # bits).  Jobs queued for the side stream are merged per hand-over (side_flush); the encoder backward collects a whole layer's four
    # groups itself (t5_encoder_backward).  MRB_LORA_GRADS_BATCH=0: one launch per group, as in round 4.
    lora_grads_batch = os.environ.get("MRB_LORA_GRADS_BATCH", "1") == "1"

    def lg_bwd(self, g: LoraGroup, dy: torch.Tensor, x: torch.Tensor, u: torch.Tensor, gbuf: torch.Tensor, dx: Optional[torch.Tensor],
               residual: Optional[torch.Tensor] = None, side: bool = False, tile_cfg: int = 0, flush: bool = True, tout=None, t_rows: int = 0,
               prefetch=None, collect: Optional[list] = None, parts: Optional[torch.Tensor] = None, parts_cfg: Tuple[int, int] = (1, 13),
               g_ready: bool = False):
        """g_ready (round 6): gbuf already holds g = dy (scale B) — the kernel that wrote dy computed it (ops.rmsnorm_bwd(g_prod=)).
        parts (round 5, [k_splits + 1, M, K_in] fp32 or bf16; dx must be None): the input gradient as PARTIAL products of the 4-wave
        kernel's K-split form (ops.gemm_ksplit, parts_cfg = (k_splits, tile config)); the LoRA term is the last part, unmasked — the
        consumer (ops.rmsnorm_bwd / ops.gated_gelu_bwd) adds the parts and applies this group's lora_dropout mask to it.

        dy bf16 [M,N]; x the saved bf16 input; u the saved [M,64] LoRA activations.  Accumulates dA, dB of every adapter of the
        group (one launch) and (optionally) dx = dy W (+ residual) + mask * (g A) (one GEMM: the rank-8 term is its K-extension).
        side=True: the weight-gradient launch goes to the gradient side stream and runs beside the dX GEMM (the caller guarantees
        that dy / gbuf are not overwritten before its next side_join()).  flush=False only QUEUES that launch: it goes out with the
        next flushing call (side_flush) — every hand-over to the side stream is an event record on the main stream, and a record
        between two kernels costs ~7 us of dispatch bubble (round 3, tools/prof_layer.py: 5 records = 48 us per encoder layer)."""
        drop = self.drop(g.site, self.cfg.lora_dropout)
        seg = [v for a in g.adapters for v in (a.row0, a.row0 + a.out)] if len(g.adapters) > 1 else None
        if self.cfg.lora_mask_per_adapter and len(g.adapters) > 1 and drop is not None:
            # peft-faithful masks: the weight gradients and the rank-8 part of dX per adapter, each with ITS mask; the frozen-weight
            # part of dX is one plain GEMM
            self.lora_thin(dy, g.bblk, gbuf, g.N, seg=seg)

            def grads_per_adapter():
                for j, a in enumerate(g.adapters):
                    ops.lora_grads(dy, u[:, 8 * j:], x, gbuf[:, 8 * j:], [a.dBt], [a.row0], [a.out], [a.dA], g.K, drop=self.drop(a.site, self.cfg.lora_dropout))
            if side and self.grad_side_stream_enabled:
                self.side_defer(grads_per_adapter)
                if flush:
                    self.side_flush()
            else:
                grads_per_adapter()
            if dx is not None:
                ops.gemm(dy, g.Wt, dx, residual=residual, K=pad64(g.N))
                for j, a in enumerate(g.adapters):
                    ops.lora_dx_add(dx, gbuf[:, 8 * j: 8 * j + 8], g.acat[8 * j: 8 * j + 8], drop=self.drop(a.site, self.cfg.lora_dropout))
            return
        assert parts is None or dx is None
        fused = dx is not None and g.N % 32 == 0 and self._dec_proj_ok(g, dy.shape[0], {}, self.dec_proj_max_rows) and g.Wt.shape[0] % 16 == 0
        ks = self.k_splits_for(dy.shape[0], g.K, pad64(g.N), dx) if (dx is not None and not fused) else 1
        if fused:    # <= 16 decoder rows: g = dy B and dX = dy W + mask (.) (g A) [+ residual] in one launch
            t_ok = tout is not None and dx.dtype == bf16
            ops.dec_proj(dy, g.Wt, g.bblk, g.acatt, gbuf, dx, g.N, residual=residual, ext_drop=drop, tout=tout if t_ok else None, t_rows=t_rows)
        elif ks > 1:   # dX by the K-split skinny GEMM: this launch also pre-initialises dx (residual or zero)
            self.lora_thin(dy, g.bblk, gbuf, g.N, seg=seg, init_dst=dx, init_src=residual)
        elif not g_ready:
            self.lora_thin(dy, g.bblk, gbuf, g.N, seg=seg)                  # g' = scale * dy @ B      [M, 8*nad]
        ads = g.adapters
        if self.lora_grads_batch and (collect is not None or (side and self.grad_side_stream_enabled)):
            job = ops.lora_grads_job(dy, u, x, gbuf, [a.dBt for a in ads], [a.row0 for a in ads], [a.out for a in ads], [a.dA for a in ads], g.K, drop=drop)
            if collect is not None:
                collect.append(job)          # the caller launches the layer's jobs together
            else:
                self.side_defer(("grads", job))
                if flush:
                    self.side_flush()
        else:
            def grads():
                ops.lora_grads(dy, u, x, gbuf, [a.dBt for a in ads], [a.row0 for a in ads], [a.out for a in ads], [a.dA for a in ads], g.K, drop=drop)
            if side and self.grad_side_stream_enabled:
                self.side_defer(grads)
                if flush:
                    self.side_flush()
            else:
                grads()
        if parts is not None:
            ops.gemm_ksplit(dy, g.Wt, parts, pad64(g.N), parts_cfg[0], ext=(gbuf, g.acatt), tile_cfg=parts_cfg[1])
            return False
        if dx is not None and not fused:
            if ks > 1:
                ops.lora_dx(dy, g.Wt, gbuf, g.acatt, dx, pad64(g.N), residual=None, drop=drop, k_splits=ks)
            else:
                t_tile = tout is not None and dx.dtype == bf16 and residual is None and dy.shape[0] > 64 and self.gemm_tout_enabled
                if prefetch is not None:
                    ops.gemm_prefetch(prefetch[0], n_blocks=prefetch[2], nbytes=prefetch[1])
                ops.lora_dx(dy, g.Wt, gbuf, g.acatt, dx, pad64(g.N), residual=residual, drop=drop, tile_cfg=tile_cfg,
                            tout=tout if t_tile else None, t_rows=t_rows)
                return bool(t_tile)
        return bool(fused and tout is not None and dx.dtype == bf16)   # True: the head-transposed copies of dx were written

    vit_rowv = os.environ.get("MRB_VIT_ROWV", "1") == "1"   # (0: the transposed-copy path, for A/B)
    fuse_bwd_cast = os.environ.get("MRB_FUSE_BWD_CAST", "1") == "1"
    grad_side_stream_enabled = os.environ.get("MRB_GRAD_SIDE", "1") == "1"
    _gstream = None

    def _grad_stream(self):
        if self._gstream is None:
            self._gstream = torch.cuda.Stream(device=self.dev)
        return self._gstream

    _side_q: list = None

    side_batch = os.environ.get("MRB_SIDE_BATCH", "1") == "1"   # 0: every queued job is handed over at once (one record each; for A/B)

    def side_defer(self, fn: Callable[[], None]):
        """queue launches for the gradient side stream (fn enqueues them on the then-current stream)"""
        if self._side_q is None:
            self._side_q = []
        self._side_q.append(fn)
        if not self.side_batch:
            self.side_flush()

    def side_flush(self):
        """ONE event record on the main stream, then every queued job goes to the side stream behind it"""
        if not self._side_q:
            return
        jobs, self._side_q = self._side_q, []
        st, ev = self._grad_stream(), torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(st):
            st.wait_event(ev)
            grads = []     # ("grads", job) entries: independent launches (disjoint outputs, read-only inputs) — merged, up to 8 per launch,
            for fn in jobs:  # and issued behind the hand-over's other jobs
                if isinstance(fn, tuple):
                    grads.append(fn[1])
                else:
                    fn()
            for k in range(0, len(grads), 8):
                ops.lora_grads_batched(grads[k: k + 8])

    def side_join(self):
        """the main stream waits for everything issued (or still queued) for the gradient side stream so far"""
        self.side_flush()
        if self._gstream is not None:
            ev = torch.cuda.Event()
            with torch.cuda.stream(self._gstream):
                ev.record()
            torch.cuda.current_stream().wait_event(ev)

    # ---- encoder ---------------------------------------------------------------------------------------------
    @torch.no_grad()
    def t5_encoder_forward(self, x0: torch.Tensor, B: int, S: int, kmask: torch.Tensor, want_grad: bool = True) -> torch.Tensor:
        """x0 fp32 [B*S, d] (inputs_embeds).  Returns bf16 encoder output [B*S, d].  want_grad=False (eval / generate): the per-layer
        Q^T / K^T copies that only the backward reads (~400 MB at S = 2012, XL) are neither allocated nor written."""
        c = self.cfg
        d, H, dk, ff, p = c.d_model, c.t5_heads, c.d_kv, c.d_ff, c.t5_dropout
        inner = H * dk
        M = B * S
        x = self.buf("e_x0", (M, d), f32, zero=False)
        ops.cast_dropout(x0, out_f32=x, drop=self.drop(self.t5["sites"][0], p))
        vt = self.buf("e_vt", (B, H, ops.rup32(dk), ops.rup32(S)), bf16)
        self.enc_t_saved.clear()     # (sticky flags a later backward trusts: reset by every forward)
        w4q = self._enc_qkv_w4_ok(M)
        w4wi = self._enc_wi_w4_ok(M)
        for i, L in enumerate(self.t5["enc"]):
            qkv = self.buf(f"e{i}_qkv", (M, 3 * inner), bf16, zero=False)
            vt_i = vt
            if w4q:
                # Round 5 (MRB_ENC_QKV_W4): the projection through the hand-pipelined 4-wave kernel, which has no K extension —
                # [xn | u] x [W | B]^T is ONE plain product over K + 64 (csrc/gemm.hip gemm_w4_kernel; tools/qkv_tile_probe.py: 50-54 us
                # against 80 us for the 16-wave tile).  u by its own thin launch, the transposed copies by a transpose launch.
                g = L["qkv"]
                xnu = self.buf(f"e{i}_xnu", (M, g.K + 64), bf16)
                xn, u = xnu[:, :g.K], xnu[:, g.K:]
                self.ws[f"e{i}_xn"], self.ws[f"e{i}_u_qkv"] = xn, u
                if self.enc_qkv_fuse_norm:
                    ops.rmsnorm_lora_fwd(x, L["ln0"], c.t5_eps, xn, g.acat, u, drop=self.drop(g.site, c.lora_dropout))
                else:
                    ops.rmsnorm_fwd(x, L["ln0"], c.t5_eps, out_bf16=xn)
                    self.lora_thin(xn, g.acat, u, g.K, drop=self.drop(g.site, c.lora_dropout))
                ops.gemm(xnu, self.enc_qkv_wc[i], qkv, tile_cfg=self.enc_qkv_w4, K=g.K + 64)
                t_done = False
                if B == 1 and want_grad and dk == 64 and self.enc_qkv_t3:
                    # Q^T, K^T (for the backward) and V^T in ONE transpose launch over the 3 H "heads" of the fused output: the backward
                    # then needs no side-stream transposes, no hand-over record and no wait in front of its attention kernels
                    qkvt = self.buf(f"e{i}_qkvt", (1, 3 * H, 64, ops.rup32(S)), bf16)
                    ops.head_transpose(self.v4(qkv, B, S, 3 * H, dk, 0), out=qkvt)
                    self.ws[f"e{i}_qt"], self.ws[f"e{i}_kt"], vt_i = qkvt[:, :H], qkvt[:, H:2 * H], qkvt[:, 2 * H:]
                    t_done = True
            else:
                xn = self.buf(f"e{i}_xn", (M, pad64(d)), bf16)
                u = self.buf(f"e{i}_u_qkv", (M, 64), bf16)
                # (round 4: the projection's epilogue writes V^T for this layer's attention and Q^T / K^T for its backward)
                t_ok = self.tout_ok(dk, B, S)
                qt_i = self.buf(f"e{i}_qt", (B, H, 64, ops.rup32(S)), bf16) if (t_ok and want_grad) else None
                kt_i = self.buf(f"e{i}_kt", (B, H, 64, ops.rup32(S)), bf16) if (t_ok and want_grad) else None
                t_done = self.norm_lg_fwd(x, L["ln0"], L["qkv"], xn, u, qkv, tile_cfg=_ENC_FWD_CFG[0], tout=(qt_i, kt_i, vt) if t_ok else None, t_rows=S,
                                          prefetch=self.enc_pf([L["o"], L["wi"]] if self.enc_pf_plan == 0 else [L["o"]], M))
            self.enc_t_saved[i] = bool(t_done) and want_grad
            q4, k4, v4 = self.v4(qkv, B, S, H, dk, 0), self.v4(qkv, B, S, H, dk, inner), self.v4(qkv, B, S, H, dk, 2 * inner)
            if not t_done:
                ops.head_transpose(v4, out=vt)
            o = self.buf(f"e{i}_o", (M, pad64(inner)), bf16)
            lse = self.buf(f"e{i}_lse", (B, H, ops.rup32(S)), f32)
            adrop = self.drop(L["sites"][0], p)
            dbits = self.buf(f"e{i}_dbits", ops.drop_bits_shape(B, H, S, S), torch.int32, zero=False) if adrop is not None else None
            ops.attention_fwd(q4, k4, vt_i, self.v4(o, B, S, H, dk), lse, scale=1.0, bias_lut=self.lut_enc, kmask=kmask, drop=adrop, drop_bits=dbits)
            uo = self.buf(f"e{i}_u_o", (M, 64), bf16)
            xm = self.buf(f"e{i}_xm", (M, d), f32, zero=False)
            self.lg_fwd(L["o"], o, uo, xm, residual=x, drop=self.drop(L["sites"][1], p), tile_cfg=_ENC_FWD_CFG[1],
                        prefetch=self.enc_pf([L["wi"]], M, 1) if self.enc_pf_plan else None)
            y = self.buf(f"e{i}_y", (M, pad64(ff)), bf16)
            h = self.buf(f"e{i}_h", (M, 2 * ff), bf16, zero=False)
            nxt = [self.t5["enc"][i + 1]["qkv"]] if i + 1 < len(self.t5["enc"]) else []
            if w4wi:
                # Round 6 (MRB_ENC_WI_W4): the gated-GELU projection on the 4-wave kernel's GATED form — [xn2 | u] x [W | B]^T over K + 64, the
                # gate / linear halves of a tile from the two halves of the stacked weight, y = dropout(gelu(h0) * h1) and the
                # pre-activations from its epilogue (csrc/gemm.hip gemm_w4_kernel<GATED>): same bits as the generic tile's gated epilogue
                g = L["wi"]
                xnu2 = self.buf(f"e{i}_xnu2", (M, g.K + 64), bf16)
                xn2, uw = xnu2[:, :g.K], xnu2[:, g.K:]
                self.ws[f"e{i}_xn2"], self.ws[f"e{i}_u_wi"] = xn2, uw
                ops.rmsnorm_fwd(xm, L["ln1"], c.t5_eps, out_bf16=xn2)
                self.lora_thin(xn2, g.acat, uw, g.K, drop=self.drop(g.site, c.lora_dropout))
                ops.gemm(xnu2, self.enc_wi_wc[i], y, out2=h, gated=True, drop=self.drop(L["sites"][2], p), tile_cfg=13, K=g.K + 64)
            else:
                xn2 = self.buf(f"e{i}_xn2", (M, pad64(d)), bf16)
                uw = self.buf(f"e{i}_u_wi", (M, 64), bf16)
                self.norm_lg_fwd(xm, L["ln1"], L["wi"], xn2, uw, y, out2=h, gated=True, drop=self.drop(L["sites"][2], p), tile_cfg=_ENC_FWD_CFG[2],
                                 prefetch=self.enc_pf([L["wo"]] + (nxt if self.enc_pf_plan < 2 else []), M, 2))
            uwo = self.buf(f"e{i}_u_wo", (M, 64), bf16)
            xo = self.buf(f"e{i + 1}_x" if i + 1 < len(self.t5["enc"]) else "e_xlast", (M, d), f32, zero=False)
            self.lg_fwd(L["wo"], y, uwo, xo, residual=xm, drop=self.drop(L["sites"][3], p), tile_cfg=_ENC_FWD_CFG[3],
                        prefetch=self.enc_pf(nxt, M, 2) if self.enc_pf_plan == 2 else None)
            self.ws[f"e{i}_xin"] = x
            x = xo
        nf = self.buf("e_nf", (M, d), f32, zero=False)
        ops.rmsnorm_fwd(x, self.t5["enc_final"], c.t5_eps, out_f32=nf)
        enc = self.buf("e_out", (M, pad64(d)), bf16)
        ops.cast_dropout(nf, out_bf16=enc, drop=self.drop(self.t5["sites"][1], p))
        self.ws["e_xfinal_in"] = x
        return enc

    # Round 5: the T5 encoder's qkv projection ([2012 x 6144 x 2048] at QVH) through the hand-pipelined 4-wave kernel of the ViT: 14 = its
    # 256x192 form (256 tiles = one full round of the chip), 13 = 256x256, 0 = the 16-wave generic tile with K extension, thin role and
    # head-transposed copies (round 4).  Stand-alone on cold weights 49.8 / 54.3 / 79.7 us (tools/qkv_tile_probe.py); in the step
    # norm + thin + GEMM + V^T transpose = 70 us against 96 (profiles/r05_layer_timeline_w4qkv.txt), 67.90 vs 68.18 ms per step.
    enc_qkv_w4 = int(os.environ.get("MRB_ENC_QKV_W4", "14"))
    enc_qkv_wc = None
    enc_qkv_fuse_norm = os.environ.get("MRB_ENC_QKV_FUSE_NORM", "0") == "1"   # RMSNorm + LoRA down product in one launch (rmsnorm_lora_fwd) instead of norm + thin
    # 1: one clip's Q^T / K^T / V^T from ONE transpose launch of the forward instead of V^T there and Q^T / K^T on the backward's side stream
    # (no hand-over record, no wait in front of the attention backward).  Measured same box: 65.70 / 65.69 vs 65.49 / 65.65 ms — the forward
    # runs with the chip to itself and pays its +8 us per layer 1:1, the backward's bubbles are absorbed by the look-ahead: off.
    enc_qkv_t3 = os.environ.get("MRB_ENC_QKV_T3", "0") == "1"

    # Round 5: the encoder backward's input-gradient GEMMs on the 4-wave kernel (K-split where the output has too few tiles): wo 83.5 -> 44 us,
    # wi 146.5 -> 79 us, qkv 88 -> 53 us per layer stand-alone (tools/bwd_w4_probe.py).  MRB_ENC_BWD_W4=0: the generic tile with its
    # masked K extension, roles and all (round 4).
    enc_bwd_w4 = os.environ.get("MRB_ENC_BWD_W4", "1") == "1"
    enc_fuse_g = os.environ.get("MRB_ENC_FUSE_G", "1") == "1"   # round 6: g = dy (scale B) of the wo / o groups from the RMSNorm backward launches (0: lora_thin launches)
    # 1: ONE side-stream hand-over per encoder layer of the backward, at the point where the K^T / Q^T job must leave anyway (behind the wi
    # product): the weight-gradient launch then holds wo, wi of the layer and o, qkv of the layer above and runs beside the o product and
    # the attention backward instead of beside the next layer's thin / wo launches.  0: a second hand-over at the end of the layer.
    enc_grads_at_wi = os.environ.get("MRB_ENC_GRADS_AT_WI", "0") == "1"

    # most K-split parts of the wi / qkv input gradients (A/B knob: fewer parts = fewer units than CUs but a cheaper consumer)
    enc_bwd_max_ks = int(os.environ.get("MRB_ENC_BWD_MAX_KS", "8"))

    def _enc_bwd_w4_ok(self, M: int) -> bool:
        c = self.cfg
        return bool(self.enc_bwd_w4 and M >= 1024 and not (c.lora_mask_per_adapter and self.training and c.lora_dropout > 0))

    @staticmethod
    def ksplit_cfg(M: int, N: int, K: int, n_cu: int = 256, max_ks: int = 8) -> Tuple[int, int]:
        """(k_splits, tile config) of ops.gemm_ksplit for an [M x N x K] product: the pair with the shortest estimated time — rounds of
        n_cu units x tile width x K-tiles per unit (the 256x192 tile of config 14 does 3/4 of the work of config 13's 256x256 per K-tile)"""
        best = None
        for cfg, bn in ((13, 256), (14, 192)):
            tiles = -(-M // 256) * -(-N // bn)
            for ks in (1, 2, 3, 4, 6, 8):
                if (K // 64) % ks or ks > max_ks:
                    continue
                units = tiles * ks
                cost = -(-units // n_cu) * bn * (K // 64 // ks + 6) + 16 * ks      # (+ 6 K-tiles: a unit's prologue and epilogue; + the consumer's extra part)
                if best is None or cost < best[0]:
                    best = (cost, ks, cfg)
        return best[1], best[2]

    # Round 6: the encoder's gated wi projection ([2012 x 2 x 5120 x 2048] at QVH) on the 4-wave kernel's gated form (1: on above 1024 rows).
    # OFF by default: same box, alternating runs (profiles/r06_ab_switches.txt) 65.06 / 65.11 ms with it, 64.17 ms without — in the step the
    # launch takes 113 us + a 9 us thin launch where the generic gated tile with its in-GEMM thin role and the prefetch of wo's weights took
    # 102 us, and wo behind it 80 instead of 67 us (profiles/r06_base_layer_timeline.txt): the 4-wave kernel has no role workgroups.
    enc_wi_w4 = int(os.environ.get("MRB_ENC_WI_W4", "0"))
    enc_wi_wc = None

    def _enc_wc_build(self, name: str):
        """[layers, N, K + 64] = [W | B] of the encoder's ``name`` groups (+ the rows of wext_all their B columns are refreshed from)"""
        gs = [L[name] for L in self.t5["enc"]]
        g0 = gs[0]
        if g0.K % 64 or any(g.K != g0.K or g.W.shape[0] != g0.W.shape[0] for g in gs):
            return None, None
        N = g0.W.shape[0]
        wc = torch.zeros(len(gs), N, g0.K + 64, dtype=bf16, device=self.dev)
        rows = []
        base = self.wext_all.data_ptr()
        for i, g in enumerate(gs):
            wc[i, :, :g.K].copy_(g.W[:, :g.K])
            r0 = (g.wext.data_ptr() - base) // (64 * 2)
            rows.append(torch.arange(r0, r0 + N, dtype=torch.int64))
        rows = torch.cat(rows).to(self.dev)
        wc[:, :, g0.K:].copy_(self.wext_all.index_select(0, rows).view(len(gs), N, 64))
        return wc, rows

    def _enc_wi_w4_ok(self, M: int) -> bool:
        c = self.cfg
        if not self.enc_wi_w4 or M < 1024 or (c.lora_mask_per_adapter and self.training and c.lora_dropout > 0) or c.d_ff % 8:
            return False
        if self.enc_wi_wc is None:
            self.enc_wi_wc, self._enc_wi_rows = self._enc_wc_build("wi")
            if self.enc_wi_wc is None:
                self.enc_wi_w4 = 0
                return False
        return True

    def _enc_qkv_w4_ok(self, M: int) -> bool:
        if not self.enc_qkv_w4 or M < 1024 or (self.cfg.lora_mask_per_adapter and self.training and self.cfg.lora_dropout > 0):
            return False
        if self.enc_qkv_wc is None:       # [layers, N, K + 64] = [W | B] per layer; B columns refreshed by refresh_trainable
            gs = [L["qkv"] for L in self.t5["enc"]]
            g0 = gs[0]
            if g0.K % 64 or any(g.K != g0.K or g.W.shape[0] != g0.W.shape[0] for g in gs):
                self.enc_qkv_w4 = 0
                return False
            N = g0.W.shape[0]
            wc = torch.zeros(len(gs), N, g0.K + 64, dtype=bf16, device=self.dev)
            rows = []
            base = self.wext_all.data_ptr()
            for i, g in enumerate(gs):
                wc[i, :, :g.K].copy_(g.W[:, :g.K])
                r0 = (g.wext.data_ptr() - base) // (64 * 2)
                rows.append(torch.arange(r0, r0 + N, dtype=torch.int64))
            self._enc_qkv_rows = torch.cat(rows).to(self.dev)
            self.enc_qkv_wc = wc
            self.enc_qkv_wc[:, :, g0.K:].copy_(self.wext_all.index_select(0, self._enc_qkv_rows).view(len(gs), N, 64))
        return True

    @torch.no_grad()
    def t5_encoder_backward(self, denc: torch.Tensor, B: int, S: int, kmask: torch.Tensor) -> torch.Tensor:
        """denc fp32 [B*S, d]: grad of the encoder output.  Returns fp32 grad of inputs_embeds."""
        c = self.cfg
        d, H, dk, ff, p = c.d_model, c.t5_heads, c.d_kv, c.d_ff, c.t5_dropout
        inner = H * dk
        M = B * S
        t = self.buf("eb_t", (M, d), f32, zero=False)
        ops.cast_dropout(denc, out_f32=t, drop=self.drop(self.t5["sites"][1], p))
        dx = self.buf("eb_dx_a", (M, d), f32, zero=False)
        ops.rmsnorm_bwd(t, self.ws["e_xfinal_in"], self.t5["enc_final"], c.t5_eps, dx)
        # (dyb alternates between two buffers: the fused write of layer i - 1's operand happens at the END of layer i, when layer i's
        # weight-gradient launch on the side stream may still be reading its own; the other buffer's readers were joined at the top of i)
        # Round 5: ONE weight-gradient launch per layer (the four groups' jobs together, on the side stream at the end of the layer) and its
        # completion is awaited TWO layers later: the buffers it reads exist twice (layer parity; dyb, which the layer ABOVE writes for the
        # layer below, three times), so the main stream never waits for a side-stream launch that was issued a moment ago (round 4: four
        # launches, two hand-overs and one join per layer — the join at the top of a layer waited for the qkv group's launch).
        batch = self.lora_grads_batch and self.grad_side_stream_enabled and not c.lora_mask_per_adapter
        at_wi = batch and self.enc_grads_at_wi
        carry: list = []
        dyb_pair = (self.buf("eb_dyb", (M, pad64(d)), bf16), self.buf("eb_dyb_alt", (M, pad64(d)), bf16)) + ((self.buf("eb_dyb_alt2", (M, pad64(d)), bf16),) if batch else ())
        nb = 2 if batch else 1
        dyb2_s = [self.buf("eb_dyb2" + "_alt" * k, (M, pad64(d)), bf16) for k in range(nb)]
        g_s = [tuple(self.buf(n + "_alt" * k, (M, 64), bf16) for n in ("eb_g", "eb_g2", "eb_g3", "eb_g4")) for k in range(nb)]
        # Round 6: the rank-8 products g = dy (scale B) of the wo and o groups come out of the RMSNorm backward launches that write their dy
        # operands (ops.rmsnorm_bwd(g_prod=)): two lora_thin launches per layer (19-48 + 10 us on the main stream) disappear.  The wo group's g
        # is written by the layer ABOVE, like its dy: three buffers by layer index, as for dyb.
        L0_ = self.t5["enc"][0]
        fuse_g = (self.enc_fuse_g and self.fuse_bwd_cast and not (c.lora_mask_per_adapter and self.training and c.lora_dropout > 0)
                  and all(len(L0_[n].adapters) == 1 and L0_[n].N == d and L0_[n].bblk.shape[0] == 8 for n in ("wo", "o")) and d % 4 == 0 and d <= 2048
                  and M > max(self.dec_proj_max_rows, 32))     # (fewer rows: the one-launch projection computes g itself)
        gbw = [self.buf("eb_gw" + "_alt" * k, (M, 64), bf16) for k in range(3)] if fuse_g else None
        dyact = self.buf("eb_dyact", (M, ff), bf16, zero=False)
        # Round 5: the three big input-gradient GEMMs of a layer (wo: [M x ff x d], wi: [M x d x 2 ff], qkv: [M x d x 3 inner]) on the
        # hand-pipelined 4-wave kernel, the [M x d] ones as a K-split that fills the chip; their outputs are parts the consumers add
        w4b = self._enc_bwd_w4_ok(M)
        if w4b:
            L0 = self.t5["enc"][0]
            cfg_wo = self.ksplit_cfg(M, L0["wo"].K, pad64(L0["wo"].N), max_ks=1)       # (the gated-GELU backward adds exactly two parts)
            cfg_wi, cfg_qkv = (self.ksplit_cfg(M, g.K, pad64(g.N), max_ks=self.enc_bwd_max_ks) for g in (L0["wi"], L0["qkv"]))
            dyact_p = self.buf("eb_dyact_p", (cfg_wo[0] + 1, M, ff), bf16, zero=False)
            dxn_p_wi = self.buf("eb_dxn_p_wi", (cfg_wi[0] + 1, M, d), f32, zero=False)
            dxn_p_qkv = self.buf("eb_dxn_p_qkv", (cfg_qkv[0] + 1, M, d), f32, zero=False)
        dh_s = [self.buf("eb_dh" + "_alt" * k, (M, 2 * ff), bf16, zero=False) for k in range(nb)]
        dxn = self.buf("eb_dxn", (M, d), f32, zero=False)
        do = self.buf("eb_do", (M, inner), bf16, zero=False)
        dqkv_s = [self.buf("eb_dqkv" + "_alt" * k, (M, 3 * inner), bf16, zero=False) for k in range(nb)]
        grads_done: Dict[int, torch.cuda.Event] = {}
        rs = ops.rup32(S)
        kt, qt, dot = (self.buf(n, (B, H, ops.rup32(dk), rs), bf16) for n in ("eb_kt", "eb_qt", "eb_dot"))
        delta = self.buf("eb_delta", (B, H, rs), f32)
        other = self.buf("eb_dx_b", (M, d), f32, zero=False)
        dyb_ready = False
        for i in reversed(range(len(self.t5["enc"]))):
            L = self.t5["enc"][i]
            nd = len(dyb_pair)
            dyb = dyb_pair[i % nd]
            par = i & 1 if batch else 0
            dyb2, dh, dqkv = dyb2_s[par], dh_s[par], dqkv_s[par]
            gb, gb2, gb3, gb4 = g_s[par]
            layer_jobs: Optional[list] = [] if batch else None
            if batch:
                # the launch that read this parity's buffers two layers ago (at_wi: the launch of the layer above, which holds the o / qkv
                # jobs of the layer two above and was handed over a whole layer ago)
                ev_old = grads_done.pop(i + 1 if at_wi else i + 2, None)
                if ev_old is not None:
                    torch.cuda.current_stream().wait_event(ev_old)
            else:
                # the LoRA weight-gradient launches of this layer run on the side stream beside the dX GEMMs; their inputs (dyb/dyb2/dh/
                # dqkv and the four g buffers) are written once per layer, so one join per layer keeps every reader ahead of its next writer
                self.side_join()
            # K^T / Q^T of this layer depend only on saved forward activations: transposed on the side stream while the FFN backward runs
            kq_ready = None
            t_saved = bool(self.enc_t_saved.get(i))
            if self.grad_side_stream_enabled and not t_saved:
                qkv_i = self.ws[f"e{i}_qkv"]
                kq_ready = torch.cuda.Event()

                def kq_job(qkv_i=qkv_i, kq_ready=kq_ready):
                    ops.head_transpose(self.v4(qkv_i, B, S, H, dk, inner), out=kt)
                    ops.head_transpose(self.v4(qkv_i, B, S, H, dk, 0), out=qt)
                    kq_ready.record()
                # queued: goes out with the wi group's record below (the previous layer's attention backward, the last reader of
                # kt / qt, is ahead of that point; this layer's attention backward is ~400 us behind it)
                self.side_defer(kq_job)
            # x_out = xm + drop(wo(y));  y = drop(gelu(wi_0 xn2) * wi_1 xn2)
            # (the bf16 operands dyb / dyb2 = dropout-backward(dx) are written by the RMSNorm backward that produced dx — one launch
            # and one 16 MB read fewer per sub-layer; only the top layer, whose dx comes from the decoder, casts on its own)
            if not dyb_ready:
                ops.cast_dropout(dx, out_bf16=dyb, drop=self.drop(L["sites"][3], p))
            if fuse_g:
                gb = gbw[i % 3]
            if w4b:
                self.lg_bwd(L["wo"], dyb, self.ws[f"e{i}_y"], self.ws[f"e{i}_u_wo"], gb, None, side=True, flush=False, collect=layer_jobs,
                            parts=dyact_p, parts_cfg=cfg_wo, g_ready=fuse_g and dyb_ready)
                ops.gated_gelu_bwd(dyact_p[0], self.ws[f"e{i}_h"], dh, drop=self.drop(L["sites"][2], p), dy_ext=dyact_p[1],
                                   ext_drop=self.drop(L["wo"].site, c.lora_dropout))
                self.lg_bwd(L["wi"], dh, self.ws[f"e{i}_xn2"], self.ws[f"e{i}_u_wi"], gb2, None, side=True, collect=layer_jobs,
                            parts=dxn_p_wi, parts_cfg=cfg_wi)
            else:
                self.lg_bwd(L["wo"], dyb, self.ws[f"e{i}_y"], self.ws[f"e{i}_u_wo"], gb, dyact, side=True, tile_cfg=_ENC_BWD_CFG[0], flush=False,
                            prefetch=self.enc_pf_bwd([L["wi"]], M), collect=layer_jobs, g_ready=fuse_g and dyb_ready)
                ops.gated_gelu_bwd(dyact, self.ws[f"e{i}_h"], dh, drop=self.drop(L["sites"][2], p))
                self.lg_bwd(L["wi"], dh, self.ws[f"e{i}_xn2"], self.ws[f"e{i}_u_wi"], gb2, dxn, side=True, tile_cfg=_ENC_BWD_CFG[1],
                            prefetch=self.enc_pf_bwd([L["o"]], M), collect=layer_jobs)
            if at_wi:
                # ONE hand-over per layer: behind the K^T / Q^T job go the weight-gradient pairs that are ready here — wo, wi of this layer,
                # o, qkv of the layer above — and run beside the o product and the attention backward
                jobs_now = carry + layer_jobs
                layer_jobs = []
                if jobs_now:
                    ev_done = torch.cuda.Event()

                    def grads_job(jobs=jobs_now, ev_done=ev_done):
                        ops.lora_grads_batched(jobs)
                        ev_done.record()
                    self.side_defer(grads_job)
                    grads_done[i] = ev_done
                self.side_flush()
            elif batch and kq_ready is not None:
                self.side_flush()      # (the K^T / Q^T job queued above must go out here: this layer's attention backward waits for it)
            dxn_wi = dxn_p_wi if w4b else dxn
            ext_wi = dict(ext_drop=self.drop(L["wi"].site, c.lora_dropout), ext_part=True) if w4b else {}
            if self.fuse_bwd_cast:
                ops.rmsnorm_bwd(dxn_wi, self.ws[f"e{i}_xm"], L["ln1"], c.t5_eps, other, dx_add=dx, out_bf16=dyb2, out_drop=self.drop(L["sites"][1], p),
                                g_prod=(L["o"].bblk, gb3) if fuse_g else None, **ext_wi)
            else:
                ops.rmsnorm_bwd(dxn_wi, self.ws[f"e{i}_xm"], L["ln1"], c.t5_eps, other, dx_add=dx, **ext_wi)
                ops.cast_dropout(other, out_bf16=dyb2, drop=self.drop(L["sites"][1], p))
            dx, other = other, dx
            # xm = x_in + drop(o(attn(qkv(xn))))
            dot_done = self.lg_bwd(L["o"], dyb2, self.ws[f"e{i}_o"], self.ws[f"e{i}_u_o"], gb3, do, side=True, tile_cfg=_ENC_BWD_CFG[2], flush=False,
                                   tout=(dot,) if self.tout_ok(dk, B, S, 2) else None, t_rows=S, collect=layer_jobs, g_ready=fuse_g)
            qkv, o = self.ws[f"e{i}_qkv"], self.ws[f"e{i}_o"]
            q4, k4, v4 = self.v4(qkv, B, S, H, dk, 0), self.v4(qkv, B, S, H, dk, inner), self.v4(qkv, B, S, H, dk, 2 * inner)
            do4 = self.v4(do, B, S, H, dk)
            if not dot_done:
                ops.head_transpose(do4, out=dot)
            kt_x, qt_x = kt, qt
            if t_saved:
                kt_x, qt_x = self.ws[f"e{i}_kt"], self.ws[f"e{i}_qt"]
            elif kq_ready is not None:
                torch.cuda.current_stream().wait_event(kq_ready)
            else:
                ops.head_transpose(k4, out=kt)
                ops.head_transpose(q4, out=qt)
            ops.attention_bwd(q4, k4, v4, self.v4(o, B, S, H, dk), do4, kt_x, qt_x, dot, self.ws[f"e{i}_lse"], delta,
                              self.v4(dqkv, B, S, H, dk, 0), self.v4(dqkv, B, S, H, dk, inner), self.v4(dqkv, B, S, H, dk, 2 * inner),
                              scale=1.0, bias_lut=self.lut_enc, kmask=kmask, drop=self.drop(L["sites"][0], p),
                              drop_bits=self.ws.get(f"e{i}_dbits") if self.drop(L["sites"][0], p) is not None else None)
            if w4b:
                self.lg_bwd(L["qkv"], dqkv, self.ws[f"e{i}_xn"], self.ws[f"e{i}_u_qkv"], gb4, None, side=True, collect=layer_jobs,
                            parts=dxn_p_qkv, parts_cfg=cfg_qkv)
            else:
                self.lg_bwd(L["qkv"], dqkv, self.ws[f"e{i}_xn"], self.ws[f"e{i}_u_qkv"], gb4, dxn, side=True, tile_cfg=_ENC_BWD_CFG[3],
                            prefetch=self.enc_pf_bwd([self.t5["enc"][i - 1]["wo"]], M) if i > 0 else None, collect=layer_jobs)
            dxn_qkv = dxn_p_qkv if w4b else dxn
            ext_qkv = dict(ext_drop=self.drop(L["qkv"].site, c.lora_dropout), ext_part=True) if w4b else {}
            if at_wi:
                carry = layer_jobs          # (o, qkv: they leave with the layer below's hand-over)
            elif batch and layer_jobs:   # the layer's four weight-gradient pairs: one launch, one hand-over
                ev_done = torch.cuda.Event()

                def grads_job(jobs=layer_jobs, ev_done=ev_done):
                    ops.lora_grads_batched(jobs)
                    ev_done.record()
                self.side_defer(grads_job)
                self.side_flush()
                grads_done[i] = ev_done
            if i > 0 and self.fuse_bwd_cast:   # ... and the layer below's first operand
                ops.rmsnorm_bwd(dxn_qkv, self.ws[f"e{i}_xin"], L["ln0"], c.t5_eps, other, dx_add=dx, out_bf16=dyb_pair[(i - 1) % nd],
                                out_drop=self.drop(self.t5["enc"][i - 1]["sites"][3], p),
                                g_prod=(self.t5["enc"][i - 1]["wo"].bblk, gbw[(i - 1) % 3]) if fuse_g else None, **ext_qkv)
                dyb_ready = True
            else:
                ops.rmsnorm_bwd(dxn_qkv, self.ws[f"e{i}_xin"], L["ln0"], c.t5_eps, other, dx_add=dx, **ext_qkv)
                dyb_ready = False
            dx, other = other, dx
        if at_wi and carry:
            self.side_defer(lambda jobs=carry: ops.lora_grads_batched(jobs))
        self.side_join()
        dinp = self.buf("eb_dinp", (M, d), f32, zero=False)
        ops.cast_dropout(dx, out_f32=dinp, drop=self.drop(self.t5["sites"][0], p))
        return dinp

    # ---- decoder + LM head + loss (forward and backward) ---------------------------------------------------------
    cross_kv_batched = os.environ.get("MRB_CKV_BATCH", "1") == "1"

    dec_grid_follows_reserve = os.environ.get("MRB_DEC_GRID_AUTO", "1") == "1"
    ckv_fwd_chunks = tuple(int(x) for x in os.environ.get("MRB_CKV_FWD_CHUNKS", "2,6,8,8").split(","))
    ckv_min_rows = int(os.environ.get("MRB_CKV_MIN_ROWS", "512"))

    def cross_kv_all(self, enc: torch.Tensor, B: int, S: int, prefix: str, events: bool = False):
        """Cross-attention K / V of ALL decoder layers for one encoder output, in CHUNKS of layers (round 4; chunk sizes ckv_fwd_chunks: the
        first chunk is small so that decoder layer 0 does not wait for everything): per chunk the LoRA "down" products of its adapters (one
        batched thin launch, each layer with its own lora_dropout call site) and ONE GEMM [B S, d] x [d, layers * 2 * inner] whose
        output-column group of a layer takes that layer's "down" activations as its K extension and whose epilogue writes K^T and V^T.
        Until round 3: per layer a thin launch, a GEMM and two head_transpose launches (modeling_t5.py:561-599 does it layer by layer
        inside the decoder).  events: record an event behind every chunk (the caller runs this on a side stream).  Returns per layer
        (K rows view, V^T, K^T, u view, ckv view, event or None), or None when the stacked form does not apply (d_kv != 64, several clips
        of a length that is not a multiple of 32, per-adapter masks, short inputs — below ckv_min_rows rows the decoder-style streaming
        projection of each layer is the better kernel: Charades-STA's 72 rows)."""
        ca = getattr(self, "ckv_all", None)
        c = self.cfg
        H, dk = c.t5_heads, c.d_kv
        if (ca is None or not self.cross_kv_batched or not self.tout_ok(dk, B, S) or B * S < self.ckv_min_rows
                or (c.lora_mask_per_adapter and self.training and c.lora_dropout > 0)):
            return None
        Lc, N, K, R = ca["L"], ca["N"], ca["K"], ca["R"]
        Me = B * S
        u_all = self.buf(prefix + "u_ckv_all", (Me, Lc * 64), bf16)
        ckv_all = self.buf(prefix + "ckv_all", (Me, Lc * N), bf16, zero=False)
        t_all = self.buf(prefix + "ckvT_all", (2 * Lc, B, H, 64, ops.rup32(S)), bf16)
        out = []
        i0 = 0
        sizes = list(self.ckv_fwd_chunks)
        while i0 < Lc:
            i1 = min(Lc, i0 + (sizes.pop(0) if sizes else self.ckv_fwd_chunks[-1]))
            G = i1 - i0
            ops.lora_rows_batched(enc, ca["acat"][i0 * R:], u_all[:, i0 * 64:], K, G, a_gstride=R * K, u_gstride=64, R=R,
                                  drop=self.drop(ca["site0"] + i0 * ca["site_stride"], c.lora_dropout), site_stride=ca["site_stride"])
            ops.gemm(enc, ca["W"][i0 * N:i1 * N], ckv_all[:, i0 * N:i1 * N], aext=u_all[:, i0 * 64:], wext=ca["wext"][i0 * N:i1 * N], ext_group_n=N,
                     tout=t_all[2 * i0:2 * i1], t_rows=S)
            ev = None
            if events:
                ev = torch.cuda.Event()
                ev.record()
            for i in range(i0, i1):
                out.append((self.v4(ckv_all, B, S, H, dk, i * N), t_all[2 * i + 1], t_all[2 * i], u_all[:, i * 64:(i + 1) * 64], ckv_all[:, i * N:(i + 1) * N],
                            ev if i == i0 else None))   # (stream order: a chunk's later layers are behind its first layer's wait)
            i0 = i1
        return out

    ckv_bwd_chunks = tuple(int(x) for x in os.environ.get("MRB_CKV_BWD_CHUNKS", "10,8,4,2").split(","))

    def ckv_chunk_bwd(self, i0: int, i1: int, dckv_all: torch.Tensor, g_all: torch.Tensor, enc: torch.Tensor, denc: torch.Tensor):
        """Backward of the cross-attention K / V projections of decoder layers [i0, i1) (peft lora.Linear backward around modeling_t5.py:
        561-599), launched on whatever stream is current: g = dy (sB) of every layer (one batched thin launch), the adapters' weight
        gradients (one launch per layer), the rank-8 input-gradient terms of all layers with their own lora_dropout masks (one pass over
        denc), and denc += dy_chunk W_chunk as ONE GEMM over the chunk's (i1 - i0) * 2 * inner output features."""
        ca, c = self.ckv_all, self.cfg
        N, K, R = ca["N"], ca["K"], ca["R"]
        G = i1 - i0
        ops.lora_rows_batched(dckv_all[:, i0 * N:], ca["bblk"][i0 * R:], g_all[:, i0 * 64:], N, G, x_gstride=N, a_gstride=R * N, u_gstride=64, R=R)
        for i in range(i0, i1):
            g = self.t5["dec"][i]["ckv"]
            ads = g.adapters
            ops.lora_grads(dckv_all[:, i * N:(i + 1) * N], self.ws[f"d{i}_u_ckv"], enc, g_all[:, i * 64:(i + 1) * 64], [a.dBt for a in ads], [a.row0 for a in ads],
                           [a.out for a in ads], [a.dA for a in ads], g.K, drop=self.drop(g.site, c.lora_dropout))
        ops.lora_dx_add_batched(denc, g_all[:, i0 * 64:], ca["acat"][i0 * R:], K, G, g_gstride=64, a_gstride=R * K, R=R,
                                drop=self.drop(ca["site0"] + i0 * ca["site_stride"], c.lora_dropout), site_stride=ca["site_stride"])
        Me = denc.shape[0]
        if self._enc_bwd_w4_ok(Me) and ((G * N) // 64) % 4 == 0:
            # round 5: [Me x d] is 64 tiles of 256x256 and K = G * 2 * inner is 8192 .. 40960: the 4-wave kernel's K-split, then one add
            ks, cfg = self.ksplit_cfg(Me, K, G * N)
            parts = self.buf("db_denc_parts", (8, Me, K), f32, zero=False)[:ks]
            ops.gemm_ksplit(dckv_all[:, i0 * N:i1 * N], ca["Wt"][:, i0 * N:i1 * N], parts, G * N, ks, tile_cfg=cfg)
            ops.sum_parts(parts, denc, residual=denc)
        else:
            ops.gemm(dckv_all[:, i0 * N:i1 * N], ca["Wt"][:, i0 * N:i1 * N], denc, residual=denc)

    @torch.no_grad()
    def t5_cross_kv(self, enc: torch.Tensor, Be: int, S: int):
        """Cross-attention K / V^T of every decoder layer for a fixed encoder output (inference: computed once per clip and reused by
        every decoding step and every beam).  Returns a list of (k4 view [Be,S,H,dk], V^T [Be,H,dkp,Sp]) per layer."""
        c = self.cfg
        H, dk = c.t5_heads, c.d_kv
        inner = H * dk
        Me = Be * S
        allkv = self.cross_kv_all(enc, Be, S, "g_")
        if allkv is not None:
            return [(k4, vt) for k4, vt, _, _, _, _ in allkv]
        cache = []
        for i, L in enumerate(self.t5["dec"]):
            ukv = self.buf(f"g{i}_u_ckv", (Me, 64), bf16)
            ckv = self.buf(f"g{i}_ckv", (Me, 2 * inner), bf16, zero=False)
            self.lg_fwd(L["ckv"], enc, ukv, ckv)
            vt = self.buf(f"g{i}_vt_c", (Be, H, ops.rup32(dk), ops.rup32(S)), bf16)
            ops.head_transpose(self.v4(ckv, Be, S, H, dk, inner), out=vt)
            cache.append((self.v4(ckv, Be, S, H, dk, 0), vt))
        return cache

    @torch.no_grad()
    @_with_attention_split
    def t5_decoder_forward(self, dec_ids: torch.Tensor, dec_mask: torch.Tensor, enc: torch.Tensor, B: int, S: int, kmask: torch.Tensor,
                           labels: Optional[torch.Tensor] = None, want_grad: bool = True, cross_cache=None, cross_batch: Optional[int] = None,
                           dev_in: Optional[dict] = None):
        """cross_cache (inference only): the output of t5_cross_kv for ``cross_batch`` encoder sequences; the B decoder sequences are
        then cross_batch groups of B / cross_batch beams, and — cross-attention having no causal structure — the beams of a group are
        simply more query rows against ITS encoder's keys: no per-beam copy of the encoder output, no K/V re-projection per step."""
        c = self.cfg
        d, H, dk, ff, p, V = c.d_model, c.t5_heads, c.d_kv, c.d_ff, c.t5_dropout, c.vocab
        inner = H * dk
        Ld = dec_ids.shape[1]
        R, Me = B * Ld, B * S
        # dev_in (the captured-step path, _layout_dev(static=True)): the decoder's integer inputs are already on the device, in buffers whose
        # addresses do not change from step to step — nothing below touches the host
        ids32 = dev_in["dec_ids32"] if dev_in is not None else self.h2d(dec_ids.reshape(-1), torch.int32)
        rows = dev_in["dec_rows"] if dev_in is not None else torch.arange(R, dtype=torch.int32, device=self.dev)
        x0 = self.buf("d_emb", (R, d), f32, zero=False)
        ops.row_copy(self.emb, ids32, x0, rows)
        x = self.buf("d_x0", (R, d), f32, zero=False)
        ops.cast_dropout(x0, out_f32=x, drop=self.drop(self.t5["sites"][2], p))
        vt_s = self.buf("d_vt_s", (B, H, ops.rup32(dk), ops.rup32(Ld)), bf16)
        dmask = dev_in["dec_mask"] if dev_in is not None else self.pad_mask(dec_mask)
        # Cross-attention K / V of all layers depend only on the encoder output: they are projected (LoRA included), and V^T / K^T
        # (for the backward) transposed, on the side stream while the main stream walks the decoder's serial chain; each layer waits
        # for its own event.  Per-layer buffers (the projections are kept for the backward anyway).
        ckv_side = []
        if cross_cache is None:
            use_side = self.grad_side_stream_enabled and want_grad and labels is not None and os.environ.get("MRB_DEC_FWD_SIDE", "1") == "1"
            st = self._grad_stream() if use_side else None
            if use_side:
                ev0 = torch.cuda.Event()
                ev0.record()
                st.wait_event(ev0)
            with torch.cuda.stream(st) if use_side else contextlib.nullcontext():
                allkv = self.cross_kv_all(enc, B, S, "d_", events=use_side)
                self.ckv_stacked = allkv is not None
                if allkv is not None:
                    for i, (k4, vt_i, kt_i, u_i, ckv_i, ready) in enumerate(allkv):
                        self.ws[f"d{i}_ckv"], self.ws[f"d{i}_kt_c"], self.ws[f"d{i}_u_ckv"] = ckv_i, kt_i, u_i
                        ckv_side.append((k4, vt_i, ready))
            for i, L in (enumerate(self.t5["dec"]) if allkv is None else ()):
                ukv = self.buf(f"d{i}_u_ckv", (Me, 64), bf16)
                ckv = self.buf(f"d{i}_ckv", (Me, 2 * inner), bf16, zero=False)
                vt_i = self.buf(f"d{i}_vt_c", (B, H, ops.rup32(dk), ops.rup32(S)), bf16)
                kt_i = self.buf(f"d{i}_kt_c", (B, H, ops.rup32(dk), ops.rup32(S)), bf16) if want_grad else None
                with torch.cuda.stream(st) if use_side else contextlib.nullcontext():
                    self.lg_fwd(L["ckv"], enc, ukv, ckv)
                    ops.head_transpose(self.v4(ckv, B, S, H, dk, inner), out=vt_i)
                    if kt_i is not None:
                        ops.head_transpose(self.v4(ckv, B, S, H, dk, 0), out=kt_i)
                    ready = None
                    if use_side:
                        ready = torch.cuda.Event()
                        ready.record()
                ckv_side.append((self.v4(ckv, B, S, H, dk, 0), vt_i, ready))
        for i, L in enumerate(self.t5["dec"]):
            xn = self.buf(f"d{i}_xn", (R, pad64(d)), bf16)
            u = self.buf(f"d{i}_u_qkv", (R, 64), bf16)
            qkv = self.buf(f"d{i}_qkv", (R, 3 * inner), bf16, zero=False)
            # (the fused decoder projection also writes V^T for this layer's attention and — training — Q^T / K^T / cross-Q^T for the backward:
            # no head_transpose launches on the decoder chain)
            keep_t = want_grad and labels is not None and dk == 64 and self.dec_tout_enabled
            qt_i = self.buf(f"d{i}_qt_s", (B, H, 64, ops.rup32(Ld)), bf16) if keep_t else None
            kt_i = self.buf(f"d{i}_kt_s", (B, H, 64, ops.rup32(Ld)), bf16) if keep_t else None
            qtc_i = self.buf(f"d{i}_qt_c", (B, H, 64, ops.rup32(Ld)), bf16) if keep_t else None
            t_done = self.norm_lg_fwd(x, L["ln0"], L["qkv"], xn, u, qkv, tout=(qt_i, kt_i, vt_s) if (dk == 64 and self.dec_tout_enabled) else None, t_rows=Ld)
            q4, k4, v4 = self.v4(qkv, B, Ld, H, dk, 0), self.v4(qkv, B, Ld, H, dk, inner), self.v4(qkv, B, Ld, H, dk, 2 * inner)
            self.dec_t_saved[i] = bool(t_done and keep_t)
            if not t_done:
                ops.head_transpose(v4, out=vt_s)
            o = self.buf(f"d{i}_o", (R, pad64(inner)), bf16)
            lse = self.buf(f"d{i}_lse", (B, H, ops.rup32(Ld)), f32)
            ops.attention_fwd(q4, k4, vt_s, self.v4(o, B, Ld, H, dk), lse, scale=1.0, bias_lut=self.lut_dec, kmask=dmask, causal=True, drop=self.drop(L["sites"][0], p))
            uo = self.buf(f"d{i}_u_o", (R, 64), bf16)
            x1 = self.buf(f"d{i}_x1", (R, d), f32, zero=False)
            self.lg_fwd(L["o"], o, uo, x1, residual=x, drop=self.drop(L["sites"][1], p))
            # cross attention
            xn1 = self.buf(f"d{i}_xn1", (R, pad64(d)), bf16)
            ucq = self.buf(f"d{i}_u_cq", (R, 64), bf16)
            cq = self.buf(f"d{i}_cq", (R, inner), bf16, zero=False)
            tc_done = self.norm_lg_fwd(x1, L["ln1"], L["cq"], xn1, ucq, cq, tout=(qtc_i,) if qtc_i is not None else None, t_rows=Ld)
            self.dec_tc_saved[i] = bool(tc_done and keep_t)
            co = self.buf(f"d{i}_co", (R, pad64(inner)), bf16)
            if cross_cache is None:
                ck4, vt_i, ready = ckv_side[i]
                if ready is not None:
                    torch.cuda.current_stream().wait_event(ready)
                lsec = self.buf(f"d{i}_lsec", (B, H, ops.rup32(Ld)), f32)
                ops.attention_fwd(self.v4(cq, B, Ld, H, dk), ck4, vt_i, self.v4(co, B, Ld, H, dk), lsec, scale=1.0, kmask=kmask, drop=self.drop(L["sites"][2], p))
            else:
                Bc = cross_batch
                rows = (B // Bc) * Ld  # query rows per encoder sequence: beams x positions
                ck4, vt_i = cross_cache[i]
                ops.attention_fwd(self.v4(cq, Bc, rows, H, dk), ck4, vt_i, self.v4(co, Bc, rows, H, dk), None, scale=1.0, kmask=kmask)
            uco = self.buf(f"d{i}_u_co", (R, 64), bf16)
            x2 = self.buf(f"d{i}_x2", (R, d), f32, zero=False)
            self.lg_fwd(L["co"], co, uco, x2, residual=x1, drop=self.drop(L["sites"][3], p))
            # FFN
            xn2 = self.buf(f"d{i}_xn2", (R, pad64(d)), bf16)
            uw = self.buf(f"d{i}_u_wi", (R, 64), bf16)
            y = self.buf(f"d{i}_y", (R, pad64(ff)), bf16)
            h = self.buf(f"d{i}_h", (R, 2 * ff), bf16, zero=False)
            self.norm_lg_fwd(x2, L["ln2"], L["wi"], xn2, uw, y, out2=h, gated=True, drop=self.drop(L["sites"][4], p), tile_cfg=2)
            uwo = self.buf(f"d{i}_u_wo", (R, 64), bf16)
            x3 = self.buf(f"d{i}_x3", (R, d), f32, zero=False)
            self.lg_fwd(L["wo"], y, uwo, x3, residual=x2, drop=self.drop(L["sites"][5], p))
            self.ws[f"d{i}_xin"] = x
            x = x3
        self.ws["d_xfinal_in"] = x
        nf = self.buf("d_nf", (R, d), f32, zero=False)
        ops.rmsnorm_fwd(x, self.t5["dec_final"], c.t5_eps, out_f32=nf)
        seq = self.buf("d_seq", (R, pad64(d)), bf16)
        ops.cast_dropout(nf, out_bf16=seq, drop=self.drop(self.t5["sites"][3], p))
        ulm = self.buf("d_u_lm", (R, 64), bf16)
        logits = self.buf("d_logits", (R, V), f32, zero=False)
        self.lg_fwd(self.t5["lm"], seq, ulm, logits)
        if labels is None:  # generation: logits only
            return None, logits
        lab = dev_in["labels32"] if dev_in is not None else self.h2d(labels.reshape(-1), torch.int32)
        loss = self.buf("loss", (1,), f32)
        loss.zero_()
        dlog = self.buf("d_dlogits", (R, V), bf16, zero=False) if want_grad else None
        if dev_in is not None:     # captured step: the valid-label count is a device word of the bucket's static set (not part of the key)
            ops.cross_entropy(logits, lab, 0.0, loss, dlog, n_valid_dev=dev_in["n_valid"])
        else:                       # (float32 division: the same bits as the device form)
            import numpy as np
            ops.cross_entropy(logits, lab, float(np.float32(1.0) / np.float32(max(int((labels != -100).sum()), 1))), loss, dlog)
        return loss, logits

    # ---- incremental decoding (generate): self-attention K / V cache, one new position per call
    @torch.no_grad()
    def t5_decode_begin(self, R: int, max_len: int, alt_cache: bool = False) -> dict:
        """State of an incremental decode of R sequences (beams x clips) of at most ``max_len`` positions: the self-attention keys and
        values of every decoder layer, row-major like the qkv buffer they are cut from: [2 (k, v), layers, R, Lmax, H * d_kv] bf16.
        alt_cache: also a second cache of the same shape — a step whose ``parents`` live on the device re-orders the cache by copying
        it into the other buffer (ops.kv_gather_rows: parents repeat, so not in place) and swaps the two."""
        c = self.cfg
        assert max_len <= 128, "incremental decode: the shifted relative-position LUT covers 128 positions"
        inner = c.t5_heads * c.d_kv
        Lmax = ops.rup32(max_len)
        kv = self.buf("g_self_kv", (2, len(self.t5["dec"]), R, Lmax, inner), bf16)
        if getattr(self, "lut_dec_pad", None) is None:
            # the kernels index the bias LUT with clamp(key - query_row, -128, 128) + 128 and the one query of a step is row 0 of ITS
            # launch but position t of the sequence: a base pointer moved back by t gives lut[(key - t) + 128] (no clamp can trigger
            # below 128 positions); 128 floats of front padding keep the moved pointer inside the allocation
            self.lut_dec_pad = torch.cat([torch.zeros(128, dtype=f32, device=self.dev), self.lut_dec.reshape(-1)])
        state = {"kv": kv, "t": 0, "R": R, "Lmax": Lmax}
        if alt_cache:
            state["kv_alt"] = self.buf("g_self_kv_alt", kv.shape, bf16)
        return state

    @torch.no_grad()
    @_with_attention_split
    def t5_decode_step(self, state: dict, tokens: torch.Tensor, parents: Optional[torch.Tensor], cross_cache, cross_batch: int, kmask):
        """One decoder position for R sequences: tokens [R] (the newest token of each), parents [R] (row of the previous call each
        sequence extends; None = unchanged order) -> fp32 logits [R, vocab] of the next token.  Host tensors, or DEVICE tensors (int32:
        tokens index the embedding table as they are, parents always gather the cache into the state's second buffer — nothing is
        uploaded or compared, so the host never waits; needs t5_decode_begin(alt_cache=True)).  modeling_t5.py:747-826 with
        use_cache=True: the new position's K / V are appended to the cache, the query attends to positions 0..t (nothing to mask: the
        causal mask of the last row is empty), cross-attention reads the per-clip K / V of t5_cross_kv."""
        c = self.cfg
        d, H, dk, ff, V = c.d_model, c.t5_heads, c.d_kv, c.d_ff, c.vocab
        inner = H * dk
        R, t, kv, Lmax = state["R"], state["t"], state["kv"], state["Lmax"]
        assert not self.training and tokens.numel() == R and t < Lmax
        if state.get("fused"):
            return self._t5_decode_step_fused(state, tokens, parents, cross_cache, cross_batch, kmask)
        if parents is not None and parents.is_cuda:
            assert parents.dtype == torch.int32 and parents.numel() == R and "kv_alt" in state, "device parents: int32 [R] and t5_decode_begin(alt_cache=True)"
            if t > 0:
                ops.kv_gather_rows(kv, state["kv_alt"], parents, t)
                kv, state["kv"], state["kv_alt"] = state["kv_alt"], state["kv_alt"], kv
        elif parents is not None and t > 0 and not torch.equal(parents, torch.arange(R)):
            kv[:, :, :, :t] = kv[:, :, :, :t].index_select(2, self.h2d(parents, torch.int64))
        rows = torch.arange(R, dtype=torch.int32, device=self.dev)
        x = self.buf("s_x", (R, d), f32, zero=False)
        ops.row_copy(self.emb, self.h2d(tokens.reshape(-1), torch.int32), x, rows)
        lut = self.lut_dec_pad[128 - t:]
        xn = self.buf("s_xn", (R, pad64(d)), bf16)
        u = {k: self.buf("s_u_" + k, (R, 64), bf16) for k in ("qkv", "o", "cq", "co", "wi", "wo", "lm")}
        qkv = self.buf("s_qkv", (R, 3 * inner), bf16, zero=False)
        o = self.buf("s_o", (R, pad64(inner)), bf16)
        cq = self.buf("s_cq", (R, inner), bf16, zero=False)
        co = self.buf("s_co", (R, pad64(inner)), bf16)
        y = self.buf("s_y", (R, pad64(ff)), bf16)
        xa, xb = self.buf("s_xa", (R, d), f32, zero=False), self.buf("s_xb", (R, d), f32, zero=False)
        vt = self.buf("s_vt", (R, H, ops.rup32(dk), ops.rup32(t + 1)), bf16)
        Bc = cross_batch
        for i, L in enumerate(self.t5["dec"]):
            self.norm_lg_fwd(x, L["ln0"], L["qkv"], xn, u["qkv"], qkv)
            kv[:, i, :, t] = qkv[:, inner:].view(R, 2, inner).transpose(0, 1)
            k4 = torch.as_strided(kv, (R, t + 1, H, dk), (Lmax * inner, inner, dk, 1), kv[0, i].storage_offset())
            v4 = torch.as_strided(kv, (R, t + 1, H, dk), (Lmax * inner, inner, dk, 1), kv[1, i].storage_offset())
            ops.head_transpose(v4, out=vt)
            ops.attention_fwd(self.v4(qkv, R, 1, H, dk, 0), k4, vt, self.v4(o, R, 1, H, dk), None, scale=1.0, bias_lut=lut)
            self.lg_fwd(L["o"], o, u["o"], xa, residual=x)
            self.norm_lg_fwd(xa, L["ln1"], L["cq"], xn, u["cq"], cq)
            ck4, vt_c = cross_cache[i]
            ops.attention_fwd(self.v4(cq, Bc, R // Bc, H, dk), ck4, vt_c, self.v4(co, Bc, R // Bc, H, dk), None, scale=1.0, kmask=kmask)
            self.lg_fwd(L["co"], co, u["co"], xb, residual=xa)
            self.norm_lg_fwd(xb, L["ln2"], L["wi"], xn, u["wi"], y, gated=True, tile_cfg=2)
            self.lg_fwd(L["wo"], y, u["wo"], x, residual=xb)
        nf = self.buf("s_nf", (R, pad64(d)), bf16)
        ops.rmsnorm_fwd(x, self.t5["dec_final"], c.t5_eps, out_bf16=nf)
        logits = self.buf("s_logits", (R, V), f32, zero=False)
        self.lg_fwd(self.t5["lm"], nf, u["lm"], logits)
        state["t"] = t + 1
        return logits

    # ---- opt-in (state["fused"]): the self-attention block of a decode step as ONE launch per layer (csrc/decode.hip) instead of the
    # strided copy into the cache, the head_transpose of the whole V cache and the MFMA tile kernel on one query row — and, with device
    # parents, instead of the kv_gather_rows pass over the complete cache: the kernel stores the rows it reads for the attention into the
    # other cache buffer.  Nothing in these launches depends on the position through a shape, a stride or a pointer.
    def _decode_fused_body(self, kv_src, kv_dst, tok32, parents, cross_cache, cross_batch: int, kmask, pos: Optional[int] = None, pos_dev=None):
        """every launch of one fused decode step: tok32 / parents int32 on the device (parents None: cache in place, kv_dst is kv_src);
        the position is ``pos`` or the device word ``pos_dev``.  Returns the logits workspace."""
        c = self.cfg
        d, H, dk, ff, V = c.d_model, c.t5_heads, c.d_kv, c.d_ff, c.vocab
        inner = H * dk
        R = kv_src.shape[2]
        rows = self.ws.get("s_rows")
        if rows is None or rows.numel() < R:
            rows = self.ws["s_rows"] = torch.arange(max(R, 64), dtype=torch.int32, device=self.dev)
        x = self.buf("s_x", (R, d), f32, zero=False)
        ops.row_copy(self.emb, tok32, x, rows[:R])
        xn = self.buf("s_xn", (R, pad64(d)), bf16)
        u = {k: self.buf("s_u_" + k, (R, 64), bf16) for k in ("qkv", "o", "cq", "co", "wi", "wo", "lm")}
        qkv = self.buf("s_qkv", (R, 3 * inner), bf16, zero=False)
        o = self.buf("s_o", (R, pad64(inner)), bf16)
        cq = self.buf("s_cq", (R, inner), bf16, zero=False)
        co = self.buf("s_co", (R, pad64(inner)), bf16)
        y = self.buf("s_y", (R, pad64(ff)), bf16)
        xa, xb = self.buf("s_xa", (R, d), f32, zero=False), self.buf("s_xb", (R, d), f32, zero=False)
        Bc = cross_batch
        for i, L in enumerate(self.t5["dec"]):
            self.norm_lg_fwd(x, L["ln0"], L["qkv"], xn, u["qkv"], qkv)
            ops.decode_self_attention(kv_src, kv_dst, qkv, o, self.lut_dec, i, H, pos=pos, pos_dev=pos_dev, parents=parents, scale=1.0)
            self.lg_fwd(L["o"], o, u["o"], xa, residual=x)
            self.norm_lg_fwd(xa, L["ln1"], L["cq"], xn, u["cq"], cq)
            ck4, vt_c = cross_cache[i]
            ops.attention_fwd(self.v4(cq, Bc, R // Bc, H, dk), ck4, vt_c, self.v4(co, Bc, R // Bc, H, dk), None, scale=1.0, kmask=kmask)
            self.lg_fwd(L["co"], co, u["co"], xb, residual=xa)
            self.norm_lg_fwd(xb, L["ln2"], L["wi"], xn, u["wi"], y, gated=True, tile_cfg=2)
            self.lg_fwd(L["wo"], y, u["wo"], x, residual=xb)
        nf = self.buf("s_nf", (R, pad64(d)), bf16)
        ops.rmsnorm_fwd(x, self.t5["dec_final"], c.t5_eps, out_bf16=nf)
        logits = self.buf("s_logits", (R, V), f32, zero=False)
        self.lg_fwd(self.t5["lm"], nf, u["lm"], logits)
        return logits

    def _decode_fused_buffers(self, state: dict, parents):
        """(kv_src, kv_dst, parents for the kernel) of the next fused step; device parents swap the state's two cache buffers"""
        R, t, kv = state["R"], state["t"], state["kv"]
        if parents is not None and parents.is_cuda:
            assert parents.dtype == torch.int32 and parents.numel() == R and "kv_alt" in state, "device parents: int32 [R] and t5_decode_begin(alt_cache=True)"
            dst = state["kv_alt"]
            state["kv"], state["kv_alt"] = dst, kv      # (every step, position 0 included: the direction of a step is its parity)
            return kv, dst, parents
        if parents is not None and t > 0 and not torch.equal(parents, torch.arange(R)):
            kv[:, :, :, :t] = kv[:, :, :, :t].index_select(2, self.h2d(parents, torch.int64))
        return kv, kv, None

    def _t5_decode_step_fused(self, state: dict, tokens, parents, cross_cache, cross_batch: int, kmask):
        src, dst, par = self._decode_fused_buffers(state, parents)
        logits = self._decode_fused_body(src, dst, self.h2d(tokens.reshape(-1), torch.int32), par, cross_cache, cross_batch, kmask, pos=state["t"])
        state["t"] += 1
        return logits

    # ---- opt-in: the fused step with DEVICE tokens / parents as a captured graph.  The position is a device word that the graph itself
    # increments, so one graph per direction of the cache ping-pong serves every position of every later call with the same buffers.
    _dec_graphs = None
    dec_graph_captures = 0     # (counted per engine: the increments below bind instance attributes)
    dec_graph_replays = 0

    @torch.no_grad()
    @_with_attention_split
    def t5_decode_step_graph(self, state: dict, tokens: torch.Tensor, parents: torch.Tensor, cross_cache, cross_batch: int, kmask):
        """t5_decode_step for a fused state and int32 device tokens / parents.  Position 0 of a decode runs eager (it creates every named
        workspace and sets the position word); every later position is one replay of the graph of its direction, captured when first needed.
        Key: (R, cross_batch, S, Lmax), the addresses of the cross cache, the mask, tokens, parents and of the step's own workspaces; a
        mismatch captures anew, the oldest of more than ``graph_max_buckets`` keys is dropped."""
        from collections import OrderedDict
        R, t, Lmax = state["R"], state["t"], state["Lmax"]
        assert not self.training and state.get("fused") and tokens.is_cuda and tokens.dtype == torch.int32 and tokens.numel() == R and t < Lmax
        pos_dev = self.buf("s_pos", (1,), torch.int32)
        src, dst, par = self._decode_fused_buffers(state, parents)
        tok32 = tokens.reshape(-1)
        state["t"] = t + 1
        if kmask is not None:      # (pad_mask builds a fresh tensor per call: the graphs read the key mask from a workspace of their own)
            static_mask = self.buf("s_kmask", kmask.shape, kmask.dtype)
            if t == 0:
                static_mask.copy_(kmask)
            kmask = static_mask
        if t == 0:
            pos_dev.zero_()
            logits = self._decode_fused_body(src, dst, tok32, par, cross_cache, cross_batch, kmask, pos_dev=pos_dev)
            pos_dev.add_(1)
            state["graph_ptrs"] = tuple(self.ws[n].data_ptr() for n in sorted(self.ws) if n.startswith("s_") and torch.is_tensor(self.ws[n]))
            return logits
        S = int(cross_cache[0][0].shape[1])
        key = (R, int(cross_batch), S, Lmax, tuple((k4.data_ptr(), vt.data_ptr()) for k4, vt in cross_cache),
               None if kmask is None else kmask.data_ptr(), tok32.data_ptr(), par.data_ptr(), state["graph_ptrs"])   # (the s_* workspaces: s_kmask among them)
        if self._dec_graphs is None:
            self._dec_graphs = OrderedDict()
        rec = self._dec_graphs.get(key)
        if rec is None:
            # (a workspace that grew has moved for good: keys holding its old address can never be met again and would only keep
            # their graphs alive until the cap evicts them)
            for stale in [k for k in self._dec_graphs if k[-1] != state["graph_ptrs"]]:
                self._dec_graphs.pop(stale).clear()
            rec = self._dec_graphs[key] = {}
            while len(self._dec_graphs) > self.graph_max_buckets:
                self._dec_graphs.popitem(last=False)[1].clear()
        else:
            self._dec_graphs.move_to_end(key)
        direction = (src.data_ptr(), dst.data_ptr())
        entry = rec.get(direction)
        if entry is None:
            def fn():
                out = self._decode_fused_body(src, dst, tok32, par, cross_cache, cross_batch, kmask, pos_dev=pos_dev)
                pos_dev.add_(1)
                return out
            entry = rec[direction] = self._capture(fn)     # (records only: the replay below runs the step)
            self.dec_graph_captures += 1
        entry[0].replay()
        self.dec_graph_replays += 1
        return entry[1]

    @torch.no_grad()
    @_with_attention_split
    def t5_decoder_backward(self, enc: torch.Tensor, B: int, S: int, Ld: int, kmask: torch.Tensor, dec_mask: torch.Tensor,
                            dev_in: Optional[dict] = None) -> torch.Tensor:
        """Backward from d_dlogits.  Returns fp32 grad of the encoder output [B*S, d]."""
        c = self.cfg
        d, H, dk, ff, p, V = c.d_model, c.t5_heads, c.d_kv, c.d_ff, c.t5_dropout, c.vocab
        inner = H * dk
        R, Me = B * Ld, B * S
        dmask = dev_in["dec_mask"] if dev_in is not None else self.pad_mask(dec_mask)
        gb = self.buf("db_g", (R, 64), bf16)
        dside = self.grad_side_stream_enabled and os.environ.get("MRB_DEC_SIDE", "1") == "1"
        gbs = [self.buf(f"db_g{j}", (R, 64), bf16) for j in range(6)]  # one g buffer per LoRA group of a layer (side-stream readers)
        dseq = self.buf("db_dseq", (R, d), f32, zero=False)
        self.lg_bwd(self.t5["lm"], self.ws["d_dlogits"], self.ws["d_seq"], self.ws["d_u_lm"], gb, dseq)
        t = self.buf("db_t", (R, d), f32, zero=False)
        ops.cast_dropout(dseq, out_f32=t, drop=self.drop(self.t5["sites"][3], p))
        dx = self.buf("db_dx_a", (R, d), f32, zero=False)
        other = self.buf("db_dx_b", (R, d), f32, zero=False)
        ops.rmsnorm_bwd(t, self.ws["d_xfinal_in"], self.t5["dec_final"], c.t5_eps, dx)
        denc = self.buf("db_denc", (Me, d), f32)
        denc.zero_()
        dybs = [self.buf(f"db_dyb{j}", (R, pad64(d)), bf16) for j in range(3)]
        dyact = self.buf("db_dyact", (R, ff), bf16, zero=False)
        dh = self.buf("db_dh", (R, 2 * ff), bf16, zero=False)
        dxn = self.buf("db_dxn", (R, d), f32, zero=False)
        do = self.buf("db_do", (R, inner), bf16, zero=False)
        dqkv = self.buf("db_dqkv", (R, 3 * inner), bf16, zero=False)
        dcq = self.buf("db_dcq", (R, inner), bf16, zero=False)
        rl, rs = ops.rup32(Ld), ops.rup32(S)
        kt_s, qt_s, dot_s = (self.buf(n, (B, H, ops.rup32(dk), rl), bf16) for n in ("db_kt_s", "db_qt_s", "db_dot_s"))
        delta = self.buf("db_delta", (B, H, rl), f32)
        dyb0_ready = False
        dyb0_pair = (dybs[0], self.buf("db_dyb0b", (R, pad64(d)), bf16))
        # round 4: with the stacked cross K / V projection (cross_kv_all) its backward runs per CHUNK of layers: dK / dV of all layers land
        # in one [Me, L * 2 * inner] buffer, and when the backward has passed the lowest layer of a chunk the chunk's three launches go to the
        # side stream (see ckv_chunk_bwd).  Chunks get smaller towards layer 0: only the last one is not hidden behind the decoder chain.
        stacked = bool(getattr(self, "ckv_stacked", False)) and getattr(self, "ckv_all", None) is not None
        chunk_starts: Dict[int, int] = {}
        if stacked:
            Lc = len(self.t5["dec"])
            dckv_all = self.buf("db_dckv_all", (Me, Lc * 2 * inner), bf16, zero=False)
            g_all = self.buf("db_ge_all", (Me, Lc * 64), bf16)
            hi = Lc
            for size in self.ckv_bwd_chunks:
                lo = max(0, hi - size)
                if hi > lo:
                    chunk_starts[lo] = hi
                hi = lo
            while hi > 0:     # (more layers than the schedule names: keep cutting chunks of the last size)
                lo = max(0, hi - self.ckv_bwd_chunks[-1])
                chunk_starts[lo] = hi
                hi = lo
        for i in reversed(range(len(self.t5["dec"]))):
            L = self.t5["dec"][i]
            # side stream (see the encoder backward): the LoRA weight-gradient launches of this layer, and the WHOLE backward of the
            # cross-attention K/V projection (it only feeds denc, which nobody reads before the encoder backward; per-layer dckv / g
            # buffers, the accumulation into denc stays in order on that stream).  One join per layer for the buffers written once per layer.
            self.side_join()
            dyb = dyb0_pair[i & 1]
            if not dyb0_ready:   # (top layer: dx comes from the final norm's backward; below, the previous layer's last RMSNorm backward wrote it)
                ops.cast_dropout(dx, out_bf16=dyb, drop=self.drop(L["sites"][5], p))
            self.lg_bwd(L["wo"], dyb, self.ws[f"d{i}_y"], self.ws[f"d{i}_u_wo"], gbs[0], dyact, side=dside, flush=False)
            ops.gated_gelu_bwd(dyact, self.ws[f"d{i}_h"], dh, drop=self.drop(L["sites"][4], p))
            self.lg_bwd(L["wi"], dh, self.ws[f"d{i}_xn2"], self.ws[f"d{i}_u_wi"], gbs[1], dxn, side=dside)
            # (the bf16 operand of the next sub-layer = dropout-backward(dx) is written by the RMSNorm backward that produces dx, as in the
            # encoder backward: one launch fewer per sub-layer)
            dyb = dybs[1]
            if self.fuse_bwd_cast:
                ops.rmsnorm_bwd(dxn, self.ws[f"d{i}_x2"], L["ln2"], c.t5_eps, other, dx_add=dx, out_bf16=dyb, out_drop=self.drop(L["sites"][3], p))
            else:
                ops.rmsnorm_bwd(dxn, self.ws[f"d{i}_x2"], L["ln2"], c.t5_eps, other, dx_add=dx)
                ops.cast_dropout(other, out_bf16=dyb, drop=self.drop(L["sites"][3], p))
            dx, other = other, dx
            # cross attention
            dot_done = self.lg_bwd(L["co"], dyb, self.ws[f"d{i}_co"], self.ws[f"d{i}_u_co"], gbs[2], do, side=dside, flush=False,
                                   tout=(dot_s,) if (dk == 64 and self.dec_tout_enabled) else None, t_rows=Ld)
            dckv = dckv_all[:, i * 2 * inner:(i + 1) * 2 * inner] if stacked else self.buf(f"db_dckv{i}", (Me, 2 * inner), bf16, zero=False)
            cq, ckv, co = self.ws[f"d{i}_cq"], self.ws[f"d{i}_ckv"], self.ws[f"d{i}_co"]
            q4, k4, v4 = self.v4(cq, B, Ld, H, dk), self.v4(ckv, B, S, H, dk, 0), self.v4(ckv, B, S, H, dk, inner)
            do4 = self.v4(do, B, Ld, H, dk)
            kt_c = self.ws[f"d{i}_kt_c"]  # made beside the forward (t5_decoder_forward)
            qt_x = qt_s
            if self.dec_tc_saved.get(i):
                qt_x = self.ws[f"d{i}_qt_c"]     # written by the forward's fused projection
            else:
                ops.head_transpose(q4, out=qt_s)
            if not dot_done:
                ops.head_transpose(do4, out=dot_s)
            ops.attention_bwd(q4, k4, v4, self.v4(co, B, Ld, H, dk), do4, kt_c, qt_x, dot_s, self.ws[f"d{i}_lsec"], delta,
                              self.v4(dcq, B, Ld, H, dk), self.v4(dckv, B, S, H, dk, 0), self.v4(dckv, B, S, H, dk, inner),
                              scale=1.0, kmask=kmask, drop=self.drop(L["sites"][2], p))
            if stacked:   # the cross K / V projections' backward in chunks of layers (see ckv_chunk_bwd); queued like the per-layer form
                if i in chunk_starts:
                    i1 = chunk_starts[i]
                    if dside:
                        self.side_defer(lambda i0=i, i1=i1: self.ckv_chunk_bwd(i0, i1, dckv_all, g_all, enc, denc))
                    else:
                        self.ckv_chunk_bwd(i, i1, dckv_all, g_all, enc, denc)
            elif dside:   # queued: goes out with the cq group's record
                ge_i, u_ckv_i = self.buf(f"db_ge{i}", (Me, 64), bf16), self.ws[f"d{i}_u_ckv"]
                self.side_defer(lambda L=L, dckv=dckv, ge_i=ge_i, u_ckv_i=u_ckv_i: self.lg_bwd(L["ckv"], dckv, enc, u_ckv_i, ge_i, denc, residual=denc))
            else:
                self.lg_bwd(L["ckv"], dckv, enc, self.ws[f"d{i}_u_ckv"], self.buf(f"db_ge{i}", (Me, 64), bf16), denc, residual=denc)
            self.lg_bwd(L["cq"], dcq, self.ws[f"d{i}_xn1"], self.ws[f"d{i}_u_cq"], gbs[3], dxn, side=dside)
            dyb = dybs[2]
            if self.fuse_bwd_cast:
                ops.rmsnorm_bwd(dxn, self.ws[f"d{i}_x1"], L["ln1"], c.t5_eps, other, dx_add=dx, out_bf16=dyb, out_drop=self.drop(L["sites"][1], p))
            else:
                ops.rmsnorm_bwd(dxn, self.ws[f"d{i}_x1"], L["ln1"], c.t5_eps, other, dx_add=dx)
                ops.cast_dropout(other, out_bf16=dyb, drop=self.drop(L["sites"][1], p))
            dx, other = other, dx
            # self attention
            dot_done = self.lg_bwd(L["o"], dyb, self.ws[f"d{i}_o"], self.ws[f"d{i}_u_o"], gbs[4], do, side=dside, flush=False,
                                   tout=(dot_s,) if (dk == 64 and self.dec_tout_enabled) else None, t_rows=Ld)
            qkv, o = self.ws[f"d{i}_qkv"], self.ws[f"d{i}_o"]
            q4, k4, v4 = self.v4(qkv, B, Ld, H, dk, 0), self.v4(qkv, B, Ld, H, dk, inner), self.v4(qkv, B, Ld, H, dk, 2 * inner)
            do4 = self.v4(do, B, Ld, H, dk)
            kt_x, qt_x = kt_s, qt_s
            if self.dec_t_saved.get(i):
                kt_x, qt_x = self.ws[f"d{i}_kt_s"], self.ws[f"d{i}_qt_s"]
            else:
                ops.head_transpose(k4, out=kt_s)
                ops.head_transpose(q4, out=qt_s)
            if not dot_done:
                ops.head_transpose(do4, out=dot_s)
            ops.attention_bwd(q4, k4, v4, self.v4(o, B, Ld, H, dk), do4, kt_x, qt_x, dot_s, self.ws[f"d{i}_lse"], delta,
                              self.v4(dqkv, B, Ld, H, dk, 0), self.v4(dqkv, B, Ld, H, dk, inner), self.v4(dqkv, B, Ld, H, dk, 2 * inner),
                              scale=1.0, bias_lut=self.lut_dec, kmask=dmask, causal=True, drop=self.drop(L["sites"][0], p))
            self.lg_bwd(L["qkv"], dqkv, self.ws[f"d{i}_xn"], self.ws[f"d{i}_u_qkv"], gbs[5], dxn, side=dside)
            if i > 0 and self.fuse_bwd_cast:   # ... and the layer below's first operand (its own buffer by layer parity: this layer's wo
                # group may still be reading dyb0_pair[i & 1] on the side stream)
                ops.rmsnorm_bwd(dxn, self.ws[f"d{i}_xin"], L["ln0"], c.t5_eps, other, dx_add=dx, out_bf16=dyb0_pair[(i - 1) & 1],
                                out_drop=self.drop(self.t5["dec"][i - 1]["sites"][5], p))
                dyb0_ready = True
            else:
                ops.rmsnorm_bwd(dxn, self.ws[f"d{i}_xin"], L["ln0"], c.t5_eps, other, dx_add=dx)
                dyb0_ready = False
            dx, other = other, dx
        # the decoder embeddings are frozen: nothing flows below dx
        self.side_join()  # denc (and the decoder adapters' gradients) are complete
        return denc

    # ------------------------------------------------------------------------------------------ whole step
    @torch.no_grad()
    def frames_forward(self, video: torch.Tensor):
        """video fp32 [B,T,3,IMG,IMG] -> frames_for_t5 fp32 [B*T*n, d]   (blip2_mr.py:444-510)"""
        c = self.cfg
        Bv, T = video.shape[:2]
        F_ = Bv * T
        Tv = (c.img // c.patch) ** 2 + 1
        xv = self._take_prefetched_vit(video)
        head_next, self._head_next = getattr(self, "_head_next", None), None
        if xv is None:
            xv = self.vit_forward(video.reshape(F_, 3, c.img, c.img), slot=self._vit_slot)
        elif head_next is not None:
            self.prefetch_vit_head(head_next)     # (this step runs no ViT kernel of its own: the ViT workspaces are free)
        img = self.buf("img", (F_ * Tv, pad64(c.vit_dim)), bf16)
        ops.layernorm_fwd(xv, self.lnv_w, self.lnv_b, self.ln_vision_eps, out_bf16=img)
        qb = self.qformer_forward(img, F_)
        fr = self.buf("frames", (F_ * c.num_query, c.d_model), f32, zero=False)
        if self.qf_prefetch and self.enc_prefetch and self.enc_prefetch[0] and fr.shape[0] >= 256:   # ... and t5_proj the first encoder layer's qkv weights
            ops.gemm_prefetch(self.t5["enc"][0]["qkv"].W, n_blocks=32)
        ops.gemm(qb, self.proj_wb, fr, bias=self.proj_b)
        if c.mean_pool:
            pooled = self.buf("frames_pooled", (F_, c.d_model), f32, zero=False)
            ops.mean_pool(fr.view(F_, c.num_query, c.d_model), pooled)
            return pooled, img, xv, qb
        return fr, img, xv, qb

    # ---- frozen-ViT look-ahead.  The ViT is frozen (freeze_vit: True), so its forward of the NEXT clip depends on nothing this
    # step computes.  It is enqueued on a second HIP stream once the T5 encoder forward has been issued and runs beside the T5
    # decoder, whose ~1700 launches on 12 tokens leave most of the CUs idle.  Its output goes to the other of two buffers (the current
    # one is still needed by this step's ln_vision backward); the next step picks it up after waiting on the completion event.
    grad_ready_hook: Optional[Callable[[str], None]] = None  # called with "lora" / "all" from forward_backward (see there)
    _vit_slot = 0
    _vit_ready = None
    _vit_stream = None
    vit_lookahead_blocks = None  # how many ViT blocks the look-ahead runs beside the decoder (None = all); the rest run in the next step
    vit_prefetch_hits = 0    # (class-wide tallies) steps that consumed a prefetched ViT output / prefetches issued but not matched
    vit_prefetch_misses = 0

    @staticmethod
    def _video_key(video: torch.Tensor):
        return (video.data_ptr(), tuple(video.shape), video._version)

    # Round 5: a HEAD leg of the look-ahead.  The step starts with ln_vision + Q-Former forward + t5_proj of the clip being trained: ~120 launches
    # of 5-25 us on 1920 rows (2.7 ms of wall clock, 1.8 ms of kernels on a fraction of the CUs) before the encoder forward fills the chip.
    # The first ``vit_head[0]`` blocks of the NEXT clip's frozen ViT run beside them, leaving ``vit_head[1]`` CUs to those launches; the first
    # leg proper (prefetch_vit, after the encoder forward has been issued) continues from there.  MRB_VIT_HEAD="blocks:reserve", 0 blocks = off.
    vit_head = tuple(int(x) for x in os.environ.get("MRB_VIT_HEAD", "2:128").split(":"))
    _vit_head_done = None
    vit_head_legs = 0        # (class-wide tally) first legs that continued a head leg

    def _first_leg_blocks(self, frames: int) -> int:
        """ViT blocks the look-ahead runs before its tail leg (prefetch_vit_tail runs the rest beside the Q-Former backward)"""
        c = self.cfg
        nb = c.vit_depth if self.vit_lookahead_blocks is None else max(1, min(c.vit_depth, int(self.vit_lookahead_blocks)))
        return max(1, nb - self._tail_blocks_for(frames))

    @torch.no_grad()
    def prefetch_vit_head(self, next_video: torch.Tensor):
        c = self.cfg
        F_ = next_video.shape[0] * next_video.shape[1]
        nh = min(int(self.vit_head[0]), self._first_leg_blocks(F_) - 1)     # (the first leg must have something left to continue with)
        if nh <= 0 or self._vit_ready is not None:
            return
        if self._vit_stream is None:
            self._vit_stream = torch.cuda.Stream(device=self.dev)
        start = torch.cuda.Event()
        start.record()
        slot = 1 - self._vit_slot
        with torch.cuda.stream(self._vit_stream):
            self._vit_stream.wait_event(start)
            with ops.gemm_cu_reserve(int(self.vit_head[1])):
                self.vit_forward(next_video.reshape(F_, 3, c.img, c.img), slot=slot, blocks=(0, nh))
        self._vit_head_done = (self._video_key(next_video), slot, nh)

    @torch.no_grad()
    def prefetch_vit(self, next_video: torch.Tensor):
        c = self.cfg
        if self._vit_stream is None:
            self._vit_stream = torch.cuda.Stream(device=self.dev)
        start = torch.cuda.Event()
        start.record()
        slot = 1 - self._vit_slot
        head, self._vit_head_done = self._vit_head_done, None
        with torch.cuda.stream(self._vit_stream):
            self._vit_stream.wait_event(start)
            F_ = next_video.shape[0] * next_video.shape[1]
            nb = self._first_leg_blocks(F_)
            frames = next_video.reshape(F_, 3, c.img, c.img)
            b0 = 0
            if head is not None and head[0] == self._video_key(next_video) and head[1] == slot and head[2] < nb:
                b0 = head[2]      # (the head leg ran blocks 0 .. b0-1 into this slot, on this stream)
                MrBlipEngine.vit_head_legs += 1
            for upto, reserve in self._reserve_schedule_for(F_):   # (first-leg blocks < upto run with `reserve` CUs left to the other streams)
                b1 = min(nb, upto)
                if b1 > b0:
                    with ops.gemm_cu_reserve(reserve):
                        xv = self.vit_forward(frames, slot=slot, blocks=(b0, b1))
                    b0 = b1
            done = torch.cuda.Event()
            done.record()
        self._vit_ready = (self._video_key(next_video), xv, done, slot, nb)
        self._vit_next = next_video

    # CUs the look-ahead's persistent GEMM kernels leave to the clip that is being trained.  Those kernels hold whole CUs for a whole
    # launch; without a reserve the other stream's short, latency-bound kernels (the decoder chain above all) queue behind them
    # (QVH, B = 1: 85.0 ms per step with 0, 80.3 with 32, 78.3 with 64, 80.3 with 96, 84.1 with 128 reserved CUs).
    vit_lookahead_reserve = int(os.environ.get("MRB_VIT_RESERVE", "64"))
    _vit_reserve_fixed = "MRB_VIT_RESERVE" in os.environ or "MRB_VIT_RESERVE_SCHED" in os.environ

    def _reserve_schedule_for(self, frames: int):
        """The reserve follows the look-ahead's size unless MRB_VIT_RESERVE[_SCHED] pins it.  With 60+ frames the ViT is the larger half
        of the step and 64 reserved CUs are the measured optimum (QVH 60 frames, QVH 4 x 60, ActivityNet 120: 48 / 64 / 80 -> +1.6 / 0 /
        +1.8 ms).  With 20 frames (Charades-STA) the ViT is 14 ms of a 35 ms step made of launch chains whose kernels run twice as long
        beside it: reserve 64 / 96 / 128 / 160 / 176 / 192 -> 35.05 / 33.49 / 32.97 / 32.42 / 32.51 / 35.18 ms.  Linear in between."""
        if self._vit_reserve_fixed:
            return self.vit_reserve_schedule
        r = 64 + max(0, 60 - int(frames)) * 12 // 5      # 60 frames -> 64, 20 frames -> 160
        return [(1 << 30, min(168, r // 8 * 8))]
    # optional per-block schedule "upto:reserve,upto:reserve" (experiments: the first blocks run beside the decoder's short kernels, the
    # later ones beside the encoder backward's GEMMs); default: one segment with vit_lookahead_reserve
    vit_reserve_schedule = ([(int(a), int(b)) for a, b in (seg.split(":") for seg in os.environ["MRB_VIT_RESERVE_SCHED"].split(","))]
                            if os.environ.get("MRB_VIT_RESERVE_SCHED") else [(1 << 30, int(os.environ.get("MRB_VIT_RESERVE", "64")))])
    vit_lookahead_early = os.environ.get("MRB_VIT_EARLY", "0") == "1"  # start beside the encoder forward instead of after it

    vit_tail_blocks = int(os.environ.get("MRB_VIT_TAIL", "5"))  # look-ahead blocks held back for prefetch_vit_tail()
    _vit_tail_fixed = "MRB_VIT_TAIL" in os.environ

    def _tail_blocks_for(self, frames: int) -> int:
        """Blocks of the look-ahead held back for the Q-Former backward.  Measured at the end of round 4 (profiles/r04_vit_tail.txt, three
        alternating sets): QVH 60 frames 5 / 6 / 7 / 8 blocks -> 67.40 / 67.26 / 67.09 / 67.30 ms; Charades-STA (20 frames) 5 / 7 -> 29.0 /
        29.5 ms; ActivityNet (120) equal; QVH x 4 clips (240 frames) 237.9 / 238.9 ms.  7 around 60 frames, 5 elsewhere; MRB_VIT_TAIL pins it."""
        if self._vit_tail_fixed:
            return int(self.vit_tail_blocks)
        return 7 if 40 <= int(frames) <= 80 else int(self.vit_tail_blocks)

    @torch.no_grad()
    def prefetch_vit_tail(self):
        """Second leg of the look-ahead: the ViT blocks the first leg left out are issued (same side stream) when the Q-Former backward
        starts — a short-kernel phase at the end of the step with idle CUs."""
        r = self._vit_ready
        if r is None or r[4] >= self.cfg.vit_depth:
            return
        c = self.cfg
        start = torch.cuda.Event()
        start.record()
        v = self._vit_next
        with torch.cuda.stream(self._vit_stream):
            self._vit_stream.wait_event(start)
            F_ = v.shape[0] * v.shape[1]
            with ops.gemm_cu_reserve(self._reserve_schedule_for(F_)[-1][1]):
                self.vit_forward(v.reshape(F_, 3, c.img, c.img), slot=r[3], blocks=(r[4], c.vit_depth))
            done = torch.cuda.Event()
            done.record()
        self._vit_ready = (r[0], r[1], done, r[3], c.vit_depth)

    def _take_prefetched_vit(self, video: torch.Tensor):
        r, self._vit_ready = self._vit_ready, None
        if r is None:
            return None
        if r[0] != self._video_key(video):
            MrBlipEngine.vit_prefetch_misses += 1
            torch.cuda.current_stream().wait_event(r[2])  # the side stream still owns the ViT workspaces until then
            return None
        torch.cuda.current_stream().wait_event(r[2])
        self._vit_slot = r[3]
        MrBlipEngine.vit_prefetch_hits += 1
        if r[4] < self.cfg.vit_depth:  # finish the remaining blocks here
            c = self.cfg
            F_ = video.shape[0] * video.shape[1]
            self.vit_forward(video.reshape(F_, 3, c.img, c.img), slot=r[3], blocks=(r[4], c.vit_depth))
        return r[1]

    @torch.no_grad()
    def forward_backward(self, video: torch.Tensor, layout: EncoderLayout, backward: bool = True, next_video: Optional[torch.Tensor] = None,
                         shard=None, train_frames: bool = True, frames: Optional[torch.Tensor] = None):
        """One micro-step: loss (device scalar) and, if ``backward``, gradients accumulated into self.grad.  ``next_video`` (optional):
        the next step's clip, whose frozen-ViT forward is overlapped with this step's decoder (see prefetch_vit).
        ``train_frames`` = False (round 6, the ANSWERER step of the video-QA path, forward_QA blip2_mr.py:325-431): the frame tokens are
        computed WITHOUT gradient (the reference runs ViT / ln_vision / Q-Former / t5_proj under torch.no_grad there), so the backward ends
        with the T5's LoRA gradients — no frame-token gradient, no t5_proj / Q-Former / ln_vision backward.  ``frames`` (with
        train_frames = False; ``video`` is then ignored): the [B * t * n, d_model] fp32 frame tokens themselves, produced by the engine
        that owns the shared towers (the localizer's).

        ``shard`` (mrblip.dist.FrameShard, optional): frame-sharded long-video mode (blip2_mr.py:444-445 — [B, T] is
        just a batch through ViT + Q-Former).  ``video`` then holds only THIS rank's frames [1, T_r, 3, IMG, IMG] of one clip whose
        ``layout`` describes all T frames: ViT / ln_vision / Q-Former / t5_proj run on the local frames, ONE all-gather assembles the
        [T * n, d_model] frame tokens on every rank, the T5 (replicated: same clip, same prompt, same dropout seed on every rank of
        the group) runs in full, and each rank continues the backward with ITS rows of the frame-token gradient — the replicated T5
        produced the same gradient everywhere, so the "reduce-scatter" of a sharded T5 degenerates to a slice.  The LoRA gradients
        are then identical on all ranks; t5_proj / ln_vision gradients are partial sums over local frames (FrameShard.combine_grads)."""
        c = self.cfg
        if frames is not None:
            assert not train_frames and next_video is None and shard is None, "precomputed frame tokens: the answerer step (no frame gradient, no look-ahead, no shard)"
            Bv, T = int(layout.attention_mask.shape[0]), 0
        else:
            Bv, T = video.shape[:2]
        F_ = Bv * T
        S, d = layout.S, c.d_model
        n = 1 if c.mean_pool else c.num_query
        sharded = shard is not None and shard.world > 1
        if sharded:
            assert Bv == 1 and T == shard.counts[shard.rank], "frame-sharded mode: one clip, this rank's frames only"
            shard.attach(self)   # (first step only) one dropout stream for the group's replicated T5, per-rank Q-Former call sites
        self.check_thin_role(block=False)   # verdict of an EARLIER step, if it has arrived (raises; see check_thin_role)
        if self.training:
            ops.seed_bump(self.seed)
        # round 4: the decoder's streaming projections run as many blocks as the look-ahead ViT leaves CUs (one round of resident blocks;
        # measured: 256 blocks beside a ViT that holds 192 CUs cost +0.4 ms per step, 64 blocks -0.3 ms); 0 = one block per CU
        if self.dec_grid_follows_reserve:
            nf = next_video.shape[0] * next_video.shape[1] if next_video is not None else 0
            ops.dec_proj_config(self._reserve_schedule_for(nf)[0][1] if next_video is not None else 0)   # (the first leg's first segment runs beside the decoder)
        self._mark("start")
        self._head_next = next_video if (backward and not sharded) else None
        if frames is not None:
            fr, img, xv, qb = frames, None, None, None
        else:
            self._qf_backward_follows = bool(backward)
            try:
                fr, img, xv, qb = self.frames_forward(video)
            finally:
                self._qf_backward_follows = False
        self._mark("frames_forward (ViT + ln_vision + Q-Former + t5_proj)")
        dev = self.dev
        use_graph = self._graph_wanted(Bv, S, backward, sharded) and frames is None
        L = self._layout_dev(layout, static=use_graph)
        inp = self.buf("inputs_embeds", (Bv * S, d), f32, zero=False)
        if sharded:
            fr_all = self.buf("frames_gathered", (shard.T * n, d), f32, zero=False)
            shard.gather_rows(fr, n, fr_all)
            fr = fr_all
        # (host-side, on the CPU index maps: a layout built for another tokens-per-frame count — n = 32 vs the mean-pooled 1 — would send
        # the row gather past the frame-token matrix)
        n_src = int(layout.frame_src.max()) + 1 if layout.frame_src.numel() else 0
        if n_src > fr.shape[0] or int(layout.frame_dst.max() if layout.frame_dst.numel() else 0) >= Bv * S:
            raise ValueError(f"encoder layout does not fit this engine: it gathers frame-token row {n_src - 1} of {fr.shape[0]} "
                             f"(layout built with another n_per_frame / T than mean_pool={self.cfg.mean_pool}, num_query={self.cfg.num_query}?)")
        kmask = L["mask"]
        Ld = layout.labels.shape[1]
        dev_in = L if use_graph else None

        def t5_part1():   # interleave + encoder forward
            ops.row_copy(fr, L["frame_src"], inp, L["frame_dst"])
            ops.row_copy(self.emb, L["emb_src"], inp, L["emb_dst"])
            return self.t5_encoder_forward(inp, Bv, S, kmask, want_grad=backward)

        def t5_part2(enc):   # decoder forward + loss, decoder backward, encoder backward
            loss, _ = self.t5_decoder_forward(layout.decoder_input_ids, layout.decoder_mask, enc, Bv, S, kmask, layout.labels, want_grad=backward,
                                              dev_in=dev_in)
            self._mark("t5_decoder_forward + loss")
            if not backward:
                return loss, None
            denc = self.t5_decoder_backward(enc, Bv, S, Ld, kmask, layout.decoder_mask, dev_in=dev_in)
            self._mark("t5_decoder_backward")
            dinp = self.t5_encoder_backward(denc, Bv, S, kmask)
            self._mark("t5_encoder_backward")
            return loss, dinp

        rec = self._graph_record(L, fr, next_video is not None) if use_graph else None
        if rec is not None and rec["state"] == "ready" and rec["allocs"] != self.ws_allocations:
            # a workspace grew since the capture (a longer bucket was seen): its backing store moved, the graph holds dead addresses —
            # capture again (every buffer of THIS bucket exists: views of the larger stores)
            rec["state"] = "warm"
            MrBlipEngine.graph_replays -= 1
        if rec is not None and rec["state"] == "ready":       # replay: two graph launches instead of ~1000 kernel launches
            rec["g1"].replay()
            if next_video is not None:
                self.prefetch_vit(next_video)
            rec["g2"].replay()
            loss, dinp = rec["loss"], rec["dinp"]
        elif rec is not None and rec["state"] == "warm":       # second visit of the bucket: every workspace exists — capture, then run
            if next_video is not None and self.vit_lookahead_early:
                raise RuntimeError("captured step: MRB_VIT_EARLY=1 (look-ahead beside the encoder forward) is not supported")
            rec["g1"], enc = self._capture(t5_part1, reset_thin=True)
            rec["g1"].replay()
            if next_video is not None:
                self.prefetch_vit(next_video)
            rec["g2"], (loss, dinp) = self._capture(lambda: t5_part2(enc))
            rec["g2"].replay()
            rec.update(state="ready", loss=loss, dinp=dinp, allocs=self.ws_allocations)
        else:
            if rec is not None and rec["visits"] + 1 >= self.graph_capture_after:
                rec["state"] = "warm"          # the NEXT visit of this bucket captures
            if next_video is not None and self.vit_lookahead_early:
                self.prefetch_vit(next_video)
            enc = t5_part1()
            self._mark("t5_encoder_forward")
            if next_video is not None and not self.vit_lookahead_early:
                self.prefetch_vit(next_video)
            loss, dinp = t5_part2(enc)
        if not backward:
            if self.gemm_thin_enabled:
                self._post_thin_check()
            return loss
        if self.grad_ready_hook is not None:
            # every LoRA gradient (92 % of the trainable floats) is final here: a data-parallel caller starts their all-reduce now and it
            # runs beside the t5_proj / Q-Former backward below (mrblip/dist.py: GradExchange)
            self.grad_ready_hook("lora")
        if not train_frames:
            self._mark("t5_proj + Q-Former backward")
            if self.grad_ready_hook is not None:
                self.grad_ready_hook("all")
            if self.gemm_thin_enabled:
                self._post_thin_check()
            return loss
        # interleave backward: only frame-token rows carry gradient (embeddings are frozen)
        dfr = self.buf("dframes", ((shard.T if sharded else F_) * n, d), f32)
        ops.row_copy(dinp, L["frame_dst"], dfr, L["frame_src"])
        if sharded:
            dfr = shard.local_rows(dfr, n)
        if c.mean_pool:
            dfull = self.buf("dframes_full", (F_, c.num_query, d), f32, zero=False)
            ops.mean_pool_bwd(dfr, dfull)
            dfr = dfull.view(F_ * c.num_query, d)
        # t5_proj backward: dW = dfr^T x, db = colsum(dfr), dx = dfr W
        Mq = F_ * c.num_query
        dfb = self.buf("dframes_b", (Mq, pad64(d)), bf16)
        ops.cast_dropout(dfr, out_bf16=dfb)
        ops.colsum(dfr, self.dproj_b)
        mp = pad64(Mq)
        dft = self.buf("dframes_t", (d, mp), bf16)
        self.transpose2d(dfb, d, dft)
        Dq = c.qf_dim
        qbt = self.buf("qb_t", (Dq, mp), bf16)
        self.transpose2d(qb, Dq, qbt)
        ops.gemm(dft, qbt, self.dproj_w, residual=self.dproj_w, K=mp)
        dq_last = self.buf("dq_last", (Mq, Dq), f32, zero=False)
        ops.gemm(dfb, self.proj_wtb, dq_last, K=pad64(d))
        if next_video is not None:
            self.prefetch_vit_tail()
        dimg = self.qformer_backward(dq_last, img, F_)
        ops.layernorm_bwd(dimg, xv, self.lnv_w, self.ln_vision_eps, None, dgamma=self.dlnv_w, dbeta=self.dlnv_b)
        self._mark("t5_proj + Q-Former backward")
        if self.grad_ready_hook is not None:
            self.grad_ready_hook("all")
        if self.gemm_thin_enabled:
            self._post_thin_check()   # (at the END of the step: an event record between two kernels costs a dispatch bubble)
        return loss

    def _mark(self, name: str):
        """phase boundary for tools/phase_times.py (self.phase_events = [] enables it; None = off)"""
        ev = getattr(self, "phase_events", None)
        if ev is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append((name, e))

    def _layout_dev(self, layout: EncoderLayout, static: bool = False):
        dev = self.dev
        if static:
            return self._layout_dev_static(layout)
        cached = getattr(layout, "_dev_cache", None)  # a layout object is immutable: its device index maps are uploaded once
        if cached is not None and cached[0] is self:
            return cached[1]
        d = dict(frame_src=self.h2d(layout.frame_src), frame_dst=self.h2d(layout.frame_dst), emb_src=self.h2d(layout.emb_src),
                 emb_dst=self.h2d(layout.emb_dst), mask=self.pad_mask(layout.attention_mask))
        try:
            layout._dev_cache = (self, d)
        except AttributeError:
            pass
        return d

    # ---- captured step (round 5; VERDICT r4 missing 5).  The T5 part of a step — interleave, encoder forward | decoder forward + loss, decoder
    # backward, encoder backward — is ~1000 of the step's ~1650 launches and, for short clips (Charades-STA: 20 frames, S = 72), a chain of
    # few-row kernels the host enqueues barely faster than the GPU runs them (24 ms of host time for a 28 ms step; 4 ranks sharing cores:
    # host-bound).  Both halves are captured as hipGraphs per shape bucket (the look-ahead ViT's hand-over sits between them and stays
    # eager: its completion is consumed by the NEXT step, which a capture cannot contain) and replayed with two launches.  What makes that
    # legal here: workspaces are capacity-based views with fixed addresses (engine.buf), seeds / AdamW hyper-parameters / loss live in device
    # memory, the side streams fork from and join back into the captured stream through events, the thin role's flag words are cleared by
    # a captured fill at the head of the first graph (its epochs are launch arguments), and the step's integer inputs live in per-bucket
    # static buffers (below).  MRB_GRAPH = 0 off / 1 on / auto (default): on for encoders of at most ``graph_auto_rows`` rows.
    graph_mode = os.environ.get("MRB_GRAPH", "auto")
    graph_auto_rows = 512
    _graphs: Dict[tuple, dict] = None
    graph_replays = 0

    def _graph_wanted(self, B: int, S: int, backward: bool, sharded: bool) -> bool:
        if self.graph_mode == "0" or not backward or sharded or getattr(self, "phase_events", None) is not None:
            return False
        return self.graph_mode == "1" or (self.graph_mode == "auto" and B * S <= self.graph_auto_rows)

    # the bucket caches are BOUNDED.  A bucket (shape key) is captured on its ``graph_capture_after``-th visit (earlier visits run
    # eager: with B > 1 many buckets are seen once), at most ``graph_max_buckets`` captured buckets / static sets are kept, least recently
    # used first out — an evicted bucket's CUDAGraphs (about 1000 nodes and a private pool each) and its pinned staging sets are released.
    graph_max_buckets = int(os.environ.get("MRB_GRAPH_MAX_BUCKETS", "16"))
    graph_capture_after = max(2, int(os.environ.get("MRB_GRAPH_AFTER", "2")))     # (>= 2: the first visit creates the bucket's workspaces)
    graph_evictions = 0

    def _graph_record(self, L: dict, fr: torch.Tensor, lookahead: bool) -> dict:
        from collections import OrderedDict
        if self._graphs is None:
            self._graphs = OrderedDict()
        key = L["key"] + (bool(self.training), fr.data_ptr(), lookahead, ops.dec_proj_config(-1))
        rec = self._graphs.get(key)
        if rec is None:
            rec = self._graphs[key] = dict(state="new", visits=0)
            while len(self._graphs) > self.graph_max_buckets:
                _, old = self._graphs.popitem(last=False)
                old.clear()                      # drops the CUDAGraph objects (g1 / g2) and the tensors they return
                MrBlipEngine.graph_evictions += 1
        else:
            self._graphs.move_to_end(key)
            if rec["state"] == "ready":
                MrBlipEngine.graph_replays += 1
        rec["visits"] = rec.get("visits", 0) + 1
        return rec

    def _capture(self, fn, reset_thin: bool = False):
        """Capture fn's launches as ONE-stream graph.  The gradient side stream is switched off inside: a captured fork / join DAG replays
        far slower than the eager streams on this runtime (ROCm 7.2: Charades-STA 28.6 ms eager, 39.4 ms as a multi-stream graph, 29.4 ms
        as a single-stream graph — profiles/r05_graph_ab.txt); what the side stream hid (0.8 ms at Charades-STA) is the price of a host
        that enqueues a step in 6 ms instead of 25."""
        g = torch.cuda.CUDAGraph()
        side = self.grad_side_stream_enabled
        self.grad_side_stream_enabled = False
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                if reset_thin and self.gemm_thin_enabled:
                    ops.thin_flags_reset(self.dev)
                out = fn()
        finally:
            self.grad_side_stream_enabled = side
        return g, out

    # The integer inputs of a step in STATIC device buffers, one set per shape bucket.  A hipGraph bakes every
    # kernel argument in: pointers, shapes and scalars.  The step's data-dependent inputs are index maps (interleave), masks, decoder ids
    # and labels — small integer tensors whose SHAPES are fixed by (B, S, L_dec, rows per source) and whose CONTENTS change with every
    # query.  They live in per-bucket device tensors that each step refills from pinned staging memory (asynchronous copies ahead of the
    # graph launches), so a graph captured for a bucket serves every later step of that bucket, whatever the text says.  The one scalar
    # that depends on contents, the number of valid label tokens (CE's 1 / count), is part of the bucket key.
    _static_sets: Dict[tuple, dict] = None

    def _layout_dev_static(self, layout: EncoderLayout) -> dict:
        from collections import OrderedDict
        if self._static_sets is None:
            self._static_sets = OrderedDict()
        B, Ld = layout.labels.shape
        has_k = not bool((layout.attention_mask != 0).all())
        has_d = not bool((layout.decoder_mask != 0).all())
        n_valid = int((layout.labels != -100).sum())
        key = (B, layout.S, Ld, layout.frame_src.numel(), layout.emb_src.numel(), has_k, has_d)
        st = self._static_sets.get(key)
        if st is not None:
            self._static_sets.move_to_end(key)
        i32 = torch.int32
        if st is None:
            def dv(n):
                return torch.zeros(n, dtype=i32, device=self.dev)

            def pin(n):
                return torch.zeros(n, dtype=i32).pin_memory()
            st = dict(key=key, n_valid=dv(1),
                      frame_src=dv(layout.frame_src.numel()), frame_dst=dv(layout.frame_dst.numel()), emb_src=dv(layout.emb_src.numel()),
                      emb_dst=dv(layout.emb_dst.numel()), dec_ids32=dv(B * Ld), labels32=dv(B * Ld),
                      dec_rows=torch.arange(B * Ld, dtype=i32, device=self.dev),
                      mask=torch.zeros(B, ops.rup32(layout.S), dtype=i32, device=self.dev) if has_k else None,
                      dec_mask=torch.zeros(B, ops.rup32(Ld), dtype=i32, device=self.dev) if has_d else None)
            # four rotating pinned staging sets, each with the event of its last copies: the host runs up to a step ahead of the GPU and
            # must not overwrite staging memory an enqueued copy has not read yet
            names = [k for k, v in st.items() if torch.is_tensor(v) and k != "dec_rows"]
            st["_pin"] = [{k: pin(st[k].numel()) for k in names} for _ in range(4)]
            st["_ev"] = [None] * 4
            st["_slot"] = 0
            st["_last"] = None
            self._static_sets[key] = st
            while len(self._static_sets) > 2 * self.graph_max_buckets:      # (a set may outlive its graphs' eviction by a while: twice the cap)
                k_old, old = self._static_sets.popitem(last=False)
                if self._graphs:
                    for gk in [gk for gk in self._graphs if gk[:len(k_old)] == k_old]:
                        self._graphs.pop(gk).clear()
                        MrBlipEngine.graph_evictions += 1
                old.clear()
        if st["_last"] is not layout:      # (the same layout object again: the buffers already hold it)
            src = dict(frame_src=layout.frame_src, frame_dst=layout.frame_dst, emb_src=layout.emb_src, emb_dst=layout.emb_dst,
                       dec_ids32=layout.decoder_input_ids, labels32=layout.labels, n_valid=torch.tensor([n_valid]))
            if has_k:
                m = torch.zeros(B, ops.rup32(layout.S), dtype=i32)
                m[:, :layout.S] = layout.attention_mask
                src["mask"] = m
            if has_d:
                m = torch.zeros(B, ops.rup32(Ld), dtype=i32)
                m[:, :Ld] = layout.decoder_mask
                src["dec_mask"] = m
            slot = st["_slot"]
            st["_slot"] = (slot + 1) % 4
            if st["_ev"][slot] is not None:
                st["_ev"][slot].synchronize()
            for k, t in src.items():
                pn = st["_pin"][slot][k]
                pn.copy_(t.reshape(-1).to(i32))
                st[k].view(-1).copy_(pn, non_blocking=True)
            st["_ev"][slot] = torch.cuda.Event()
            st["_ev"][slot].record()
            st["_last"] = layout
        return st

    def pad_mask(self, m: torch.Tensor) -> Optional[torch.Tensor]:
        """[B,S] 0/1 mask -> int32 [B, rup32(S)] on the device (the attention kernels read the key mask 16 B at a time)."""
        if bool((m != 0).all()):
            return None  # nothing is masked: the attention kernels run their mask-free specialisation
        B, S = m.shape
        out = torch.zeros(B, ops.rup32(S), dtype=torch.int32, device=self.dev)
        out[:, :S] = self.h2d(m, torch.int32)
        return out

    def dropout_site_map(self) -> Dict[str, tuple]:
        """logical dropout site (named after the reference's nn.Dropout modules) -> (call-site id, p, kind); used by the parity
        tests to rebuild the exact masks of a training step on the CPU oracle."""
        c = self.cfg
        q = self.qf_site_salt
        m = {"qf.emb": (self.qf_emb_site + q, c.qf_dropout, "2d")}
        for i, L in enumerate(self.qf["layers"]):
            m[f"qf.{i}.self.attn"] = (L["self"]["sites"][0] + q, c.qf_dropout, "attn")
            m[f"qf.{i}.self.out"] = (L["self"]["sites"][1] + q, c.qf_dropout, "2d")
            if L["cross"] is not None:
                m[f"qf.{i}.cross.attn"] = (L["cross"]["sites"][0] + q, c.qf_dropout, "attn")
                m[f"qf.{i}.cross.out"] = (L["cross"]["sites"][1] + q, c.qf_dropout, "2d")
            m[f"qf.{i}.ffn.out"] = (L["site"] + q, c.qf_dropout, "2d")
        p = c.t5_dropout
        for k, j in (("t5.enc.emb", 0), ("t5.enc.final", 1), ("t5.dec.emb", 2), ("t5.dec.final", 3)):
            m[k] = (self.t5["sites"][j], p, "2d")
        for i, L in enumerate(self.t5["enc"]):
            for j, (k, kind) in enumerate(((".attn", "attn"), (".attn_out", "2d"), (".ffn_inner", "2d"), (".ffn_out", "2d"))):
                m[f"t5.enc.{i}{k}"] = (L["sites"][j], p, kind)
        for i, L in enumerate(self.t5["dec"]):
            for j, (k, kind) in enumerate(((".self.attn", "attn"), (".self_out", "2d"), (".cross.attn", "attn"), (".cross_out", "2d"),
                                           (".ffn_inner", "2d"), (".ffn_out", "2d"))):
                m[f"t5.dec.{i}{k}"] = (L["sites"][j], p, kind)
        for g in self.groups:
            for a in g.adapters:
                per_adapter = c.lora_mask_per_adapter and len(g.adapters) > 1
                m["lora:" + a.name] = (a.site if per_adapter else g.site, c.lora_dropout, "2d")
        return m

    # ------------------------------------------------------------------------------------------ optimizer
    @torch.no_grad()
    def zero_grad(self):
        self.grad.zero_()

    # ---- the in-GEMM thin role must fail LOUDLY (VERDICT r4 weak 3 / ADVICE r4).  A consumer tile of csrc/gemm.hip whose bounded wait
    # for its producer workgroups runs out continues with whatever the K-extension operand holds and sets the device's error word
    # (ops.thin_error_word).  Three things follow from that word: (i) the fused AdamW takes it as its guard — a step whose activations may be
    # wrong is never applied, decided on the device; (ii) its value travels to pinned host memory behind every step and is read ONE STEP
    # LATE (no stream drain: the same trick as the deferred loss-scale check, blip2_mr.py _check_fused_scale) — a set word raises; (iii) the
    # runner's blocking check points (end of epoch, before every checkpoint) call check_thin_role(block=True).
    _thin_host = None
    _thin_event = None

    def thin_guard(self) -> torch.Tensor:
        return ops.thin_error_word(self.dev)

    # a timeout is loud AND survivable.  thin_fallback (MRB_THIN_FALLBACK, default on): the first set error word switches THIS engine
    # to the thin product as a launch of its own (gemm_thin_enabled = False: same bits, no in-launch wait, nothing to time out), clears the
    # word, drops the captured graphs (they hold thin-role launches) and REWINDS the optimizer clock by the steps the guarded AdamW skipped
    # on the device in the meantime (opt_step here, FlatAdamW.t through consume_thin_skipped) — bias correction then counts applied steps
    # only — and training continues with a warning.  thin_fallback = False: raise, as in round 5.
    thin_fallback = os.environ.get("MRB_THIN_FALLBACK", "1") == "1"
    thin_fallbacks = 0            # how often this engine fell back (0 in every run that owns its GPU)
    opt_clock = 0                 # optimizer steps ISSUED so far (engine.optimizer_step and the runner's FlatAdamW both tick it)
    _thin_post_clock = 0
    _thin_skipped = 0

    def note_optimizer_step(self):
        self.opt_clock += 1

    def consume_thin_skipped(self) -> int:
        """optimizer steps that were issued but dropped on the device by the guard since the last call (an external optimizer rewinds its
        own step count by this much: FlatAdamW)"""
        n, self._thin_skipped = self._thin_skipped, 0
        return n

    def _post_thin_check(self):
        """enqueue the error word's copy to the host behind everything this step launched"""
        if self._thin_host is None:
            self._thin_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._thin_host.copy_(self.thin_guard(), non_blocking=True)
        self._thin_event = torch.cuda.Event()
        self._thin_event.record()
        self._thin_post_clock = self.opt_clock

    def check_thin_role(self, block: bool = False):
        ev = self._thin_event
        if ev is None:
            if block and self.gemm_thin_enabled:
                self._post_thin_check()
                ev = self._thin_event
            else:
                return
        if block:
            ev.synchronize()
        elif not ev.query():
            return
        self._thin_event = None
        if int(self._thin_host[0]) != 0:
            w = int(self._thin_host[0]) & 0xffffffff
            if self.thin_fallback and self.gemm_thin_enabled:
                import logging
                # every AdamW issued since the check that carried this verdict was posted ran (or will run) with the word set: dropped
                torch.cuda.synchronize(self.dev)
                skipped = self.opt_clock - self._thin_post_clock
                self.gemm_thin_enabled = False
                self.thin_fallbacks += 1
                self._thin_skipped += skipped
                self.opt_step = max(0, self.opt_step - skipped)
                ops.gemm_thin_clear()
                self._thin_host.zero_()
                if self._graphs:
                    for rec in self._graphs.values():
                        rec.clear()
                    self._graphs.clear()
                logging.warning("mrblip: [error word %#010x: row block %d, workgroup %d] a tile GEMM's bounded wait for its in-launch thin-role "
                                "workgroups ran out (a shared GPU?).  %d optimizer step(s) were dropped on the device; this engine now runs the LoRA "
                                "'down' products as launches of their own (same results) and continues.", w, (w >> 16) & 0x7fff, w & 0xffff, skipped)
                return
            raise ops.MrblipError(
                f"[error word {w:#010x}: row block {(w >> 16) & 0x7fff}, workgroup {w & 0xffff}] "
                "a tile GEMM's bounded wait for its in-launch thin-role workgroups (the LoRA 'down' product, csrc/gemm.hip) ran out: the "
                "step's encoder activations and LoRA gradients may be wrong.  The guarded AdamW has skipped every optimizer step since; "
                "set MRB_GEMM_THIN=0 (the thin product as a launch of its own) to run without the role, and report the configuration")

    _grad_guard = None            # mrblip.grad_guard.GradGuard of optimizer_step(grad_guard=True), built on first use

    def grad_guard(self, max_grad_norm=None):
        """the engine's own guard block (device state + deferred host view); max_grad_norm may change from call to call"""
        from .grad_guard import GradGuard, check_max_grad_norm
        if self._grad_guard is None:
            self._grad_guard = GradGuard(self.dev, self.grad.numel())
        self._grad_guard.max_grad_norm = check_max_grad_norm(max_grad_norm)
        return self._grad_guard

    @torch.no_grad()
    def optimizer_step(self, lr: float, weight_decay: float = 0.05, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                       grad_scale: float = 1.0, grad_guard: bool = False, max_grad_norm=None):
        """AdamW(beta=(0.9,0.999), wd on >=2-D non-bias/ln params) as in runner_base.py:102-132.  Guarded by the thin role's error word: see
        check_thin_role.  grad_guard / max_grad_norm (off by default; max_grad_norm implies the guard): the gradient guard of DESIGN.md §15
        — a step whose gradient holds an inf / nan is skipped on the device, the gradient is clipped to max_grad_norm, and the device
        counter of APPLIED steps is the optimizer clock (opt_step is then not used); self.grad_guard().stats() / .read() report."""
        if grad_guard or max_grad_norm is not None:
            guard = self.grad_guard(max_grad_norm)
            guard.poll()
            self.note_optimizer_step()
            nd = self.n_decay
            guard.prepare(self.grad, lr, grad_scale, (beta1, beta2), self.hyper, guard_in=self.thin_guard() if self.gemm_thin_enabled else None)
            skip = guard.skip_word()
            ops.adamw(self.flat[:nd], self.grad[:nd], self.adam_m[:nd], self.adam_v[:nd], self.hyper, beta1, beta2, eps, weight_decay, guard=skip)
            ops.adamw(self.flat[nd:], self.grad[nd:], self.adam_m[nd:], self.adam_v[nd:], self.hyper, beta1, beta2, eps, 0.0, guard=skip)
            self.refresh_trainable()
            return
        self.opt_step += 1
        self.note_optimizer_step()
        t = self.opt_step
        self.hyper.copy_(torch.tensor([lr, 1.0 / (1 - beta1 ** t), 1.0 / math.sqrt(1 - beta2 ** t), grad_scale], dtype=f32).pin_memory(), non_blocking=True)
        nd = self.n_decay
        guard = self.thin_guard() if self.gemm_thin_enabled else None
        ops.adamw(self.flat[:nd], self.grad[:nd], self.adam_m[:nd], self.adam_v[:nd], self.hyper, beta1, beta2, eps, weight_decay, guard=guard)
        ops.adamw(self.flat[nd:], self.grad[nd:], self.adam_m[nd:], self.adam_v[nd:], self.hyper, beta1, beta2, eps, 0.0, guard=guard)
        self.refresh_trainable()
