"""Round 4: the launch-saving forms of the train step against the forms they replace, on a mid-size engine whose heads are 64 wide like the
real model's (the tiny fixtures have d_kv = 16 and never reach them): head-transposed copies from the producing GEMMs' epilogues (T5
encoder, Q-Former), the stacked cross-attention K / V projection of all decoder layers, the cross-block key split of the decoder's cross
attention.  Same seeds, dropout ON: loss and the whole flat gradient must agree (the arithmetic is the same; only summation orders of the
attention merge differ)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from util import check, relerr  # noqa: E402


def _step(flags, B=1, steps=2, dec_layers=3):
    import bench
    from mrblip import prompt as P
    from mrblip.engine import EngineConfig, MrBlipEngine, RandomSource
    from mrblip.tokenizer import FixtureTokenizer
    dev = torch.device("cuda:0")
    cfg = EngineConfig(vit_dim=320, vit_depth=2, vit_heads=5, vit_mlp=512, qf_dim=256, qf_heads=4, qf_inter=512, qf_layers=4, num_query=32,
                       d_model=256, d_kv=64, t5_heads=4, d_ff=512, t5_layers=3, t5_dec_layers=dec_layers)
    eng = MrBlipEngine(cfg, RandomSource(dev, seed=77), dev, lora_init=bench.lora_init_nonzero, seed=11)
    flags = dict(dict(enc_qkv_w4=0, enc_bwd_w4=False), **flags)     # the round-4 paths under test live in the generic tile; the 4-wave forms have their own tests below
    for k, v in flags.items():
        setattr(eng, k, v)
    if flags.get("xs_off"):
        eng.xs_ws = None
    eng.training = True
    tok = FixtureTokenizer()
    repl = P.annoying_replacement_dict(P.find_annoying_numbers(tok, 200)[0])
    T = 40                                        # 40 frames x 32 queries + prompt: S > 1024 keys (the cross-block split applies), ragged
    samples = bench.synthetic_samples(B, T, 150.0, dev, 5)
    lay = P.build_layout(tok, samples, repl, cfg.num_query, T=T)
    losses = []
    for _ in range(steps):                        # second step: the look-ahead-free path reuses every workspace
        eng.zero_grad()
        losses.append(eng.forward_backward(samples["video"], lay, backward=True).item())
    torch.cuda.synchronize()
    return losses, eng.grad.detach().clone(), eng, lay


def test_gemm_epilogue_transposes_and_stacked_cross_kv_equal_the_launches_they_replace():
    from mrblip import ops
    base_l, base_g, eng0, lay = _step(dict(gemm_tout_enabled=False, cross_kv_batched=False, xs_off=True))
    assert lay.S > 1024 and eng0.cfg.d_kv == 64
    n0 = ops.launch_count
    _step(dict(gemm_tout_enabled=False, cross_kv_batched=False, xs_off=True), steps=1)
    launches_old = ops.launch_count - n0
    for name, flags in (("gemm epilogue transposes", dict(cross_kv_batched=False, xs_off=True)),
                        ("+ stacked cross K/V", dict(xs_off=True)),
                        ("+ cross-block key split", dict())):
        n0 = ops.launch_count
        l, g, eng, _ = _step(flags)
        tag = "round-4 paths (d_kv 64, S=%d): %s: " % (lay.S, name)
        # transposes from the epilogue: the same bits.  Stacked cross K / V: its backward adds the layers' contributions to the encoder-output
        # gradient in another fp32 order (chunks of layers in one K loop) — 1e-7 there, which flips bf16 roundings of the operands the encoder
        # backward builds from it (measured 3.4e-4 on the flat gradient); the key split re-orders the softmax merge as well.
        check(tag + "loss (rel)", max(abs(a - b) / abs(b) for a, b in zip(l, base_l)), 2e-7 if "split" not in name else 1.8e-4)   # (measured 0 / 0 / 3.5e-5)
        check(tag + "flat gradient", relerr(g, base_g), 2e-7 if "epilogue" in name else 1e-3 if "split" not in name else 1.2e-2)   # (measured 0 / 3.6e-4 / 5.2e-3)
        assert eng.grad[: eng.n_lora].abs().sum() > 0
    n0 = ops.launch_count
    _step(dict(), steps=1)
    launches_new = ops.launch_count - n0
    assert launches_new < launches_old - 3 * 10, (launches_old, launches_new)     # 3 + 3 layers: transposes and per-layer K / V launches are gone


def test_batched_lora_weight_gradients_are_bit_identical_to_one_launch_per_group():
    """lora_grads_batch (MRB_LORA_GRADS_BATCH) is documented as an A/B switch with the same bits: the batched launch runs the two-tile
    body (CT = 2) where the per-group launches run the one-tile body, so loss and the whole flat gradient are compared bitwise"""
    l0, g0, eng0, _ = _step(dict(lora_grads_batch=False))
    l1, g1, eng1, _ = _step(dict(lora_grads_batch=True))
    assert not eng0.lora_grads_batch and eng1.lora_grads_batch and eng1.grad_side_stream_enabled
    assert l1 == l0, (l1, l0)
    assert torch.equal(g1, g0), relerr(g1, g0)


@pytest.mark.parametrize("fwd_chunks,bwd_chunks", [((5, 7), (12,)), ((12,), (4, 8))])
def test_stacked_cross_kv_in_chunks_of_four_and_more_layers(fwd_chunks, bwd_chunks):
    """12 decoder layers, the stacked cross K / V path in chunks of 4..12 layers (production runs 2 / 6 / 8 / 8 forward and 10 / 8 / 4 / 2
    backward with 24 layers; the 3-layer engine above never gets past 3): every cross-attention K / V adapter's weight gradients against the
    per-layer path, tensor by tensor"""
    l0, g0, eng0, _ = _step(dict(cross_kv_batched=False), dec_layers=12)
    l1, g1, eng1, _ = _step(dict(ckv_fwd_chunks=fwd_chunks, ckv_bwd_chunks=bwd_chunks), dec_layers=12)
    assert eng1.ckv_all is not None and eng1.ckv_all["L"] == 12
    tag = "round-4 paths, 12 decoder layers, cross K/V chunks %s / %s: " % (",".join(map(str, fwd_chunks)), ",".join(map(str, bwd_chunks)))
    check(tag + "loss (rel)", max(abs(a - b) / abs(b) for a, b in zip(l1, l0)), 1.5e-7)    # (measured 0: the forward is the same arithmetic)
    eb = ea = 0.0
    for L0, L1 in zip(eng0.t5["dec"], eng1.t5["dec"]):
        for a0, a1 in zip(L0["ckv"].adapters, L1["ckv"].adapters):
            assert a1.dA.abs().sum() > 0 and a1.dBt.abs().sum() > 0
            eb, ea = max(eb, relerr(a1.dBt, a0.dBt)), max(ea, relerr(a1.dA, a0.dA))
    check(tag + "cross K/V dB^T, worst adapter", eb, 1.5e-7)     # (measured 0)
    check(tag + "cross K/V dA, worst adapter", ea, 1.5e-7)       # (measured 0)
    check(tag + "flat gradient", relerr(g1, g0), 6.5e-4)   # (measured 3.1e-4: the encoder-output gradient is summed in another fp32 order, see above)


def test_several_clips_whose_length_is_not_a_multiple_of_32_fall_back():
    """B = 2 clips of a ragged length: the tile GEMM's transposed copies need one clip or clips of 32-row multiples — the engine must take
    the transpose launches (and the per-layer cross K / V) and agree with the forced-off run exactly"""
    base_l, base_g, _, lay = _step(dict(gemm_tout_enabled=False, cross_kv_batched=False), B=2, steps=1)
    l, g, eng, _ = _step(dict(), B=2, steps=1)
    assert lay.S % 32 != 0
    assert l == base_l          # same forward kernels -> the same loss bits; the gradient has fp32 atomics (LayerNorm weight gradients): 1e-6
    check("round-4 paths, 2 ragged clips: flat gradient of the fall-back vs forced-off run", relerr(g, base_g), 2e-7)   # (measured 0)


def test_role_workgroups_of_the_encoder_gemms_change_no_bit():
    """The LoRA "down" products computed by the consuming GEMMs' thin-role workgroups and the weight prefetch that rides in the encoder's /
    Q-Former's GEMMs (S > 1024 rows here, so both are active by default) against launches of their own and no prefetch: the loss of both
    steps and the whole flat gradient must be the SAME BITS (the thin body is shared, the prefetch only reads), and no tile may have run
    out of its bounded wait for the thin role."""
    from mrblip import ops
    base_l, base_g, eng0, lay = _step(dict(gemm_thin_enabled=False, enc_prefetch=(0,), qf_prefetch=False))
    assert lay.S >= eng0.gemm_thin_min_rows and lay.S >= eng0.enc_prefetch_min_rows
    n0 = ops.launch_count
    _step(dict(gemm_thin_enabled=False, enc_prefetch=(0,), qf_prefetch=False), steps=1)
    launches_old = ops.launch_count - n0
    n0 = ops.launch_count
    l, g, eng, _ = _step(dict(), steps=2)
    assert eng.gemm_thin_enabled and eng.enc_prefetch[0] > 0 and eng.qf_prefetch
    assert l == base_l, (l, base_l)
    assert torch.equal(g, base_g)
    assert ops.gemm_thin_timeouts() == 0
    n0 = ops.launch_count
    _step(dict(), steps=1)
    assert ops.launch_count - n0 <= launches_old - 2 * 3, (launches_old, ops.launch_count - n0)   # o and wo of 3 encoder layers lost their thin launch


def test_a_thin_role_timeout_is_loud_and_skips_the_optimizer_step():
    """VERDICT r4 weak 3 / ADVICE r4: a consumer tile whose bounded wait for the in-launch thin role runs out used to continue on stale
    operands with an error word nobody in the training path read.  Forced here with the test hook (the role workgroups exit without
    publishing): the device error word must be set, the guarded AdamW must leave parameters AND moments untouched, the NEXT step's entry
    check (and the runner's blocking check) must raise — and after clearing the word training continues."""
    from mrblip import ops
    _, _, eng, lay = _step(dict(thin_fallback=False), steps=1)        # a healthy step first (workspaces, flag buffer, error word exist)
    assert ops.gemm_thin_timeouts() == 0
    eng.optimizer_step(1e-3)
    torch.cuda.synchronize()
    flat0, m0, v0 = eng.flat.clone(), eng.adam_m.clone(), eng.adam_v.clone()
    assert m0.abs().sum() > 0
    import bench
    samples = bench.synthetic_samples(1, 40, 150.0, torch.device("cuda:0"), 5)
    eng.zero_grad()
    with ops.gemm_debug_stall_thin():
        eng.forward_backward(samples["video"], lay, backward=True)
    eng.optimizer_step(1e-3)                       # guarded: must be a no-op
    torch.cuda.synchronize()
    assert ops.gemm_thin_timeouts() == 1
    assert torch.equal(eng.flat, flat0) and torch.equal(eng.adam_m, m0) and torch.equal(eng.adam_v, v0)
    with pytest.raises(ops.MrblipError, match="thin-role"):
        eng.forward_backward(samples["video"], lay, backward=True)      # the verdict of the stalled step has arrived by now
    with pytest.raises(ops.MrblipError, match="thin-role"):
        eng.check_thin_role(block=True)            # the runner's blocking form (end of epoch / before a checkpoint) sees the sticky word too
    ops.gemm_thin_clear()
    eng.zero_grad()
    l = eng.forward_backward(samples["video"], lay, backward=True).item()
    eng.optimizer_step(1e-3)
    torch.cuda.synchronize()
    eng.check_thin_role(block=True)
    assert l == l and not torch.equal(eng.flat, flat0) and ops.gemm_thin_timeouts() == 0


def test_a_thin_role_timeout_falls_back_to_thin_launches_and_rewinds_the_optimizer_clock():
    """the default reaction to a timeout is not to abort.  The step in which the wait ran out and every optimizer step issued until
    the verdict is read are dropped ON THE DEVICE (guarded AdamW); the next step's entry check then switches this engine to the thin products
    as launches of their own, clears the word, rewinds the optimizer clock by the dropped steps (bias correction counts applied steps) and
    training goes on — with the bits of a run that never had the role."""
    from mrblip import ops
    _, _, eng, lay = _step(dict(), steps=1)
    assert eng.thin_fallback and eng.gemm_thin_enabled and ops.gemm_thin_timeouts() == 0
    eng.optimizer_step(1e-3)
    torch.cuda.synchronize()
    t0, flat0 = eng.opt_step, eng.flat.clone()
    import bench
    samples = bench.synthetic_samples(1, 40, 150.0, torch.device("cuda:0"), 5)
    eng.zero_grad()
    with ops.gemm_debug_stall_thin():
        eng.forward_backward(samples["video"], lay, backward=True)
    eng.optimizer_step(1e-3)                       # issued, dropped on the device
    torch.cuda.synchronize()
    assert ops.gemm_thin_timeouts() == 1 and torch.equal(eng.flat, flat0) and eng.opt_step == t0 + 1
    eng.zero_grad()
    seed_before = eng.seed.clone()
    l = eng.forward_backward(samples["video"], lay, backward=True).item()      # entry check: falls back, this step already runs without the role
    assert not eng.gemm_thin_enabled and eng.thin_fallbacks == 1 and ops.gemm_thin_timeouts() == 0
    assert eng.opt_step == t0 and eng.consume_thin_skipped() == 1
    g_fb = eng.grad.clone()
    eng.optimizer_step(1e-3)
    torch.cuda.synchronize()
    eng.check_thin_role(block=True)
    assert l == l and not torch.equal(eng.flat, flat0) and eng.opt_step == t0 + 1
    # the same step on an engine that never had the role: the same gradient bits
    _, _, ref, _ = _step(dict(gemm_thin_enabled=False), steps=1)
    ref.flat.copy_(flat0)
    ref.refresh_trainable()
    ref.seed.copy_(seed_before)                     # (forward_backward bumps the seed first: replay the fallen-back step's dropout stream)
    ref.zero_grad()
    l_ref = ref.forward_backward(samples["video"], lay, backward=True).item()
    assert l_ref == l and torch.equal(ref.grad, g_fb)


def test_encoder_gated_wi_through_the_four_wave_kernel_equals_the_generic_tile_path():
    """Round 6 (opt-in, MRB_ENC_WI_W4=1: measured 0.9 ms per step SLOWER than the generic gated tile, profiles/r06_ab_switches.txt): the gated wi
    projection as [xn2 | u] x [W | B]^T on the 4-wave kernel's gated form.  Same arithmetic as the generic tile's gated epilogue; loss and
    flat gradient against that path, dropout on, and the B columns of [W | B] must follow the optimizer."""
    base_l, base_g, eng0, lay = _step(dict(enc_wi_w4=0))
    assert lay.S >= 1024
    l, g, eng, _ = _step(dict(enc_wi_w4=1))
    assert eng.enc_wi_wc is not None and eng.enc_wi_wc.shape[2] == eng.cfg.d_model + 64
    tag = "encoder gated wi via the 4-wave kernel vs the generic tile path: "
    check(tag + "loss (rel)", max(abs(a - b) / abs(b) for a, b in zip(l, base_l)), 2e-6)
    check(tag + "flat gradient", relerr(g, base_g), 2e-3)
    eng.optimizer_step(1e-2)
    torch.cuda.synchronize()
    g0 = eng.t5["enc"][0]["wi"]
    assert torch.equal(eng.enc_wi_wc[0, :, eng.cfg.d_model:], g0.wext) and torch.equal(eng.enc_wi_wc[0, :, :g0.K], g0.W[:, :g0.K])


def test_encoder_qkv_through_the_four_wave_kernel_equals_the_generic_tile_path():
    """Round 5: above 1024 rows the T5 encoder's qkv projection runs as ONE plain product [xn | u] x [W | B]^T over K + 64 on the
    hand-pipelined 4-wave kernel (no K extension, no thin role, no epilogue transposes there: a thin launch, a V^T transpose and the
    backward's Q^T / K^T transposes replace them).  Same arithmetic, other summation order: loss and flat gradient against the generic
    tile path (enc_qkv_w4 = 0), dropout on; and the concatenated weights must follow the optimizer (B changes every step)."""
    base_l, base_g, eng0, lay = _step(dict(enc_qkv_w4=0))
    assert lay.S >= 1024
    for cfg in (14, 13):
        l, g, eng, _ = _step(dict(enc_qkv_w4=cfg))
        assert eng.enc_qkv_wc is not None and eng.enc_qkv_wc.shape[2] == eng.cfg.d_model + 64
        tag = "encoder qkv via the 4-wave kernel (cfg %d) vs the generic tile path: " % cfg
        check(tag + "loss (rel)", max(abs(a - b) / abs(b) for a, b in zip(l, base_l)), 2e-7)     # (measured 0: the K tiles are accumulated in the same order)
        check(tag + "flat gradient", relerr(g, base_g), 2e-7)
        # the B columns of [W | B] are refreshed with the trainable tensors
        eng.optimizer_step(1e-2)
        torch.cuda.synchronize()
        g0 = eng.t5["enc"][0]["qkv"]
        assert torch.equal(eng.enc_qkv_wc[0, :, eng.cfg.d_model:], g0.wext) and torch.equal(eng.enc_qkv_wc[0, :, :g0.K], g0.W[:, :g0.K])
    # one clip, the three transposed copies from ONE launch of the forward (enc_qkv_t3; measured, not the default)
    l3, g3, eng, _ = _step(dict(enc_qkv_w4=14, enc_qkv_t3=True))
    assert eng.enc_t_saved[0] and eng.ws["e0_kt"].shape[1] == eng.cfg.t5_heads
    l, g, eng, _ = _step(dict(enc_qkv_w4=14))
    assert l3 == l and relerr(g3, g) < 1e-6                     # the same bits reach the same kernels (fp32 atomics in the LayerNorm weight gradients: 1e-7)
    # several clips: V^T by its own launch, Q^T / K^T by the backward's side stream
    b2_l, b2_g, _, _ = _step(dict(enc_qkv_w4=0), B=2, steps=1)
    l, g, eng, _ = _step(dict(enc_qkv_w4=14), B=2, steps=1)
    assert not eng.enc_t_saved[0]
    check("encoder qkv via the 4-wave kernel, 2 clips vs the generic tile path: loss (rel)", abs(l[0] - b2_l[0]) / abs(b2_l[0]), 2e-7)
    check("encoder qkv via the 4-wave kernel, 2 clips vs the generic tile path: flat gradient", relerr(g, b2_g), 2e-7)


def test_encoder_input_gradients_through_the_k_split_four_wave_kernel_equal_the_generic_tile_path():
    """Round 5: the encoder backward's wo / wi / qkv input gradients as PARTS of the 4-wave kernel (a K-split where the [M x d] output has
    too few tiles), added by the gated-GELU / RMSNorm backward that consumes them, the LoRA part under its lora_dropout mask.  Same
    forward (same loss bits); the gradient differs by summation order and by ONE bf16 rounding less on the wo path."""
    base_l, base_g, eng0, lay = _step(dict(enc_bwd_w4=False))
    l, g, eng, _ = _step(dict(enc_bwd_w4=True))
    assert eng._enc_bwd_w4_ok(lay.S) and "eb_dxn_p_wi" in eng.ws and "eb_dxn_p_wi" not in eng0.ws
    assert l == base_l
    check("encoder input gradients via K-split parts vs the generic tile path: flat gradient", relerr(g, base_g), 2.5e-3)   # (measured 5.1e-4: one bf16 rounding less on the wo path)
    l2, g2, _, _ = _step(dict(enc_bwd_w4=True))
    assert l2 == l and torch.equal(g2, g)          # parts are added in part order: reproducible


def test_one_side_stream_hand_over_per_encoder_layer_changes_no_bit():
    """enc_grads_at_wi: the weight-gradient launch of the encoder backward leaves with the K^T / Q^T job behind the wi product (wo, wi of the
    layer + o, qkv of the layer above) instead of at the end of the layer — the same jobs in other launches, the same bits."""
    base_l, base_g, _, lay = _step(dict(enc_bwd_w4=True, enc_qkv_w4=14, enc_grads_at_wi=False))
    l, g, eng, _ = _step(dict(enc_bwd_w4=True, enc_qkv_w4=14, enc_grads_at_wi=True))
    assert l == base_l and relerr(g, base_g) < 1e-6      # (fp32 atomics in the LayerNorm weight gradients of the Q-Former: 1e-7)
    assert torch.equal(g[: eng.n_lora], base_g[: eng.n_lora])
