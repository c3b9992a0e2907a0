"""The fused cached self-attention of generate's decode step (csrc/decode.hip, ops.decode_self_attention, Engine.t5_decode_step with
state["fused"], BLIP2_MR.generate_fused_decode / generate_graph_decode):

(a) the kernel against an fp64 evaluation of the same bf16 inputs, entry by entry, and bit-exact checks of everything it stores;
(b) the engine's fused step, teacher-forced, against the oracle (the project's tolerances of the unfused step);
(c) generate with the switch on, host search and device search, against the oracle's decode;
(d) the captured decoder step against the eager fused step, bit for bit, and the graph bookkeeping.

Output bound of (a), per entry: |out - ref| <= 2^-8 |ref| + 1e-4 max|v| — one bf16 ulp for the store plus ten times the fp32 exp and
accumulate error over at most 161 terms.  Scores have a standard deviation of about 2 and the LUT is N(0, 1), so a bias index off by one
moves a score by about 1."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from util import check, record, relerr  # noqa: E402

SENT = 7.0   # sentinel: exactly representable in bf16


# ------------------------------------------------------------------------------------------------ (a) kernel
def _inputs(R, H, D, Lmax, layers, pos, with_parents, seed):
    g = torch.Generator().manual_seed(seed)
    inner = H * D
    kv_src = torch.randn(2, layers, R, Lmax, inner, generator=g).bfloat16()
    if not with_parents:
        kv_src[:, :, :, pos:] = SENT          # in place: positions >= pos hold nothing yet
    qkv = torch.randn(R, 3 * inner + 8, generator=g).bfloat16()
    lut = torch.randn(H, 257, generator=g)
    return kv_src, qkv, lut


def _reference(kv_src, qkv, lut, parents, R, H, D, layer, pos, scale):
    """fp64 output [R, inner] and the expected planes of this layer [2, R, pos + 1, inner] (bf16 bits)"""
    inner = H * D
    p = torch.arange(R) if parents is None else torch.tensor([x if 0 <= x < R else r for r, x in enumerate(parents)])
    planes = torch.cat([kv_src[:, layer, :, :pos].index_select(1, p), qkv[:, inner:3 * inner].view(R, 2, 1, inner).transpose(0, 1)], 2)
    k = planes[0].double().view(R, pos + 1, H, D)
    v = planes[1].double().view(R, pos + 1, H, D)
    q = qkv[:, :inner].double().view(R, H, D)
    rel = (torch.arange(pos + 1) - pos).clamp(-128, 128) + 128
    s = scale * torch.einsum("rhd,rjhd->rhj", q, k) + lut.double()[:, rel][None]
    o = torch.einsum("rhj,rjhd->rhd", torch.softmax(s, -1), v)
    return o.reshape(R, inner), planes, float(v.abs().max())


def _launch(kv_src, qkv, lut, parents, R, H, D, layer, pos, scale, pos_dev=None):
    """-> (kv_src on the device after the launch, kv_dst, out [R, inner + 8], qkv on the device)"""
    from mrblip import ops
    src = kv_src.cuda()
    dst = torch.full_like(src, SENT) if parents is not None else src
    out = torch.full((R, H * D + 8), SENT, dtype=torch.bfloat16, device="cuda")
    qd = qkv.cuda()
    par = None if parents is None else torch.tensor(parents, dtype=torch.int32).cuda()
    pd = None if pos_dev is None else torch.tensor([pos_dev], dtype=torch.int32).cuda()
    ops.decode_self_attention(src, dst, qd, out, lut.cuda(), layer, H, pos=None if pd is not None else pos, pos_dev=pd, parents=par, scale=scale)
    torch.cuda.synchronize()
    if pd is not None:
        assert int(pd) == pos_dev      # the kernel never writes the position word
    return src, dst, out, qd


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


CASES = ([(3, 2, 16, 32, 2, 1, pos, None) for pos in (0, 1, 31)] +
         [(5, 4, 64, 64, 3, 0, pos, [0, 0, 2, 1, 1]) for pos in (0, 7, 63)] +
         [(2, 3, 24, 32, 1, 0, 5, None), (2, 1, 8, 160, 1, 0, 130, None)])


@pytest.mark.parametrize("R,H,D,Lmax,layers,layer,pos,parents", CASES)
def test_kernel_against_fp64_and_everything_it_stores(R, H, D, Lmax, layers, layer, pos, parents):
    inner = H * D
    scale = 2.0 / D ** 0.5
    kv_src, qkv, lut = _inputs(R, H, D, Lmax, layers, pos, parents is not None, 1000 * D + pos)
    ref, planes, vmax = _reference(kv_src, qkv, lut, parents, R, H, D, layer, pos, scale)
    src, dst, out, qd = _launch(kv_src, qkv, lut, parents, R, H, D, layer, pos, scale)
    got = out[:, :inner].double().cpu()
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-4 * vmax
    worst = float((err / bound).max())
    print(f"decode_self_attention {(R, H, D, Lmax, layers, layer)} pos {pos}: worst |out - ref| / bound = {worst:.3f}, max abs err {float(err.max()):.3e}")
    record(f"decode_self_attention R{R} H{H} D{D} pos{pos} (worst error / bound)", worst, 1.0)
    assert bool((err <= bound).all()), (worst, float(err.max()))
    # what the kernel stores, bit for bit
    want = torch.full_like(kv_src, SENT) if parents is not None else kv_src.clone()
    want[:, layer, :, :pos + 1] = planes
    assert torch.equal(_bits(dst), _bits(want))                                  # rows <= pos of this layer; above pos and other layers untouched
    assert torch.equal(_bits(out[:, inner:]), _bits(torch.full((R, 8), SENT).bfloat16()))   # columns beyond inner of the output rows
    assert torch.equal(_bits(qd), _bits(qkv))
    if parents is not None:
        assert torch.equal(_bits(src), _bits(kv_src))
    # the device position gives the same bits, and so does a second launch
    _, dst2, out2, _ = _launch(kv_src, qkv, lut, parents, R, H, D, layer, pos, scale, pos_dev=pos)
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(dst2), _bits(dst))
    _, dst3, out3, _ = _launch(kv_src, qkv, lut, parents, R, H, D, layer, pos, scale)
    assert torch.equal(_bits(out3), _bits(out)) and torch.equal(_bits(dst3), _bits(dst))


def test_an_out_of_range_parent_behaves_as_the_row_itself():
    R, H, D, Lmax, layers, layer, pos = 5, 4, 64, 64, 3, 2, 7
    scale = 2.0 / D ** 0.5
    kv_src, qkv, lut = _inputs(R, H, D, Lmax, layers, pos, True, 5)
    _, dst_a, out_a, _ = _launch(kv_src, qkv, lut, [0, -1, 2, 5, 1 << 30], R, H, D, layer, pos, scale)
    _, dst_b, out_b, _ = _launch(kv_src, qkv, lut, [0, 1, 2, 3, 4], R, H, D, layer, pos, scale)
    assert torch.equal(_bits(out_a), _bits(out_b)) and torch.equal(_bits(dst_a), _bits(dst_b))


@pytest.mark.parametrize("parents", [None, [1, 0, 0]])
def test_a_device_position_outside_the_cache_stores_nothing(parents):
    R, H, D, Lmax, layers, layer = 3, 2, 16, 32, 2, 1
    kv_src, qkv, lut = _inputs(R, H, D, Lmax, layers, 4, parents is not None, 6)
    for bad in (Lmax, -1):
        src, dst, out, qd = _launch(kv_src, qkv, lut, parents, R, H, D, layer, 0, 1.0, pos_dev=bad)
        assert torch.equal(_bits(qd), _bits(qkv))
        assert torch.equal(_bits(out), _bits(torch.full_like(out, SENT)))
        assert torch.equal(_bits(dst), _bits(torch.full_like(dst, SENT) if parents is not None else kv_src))
        assert torch.equal(_bits(src), _bits(kv_src))


def test_wrapper_and_custom_op_reject_what_the_kernel_cannot_take():
    from mrblip import ops, torch_ops  # noqa: F401
    kv = torch.zeros(2, 1, 2, 32, 16, dtype=torch.bfloat16, device="cuda")
    qkv = torch.randn(2, 48, generator=torch.Generator().manual_seed(3)).bfloat16().cuda()
    out = torch.zeros(2, 16, dtype=torch.bfloat16, device="cuda")
    lut = torch.zeros(1, 257, device="cuda")
    par = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(ops.MrblipError, match="mrblip_decode_self_attention"):
        ops.decode_self_attention(kv, kv, qkv, out, lut, 0, 1, pos=0, parents=par)            # parents need the other buffer
    with pytest.raises(ops.MrblipError, match="mrblip_decode_self_attention"):
        ops.decode_self_attention(kv, kv, qkv, out, lut, 0, 1, pos=32)
    with pytest.raises(ops.MrblipError, match="exactly one of pos"):
        ops.decode_self_attention(kv, kv, qkv, out, lut, 0, 1)
    with pytest.raises(ops.MrblipError, match="one int32 word"):
        ops.decode_self_attention(kv, kv, qkv, out, lut, 0, 1, pos_dev=par)
    with pytest.raises(ops.MrblipError, match="cuda"):
        ops.decode_self_attention(kv, kv, qkv, out, lut.cpu(), 0, 1, pos=0)
    torch.ops.mrblip.decode_self_attention(kv, kv, qkv, out, lut, 0, 1, 3)                    # the custom operator launches the same kernel
    want = out.clone()
    ops.decode_self_attention(kv, kv, qkv, out, lut, 0, 1, pos=3)
    assert torch.equal(_bits(out), _bits(want))


# ------------------------------------------------------------------------------------------------ (b) engine, teacher-forced
@functools.lru_cache(maxsize=None)
def _shared_model():
    from test_generate_gpu import _model_and_oracle
    return _model_and_oracle(False)


def test_fused_decode_step_logits_vs_oracle_teacher_forced():
    """test_decode_step_logits_vs_oracle_teacher_forced with state["fused"]: both decoders are fed the ORACLE's greedy prefix; the unfused
    step runs first on the same prefix, so that the fused-versus-unfused difference is a number of its own."""
    model, orc, tok, samples = _shared_model()
    eng = model.engine
    from mrblip import ops

    B = samples["video"].shape[0]
    layout = model._layout(dict(samples))
    video = model._frames_to_device(samples["video"])
    fr = eng.frames_forward(video)[0]
    L = eng._layout_dev(layout)
    S, d = layout.S, eng.cfg.d_model
    inp = eng.buf("inputs_embeds", (B * S, d), torch.float32, zero=False)
    ops.row_copy(fr, L["frame_src"], inp, L["frame_dst"])
    ops.row_copy(eng.emb, L["emb_src"], inp, L["emb_dst"])
    enc_h = eng.t5_encoder_forward(inp, B, S, L["mask"])
    cross = eng.t5_cross_kv(enc_h, B, S)
    with torch.no_grad():
        enc, atts = orc.encode_for_generate(tok, samples, model.annoying_numbers_replacement_dict)
        seqs = torch.zeros(B, 1, dtype=torch.long)
        refs = []
        for t in range(8):
            refs.append(orc.next_token_logprobs(seqs, enc, atts))
            seqs = torch.cat([seqs, refs[-1].argmax(-1, keepdim=True)], 1)
    state = eng.t5_decode_begin(B, 9)
    plain = [eng.t5_decode_step(state, seqs[:, t], None, cross, B, L["mask"]).float().cpu() for t in range(8)]
    state = eng.t5_decode_begin(B, 9)
    state["fused"] = True
    launches = ops.launch_count
    worst, worst_abs, worst_vs_plain = 0.0, 0.0, 0.0
    for t in range(8):
        logits = eng.t5_decode_step(state, seqs[:, t], torch.arange(B) if t else None, cross, B, L["mask"]).float().cpu()
        lp, lp_ref = torch.log_softmax(logits, -1), refs[t]
        worst = max(worst, relerr(lp, lp_ref))
        worst_abs = max(worst_abs, float((lp - lp_ref).abs().max()))
        worst_vs_plain = max(worst_vs_plain, float((logits - plain[t]).abs().max()))
        top2 = lp_ref.topk(2, -1).values
        sure = (top2[:, 0] - top2[:, 1]) > 5e-2
        assert torch.equal(lp.argmax(-1)[sure], lp_ref.argmax(-1)[sure]), (t, lp.argmax(-1), lp_ref.argmax(-1))
    assert state["t"] == 8
    check("generate.fused step log-probs vs emu-oracle (rel L2, worst of 8 steps)", worst, 2e-3)
    check("generate.fused step log-probs vs emu-oracle (max abs, worst of 8 steps)", worst_abs, 5e-2)
    assert record("generate.fused step logits vs unfused step (max abs, worst of 8 steps)", worst_vs_plain, 5e-2) < 5e-2
    print(f"fused decode step: {(ops.launch_count - launches) / 8:.1f} C-ABI launches per step")


def test_fused_step_with_device_parents_equals_the_unfused_step():
    """The cache ping-pong with parents that are NOT the identity, strictly: the same device tokens and parents go through the unfused step
    (kv_gather_rows + copy + head_transpose + attention_fwd) and through the fused one, 3 rows per clip, 7 positions.  Layer 0 sees the same
    embedding rows on both paths, so its K / V planes of the cache must be EQUAL BIT FOR BIT after every step — rows re-ordered by a wrong
    parent, a missed swap or a row appended to the wrong buffer cannot hide behind rounding; the deeper layers' inputs differ by the
    attention's summation order, so the logits are held to the project's 5e-2 max abs.  That this bound has teeth is checked, not claimed:
    the unfused step run once more with the parents IGNORED (identity) must move the last position's logits by more than the bound."""
    model, orc, tok, samples = _shared_model()
    eng = model.engine
    from mrblip import ops

    B, K, steps = samples["video"].shape[0], 3, 7
    R = B * K
    layout = model._layout(dict(samples))
    video = model._frames_to_device(samples["video"])
    fr = eng.frames_forward(video)[0]
    L = eng._layout_dev(layout)
    S, d = layout.S, eng.cfg.d_model
    inp = eng.buf("inputs_embeds", (B * S, d), torch.float32, zero=False)
    ops.row_copy(fr, L["frame_src"], inp, L["frame_dst"])
    ops.row_copy(eng.emb, L["emb_src"], inp, L["emb_dst"])
    cross = eng.t5_cross_kv(eng.t5_encoder_forward(inp, B, S, L["mask"]), B, S)
    g = torch.Generator().manual_seed(11)
    tokens = [torch.randint(2, eng.cfg.vocab, (R,), generator=g).int().cuda() for _ in range(steps)]
    # every row's parent is a row of ITS clip; rows repeat and rows die out, differently at every step
    parents = [(torch.arange(R) // K * K + torch.randint(0, K, (R,), generator=g)).int().cuda() for _ in range(steps)]
    assert any(not torch.equal(p.cpu(), torch.arange(R).int()) for p in parents[1:])

    identity = torch.arange(R).int().cuda()

    def run(fused, use_parents=True):
        state = eng.t5_decode_begin(R, steps + 1, alt_cache=True)
        if fused:
            state["fused"] = True
        logits, planes = [], []
        for t in range(steps):
            logits.append(eng.t5_decode_step(state, tokens[t], parents[t] if use_parents else identity, cross, B, L["mask"]).float().cpu())
            planes.append(state["kv"][:, 0, :, :t + 1].clone().cpu())
        return logits, planes

    lg_u, kv_u = run(False)
    lg_f, kv_f = run(True)
    lg_wrong, _ = run(False, use_parents=False)
    moved = float((lg_wrong[-1] - lg_u[-1]).abs().max())
    print(f"unfused step with the parents ignored: last position's logits move by {moved:.3e} (max abs)")
    assert moved > 5e-2, moved
    worst = 0.0
    for t in range(steps):
        assert torch.equal(kv_f[t].view(torch.int16), kv_u[t].view(torch.int16)), f"layer-0 cache rows differ after step {t}"
        worst = max(worst, float((lg_f[t] - lg_u[t]).abs().max()))
    assert record("generate.fused step logits vs unfused step, device parents (max abs, worst of 7 steps)", worst, 5e-2) < 5e-2


# ------------------------------------------------------------------------------------------------ (c) model
# (tiny-model fixture, seed and max_length of tests/test_beam_device_gpu.py's model-level cases: 8 positions for one beam, 10 for five)
MODEL_CASES = {1: 8, 5: 10}
NOISE = 5e-2


@functools.lru_cache(maxsize=None)
def _oracle_decode(beams):
    """the oracle's own beam search of the fixture (CPU), once per beam count: (sequences, trace, enc, atts)"""
    from mrblip.search import beam_search
    model, orc, tok, samples = _shared_model()
    B = samples["video"].shape[0]
    with torch.no_grad():
        enc, atts = orc.encode_for_generate(tok, samples, model.annoying_numbers_replacement_dict, mean_pool=False)
        trace = []
        ref = beam_search(lambda seqs: orc.next_token_logprobs(seqs, enc, atts, beams_per_clip=beams), B, beams, MODEL_CASES[beams], min_length=3,
                          length_penalty=1.0, eos_id=1, pad_id=0, start_id=0, trace=trace)
    return [s.tolist() for s in ref], trace, enc, atts


@pytest.mark.parametrize("device_search", [False, True])
@pytest.mark.parametrize("beams", [1, 5])
def test_fused_generate_token_ids_equal_oracle_decode(beams, device_search):
    """test_generate_token_ids_equal_oracle_decode (mean_pool False) with generate_fused_decode on, same rule: token ids equal the oracle's
    decode, except for at most one clip whose oracle search took a decision by less than NOISE — and that clip's sequence must still be
    near-optimal under the oracle's scoring.
    The oracle search alone (CPU) at this setting: smallest decision margin 1.0e-2 (clip 0) / 1.2e-2 (clip 1) with one beam and 2.4e-3 /
    3.5e-3 with five — BELOW NOISE for both clips: the fixture's random weights give nearly flat next-token distributions and it has no
    weight seed to vary (the weights are the golden file's), so it is the tie rule below, not the margins, that decides a difference."""
    model, orc, tok, samples = _shared_model()
    B = samples["video"].shape[0]
    ref, trace, enc, atts = _oracle_decode(beams)
    model.generate_fused_decode, model.generate_device_search = True, device_search
    try:
        out = model.generate(samples, num_beams=beams, max_length=MODEL_CASES[beams], min_length=3)
        stats = model.last_generate_stats
    finally:
        model.generate_fused_decode = model.generate_device_search = False
    assert (stats is not None) == device_search
    if device_search:
        assert stats["graph_captures"] == 0 and stats["graph_replays"] == 0
    hip = [s.tolist() for s in model.last_sequences]
    tag = f"fused generate (beams={beams}, device_search={device_search}): "
    print(tag, "HIP", hip, "oracle", ref)

    def min_margin(b):
        ms = [st[b][beams - 1] - st[b][beams] for st in trace[:-1] if st[b] is not None and len(st[b]) > beams]
        fin = trace[-1][b]
        if len(fin) > 1:
            ms.append(fin[0] - fin[1])
        return min(ms)

    def oracle_score(seq):
        t = torch.tensor(seq)[None]
        tot = 0.0
        with torch.no_grad():
            for i in range(1, t.shape[1]):
                tot += float(orc.next_token_logprobs(t[:, :i], enc[b:b + 1], atts[b:b + 1])[0, seq[i]])
        return tot / max(len(seq) - 1, 1)

    n_tied = 0
    for b, (hs, rs) in enumerate(zip(hip, ref)):
        if hs == rs:
            continue
        common = next(i for i, (x, y) in enumerate(zip(hs + [-1], rs + [-2])) if x != y)
        gap = abs(oracle_score(hs) - oracle_score(rs))
        mm = min_margin(b)
        print(tag, f"clip {b}: sequences part at position {common}; oracle scores differ by {gap:.2e}; smallest decision margin of the oracle search {mm:.2e}")
        assert mm < NOISE and gap < 0.1 and common >= 1, (hs, rs, common, gap, mm)
        n_tied += 1
    assert n_tied <= 1 and len(out["prediction"]) == B
    if n_tied == 0:
        assert out["raw_prediction"] == [tok.decode(torch.tensor(s[1:]), skip_special_tokens=True) for s in ref]


# ------------------------------------------------------------------------------------------------ (d) captured decoder step
def _graph_generate(model, samples, graph, **kw):
    model.generate_device_search = model.generate_fused_decode = True
    model.generate_graph_decode = graph
    try:
        model.generate(samples, **kw)
    finally:
        model.generate_device_search = model.generate_fused_decode = model.generate_graph_decode = False
    torch.cuda.synchronize()
    return ([s.tolist() for s in model.last_sequences], model._dev_search[1].final_scores.clone(), model.engine.ws["s_logits"].clone(),
            dict(model.last_generate_stats))


def test_captured_decode_step_equals_the_eager_fused_step_bit_for_bit():
    model, _, _, samples = _shared_model()
    kw = dict(num_beams=5, max_length=10, min_length=1)
    seq_e, sc_e, lg_e, st_e = _graph_generate(model, samples, False, **kw)
    assert st_e["graph_captures"] == 0 and st_e["graph_replays"] == 0
    seq_g, sc_g, lg_g, st_g = _graph_generate(model, samples, True, **kw)
    assert seq_g == seq_e
    assert torch.equal(sc_g.view(torch.int32), sc_e.view(torch.int32))
    assert torch.equal(lg_g.view(torch.int32), lg_e.view(torch.int32))
    assert st_g["steps"] == st_e["steps"] >= 3
    assert st_g["graph_captures"] == 2 and st_g["graph_replays"] == st_g["steps"] - 1, st_g     # one graph per direction of the cache ping-pong
    # another query length is another key; the first length again finds its two graphs
    other = dict(samples)
    other["query_prompt"] = [" ".join(q.split()[:-1]) for q in samples["query_prompt"]]
    assert model._layout(dict(other)).S != model._layout(dict(samples)).S
    seq_o_e, sc_o_e, lg_o_e, _ = _graph_generate(model, other, False, **kw)
    seq_o, sc_o, lg_o, st_o = _graph_generate(model, other, True, **kw)
    assert st_o["graph_captures"] == 2 and st_o["graph_replays"] == st_o["steps"] - 1, st_o
    assert seq_o == seq_o_e and torch.equal(sc_o.view(torch.int32), sc_o_e.view(torch.int32)) and torch.equal(lg_o.view(torch.int32), lg_o_e.view(torch.int32))
    seq_3, sc_3, lg_3, st_3 = _graph_generate(model, samples, True, **kw)
    assert st_3["graph_captures"] == 0 and st_3["graph_replays"] == st_3["steps"] - 1, st_3
    assert seq_3 == seq_e and torch.equal(sc_3.view(torch.int32), sc_e.view(torch.int32)) and torch.equal(lg_3.view(torch.int32), lg_e.view(torch.int32))
    # a LONGER query grows the step's mask workspace, which moves: every older key holds its old address, can never be met again and is
    # dropped at once, so the first length is captured anew — and still gives the eager bits
    eng = model.engine
    longer = dict(samples)
    longer["query_prompt"] = [q + " and then" * 20 for q in samples["query_prompt"]]
    assert model._layout(dict(longer)).S >= model._layout(dict(samples)).S + 32
    mask_at = eng.ws["s_kmask"].data_ptr()
    seq_l_e, sc_l_e, lg_l_e, _ = _graph_generate(model, longer, False, **kw)
    seq_l, sc_l, lg_l, st_l = _graph_generate(model, longer, True, **kw)
    assert eng.ws["s_kmask"].data_ptr() != mask_at
    assert st_l["graph_captures"] == 2 and st_l["graph_replays"] == st_l["steps"] - 1, st_l
    assert len(eng._dec_graphs) == 1
    assert seq_l == seq_l_e and torch.equal(sc_l.view(torch.int32), sc_l_e.view(torch.int32)) and torch.equal(lg_l.view(torch.int32), lg_l_e.view(torch.int32))
    seq_5, sc_5, lg_5, st_5 = _graph_generate(model, samples, True, **kw)
    assert st_5["graph_captures"] == 2 and st_5["graph_replays"] == st_5["steps"] - 1, st_5
    assert len(eng._dec_graphs) == 2
    assert seq_5 == seq_e and torch.equal(sc_5.view(torch.int32), sc_e.view(torch.int32)) and torch.equal(lg_5.view(torch.int32), lg_e.view(torch.int32))
