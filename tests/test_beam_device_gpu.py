"""The device-resident beam search (csrc/search.hip, mrblip.search.DeviceBeamSearch, BLIP2_MR.generate_device_search) against fp64
references and against the host search it restates.

TIE WINDOW (every check below).  Two correct fp32 evaluations of a candidate score differ only in how the V-term log-sum-exp and one
addition were rounded: W = 32 * 2**-23 * max|finite candidate score| of the clip and step at hand (over the beams that are live, i.e. not
at the -1e9 placeholder of step 0: the placeholder beams decide nothing, and counting them would make W thousands wide).  Only cases whose
fp64 reference keeps every RELEVANT gap above W are used, and each test asserts that its cases do (no case is excused; a seed that
violated the condition was replaced by another seed, never a wider W):
  * selection test (a): every adjacent gap among the 2K + 1 best (the test compares the whole ranked list);
  * searches (b), (d), (e), which compare final token ids: the gap below the last candidate the walk consumes (the K-th kept one; the
    2K-th against the (2K+1)-th when the walk reaches the end), the gap at the rank K - 1 / K border when an EOS sits on it (an EOS of
    rank < K is a hypothesis, one of rank >= K is dropped), every pool comparison that decides an insertion or an eviction (newcomer
    against worst, worst against second worst), the `done` rule's comparison, and the final ranking's gaps down to num_return.
"""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mr-blip_amd"))

W_FACTOR = 32 * 2.0 ** -23
EOS, PAD, START = 1, 0, 0


class Gaps:
    """the relevant gaps of a reference run, each as a multiple of its W"""

    def __init__(self):
        self.items = []

    def need(self, gap, W, what):
        self.items.append((gap / W if W > 0 else math.inf, what))

    def check(self, tag):
        worst = min(self.items, default=(math.inf, ""))
        assert worst[0] > 1.0, f"{tag}: a relevant gap of the fp64 reference is only {worst[0]:.3g} W ({worst[1]}): pick another seed"
        return worst[0]


class ClipBook:
    """search.py:134-170 for one clip in Python floats (fp64), recording the gaps its decisions rest on"""

    def __init__(self, K, V, length_penalty, gaps):
        self.K, self.V, self.lp, self.gaps = K, V, length_penalty, gaps
        self.pool, self.done, self.W = [], False, 0.0        # pool: [score, payload], any order (list semantics of search.py)

    def _add(self, score, payload, what):
        K, g = self.K, self.gaps
        if len(self.pool) >= K:
            order = sorted(range(K), key=lambda j: self.pool[j][0])
            g.need(abs(score - self.pool[order[0]][0]), self.W, what + ": newcomer against the pool's worst")
            if not score > self.pool[order[0]][0]:
                return
            if K > 1:
                g.need(min(self.pool[order[1]][0], score) - self.pool[order[0]][0], self.W, what + ": worst against second worst")
            del self.pool[order[0]]
        self.pool.append([score, payload])

    def step(self, top, idx, nxt, absmax, cur_len, seq_of=None):
        """top / idx: the 2K best, nxt: score of the (2K+1)-th -> the K new beams [(beam, token, score)]"""
        K, V, g = self.K, self.V, self.gaps
        self.W = W_FACTOR * absmax
        kept, last = [], None
        toks = [ix % V for ix in idx]
        for rank, (sc, ix) in enumerate(zip(top, idx)):
            beam, tok = divmod(ix, V)
            if tok == EOS:
                if rank < K:
                    self._add(sc / (cur_len ** self.lp), None if seq_of is None else seq_of(beam) + [EOS], f"step {cur_len} EOS")
                continue
            kept.append((beam, tok, sc))
            if len(kept) == K:
                last = rank
                break
        assert last is not None
        ext = list(top) + [nxt]
        g.need(ext[last] - ext[last + 1], self.W, f"step {cur_len}: below the last consumed candidate (rank {last})")
        if len(top) > K and EOS in (toks[K - 1], toks[K]):
            g.need(top[K - 1] - top[K], self.W, f"step {cur_len}: EOS at the rank K-1 / K border")
        if len(self.pool) >= K:
            worst, thr = min(s for s, _ in self.pool), top[0] / (cur_len ** self.lp)
            # (an EOS of rank 0 that has just entered the pool as its worst entry IS the threshold: the same number divided the same
            # way, equal in every implementation — an identity, not a numeric tie)
            if not (toks[0] == EOS and worst == thr):
                g.need(abs(worst - thr), self.W, f"step {cur_len}: done rule")
            self.done = worst >= thr
        return kept

    def finalize(self, running, gen_len, num_return):
        """running: [(score, payload)] of the K beams -> the num_return best payloads"""
        if not self.done:
            for sc, payload in running:
                self._add(sc / (gen_len ** self.lp), payload, "finalize")
        ranked = sorted(self.pool, key=lambda t: t[0], reverse=True)
        for r in range(min(num_return, len(ranked) - 1)):
            self.gaps.need(ranked[r][0] - ranked[r + 1][0], self.W, f"final ranking {r} / {r + 1}")
        return [p for _, p in ranked[:num_return]], [s for s, _ in ranked]


def _ref_candidates(logits, beam_scores, seqs, K, cur_len, min_length, penalty):
    """fp64: candidate scores [B, K * V] of search.py:124-131 and the W magnitude (largest finite |score| over live beams) per clip"""
    from mrblip.search import repetition_penalty_
    R, V = logits.shape
    B = R // K
    lp = torch.log_softmax(logits.double(), -1)
    if penalty != 1.0:
        repetition_penalty_(lp, seqs[:, :cur_len].long(), float(penalty))
    if cur_len < min_length:
        lp[:, EOS] = -math.inf
    cand = (lp + beam_scores.double().view(R, 1)).view(B, K * V)
    live = (beam_scores.view(B, K, 1) > -1e8).expand(B, K, V).reshape(B, K * V) & torch.isfinite(cand)
    return cand, cand.abs().masked_fill(~live, 0.0).amax(-1)


def ref_search(logits_fn, B, K, max_new, min_length, length_penalty, penalty, num_return, V):
    """the whole search in fp64 on RAW fp32 logits from logits_fn(seqs int64 [B * K, L]); returns (hypotheses as lists, item-major; Gaps;
    per-step done flags)"""
    gaps = Gaps()
    books = [ClipBook(K, V, length_penalty, gaps) for _ in range(B)]
    seqs = [[START] for _ in range(B * K)]
    bs = torch.zeros(B, K, dtype=torch.float64)
    bs[:, 1:] = -1e9
    done_hist = []
    for step in range(max_new):
        cur_len = step + 1
        st = torch.tensor(seqs)
        cand, absmax = _ref_candidates(logits_fn(st), bs.view(-1), st, K, cur_len, min_length, penalty)
        n = min(2 * K + 1, K * V)
        top, idx = cand.topk(n, dim=-1)
        new_seqs, new_bs = [None] * (B * K), torch.zeros(B, K, dtype=torch.float64)
        for b in range(B):
            if books[b].done:
                for k in range(K):
                    new_seqs[b * K + k] = seqs[b * K + k] + [PAD]
                continue
            nxt = top[b, 2 * K].item() if n > 2 * K else -math.inf
            kept = books[b].step(top[b, :2 * K].tolist(), idx[b, :2 * K].tolist(), nxt, absmax[b].item(), cur_len,
                                 seq_of=lambda beam, b=b: seqs[b * K + beam])
            for k, (beam, tok, sc) in enumerate(kept):
                new_seqs[b * K + k] = seqs[b * K + beam] + [tok]
                new_bs[b, k] = sc
        seqs, bs = new_seqs, new_bs
        done_hist.append([bk.done for bk in books])
        if all(done_hist[-1]):
            break
    out = []
    for b in range(B):
        hyps, _ = books[b].finalize([(bs[b, k].item(), seqs[b * K + k]) for k in range(K)], len(seqs[0]) - 1, num_return)
        out.extend(hyps)
    return out, gaps, done_hist


# ------------------------------------------------------------------------------------------------ (a) beam_topk against fp64
TOPK_VARIANTS = ("plain", "penalty", "eos_masked", "step0")
# seeds: 7000 + a case number, except where that seed's fp64 reference had an adjacent gap inside W among its 2K + 1 best
TOPK_SEED_OVERRIDES = {(32128, 16, 3, "penalty"): 7129, (32128, 16, 3, "eos_masked"): 7230, (48, 16, 3, "plain"): 7160}


def _topk_case(V, K, B, variant, seed):
    g = torch.Generator().manual_seed(seed)
    R = B * K
    logits = torch.randn(R, V, generator=g) * 3.0
    cur_len = 1 if variant == "step0" else 6
    seqs = torch.randint(0, V, (R, 8), generator=g, dtype=torch.int32)
    seqs[:, 0] = START
    if variant == "step0":
        scores = torch.zeros(B, K)
        scores[:, 1:] = -1e9
    else:
        scores = -5.0 * torch.rand(B, K, generator=g)
    penalty = 1.3 if variant == "penalty" else 1.0
    min_length = 9 if variant == "eos_masked" else 1
    return logits, scores, seqs, cur_len, min_length, penalty


def _topk_cases():
    n = 0
    for V in (32128, 48):
        for K in (1, 2, 5, 16):
            for B in (1, 3):
                for variant in TOPK_VARIANTS:
                    key = (V, K, B, variant)
                    yield key + (TOPK_SEED_OVERRIDES.get(key, 7000 + n),)
                    n += 1


def topk_reference(V, K, B, variant, seed):
    logits, scores, seqs, cur_len, min_length, penalty = _topk_case(V, K, B, variant, seed)
    cand, absmax = _ref_candidates(logits, scores.view(-1), seqs, K, cur_len, min_length, penalty)
    n = min(2 * K + 1, K * V)
    top, idx = cand.topk(n, dim=-1)
    W = W_FACTOR * absmax
    gaps = Gaps()
    for b in range(B):
        for r in range(n - 1):
            gaps.need((top[b, r] - top[b, r + 1]).item(), W[b].item(), f"clip {b} ranks {r} / {r + 1}")
    return top[:, :2 * K], idx[:, :2 * K], W, gaps


@pytest.mark.parametrize("V,K,B,variant,seed", list(_topk_cases()))
def test_beam_topk_equals_fp64_topk(V, K, B, variant, seed):
    from mrblip import ops
    logits, scores, seqs, cur_len, min_length, penalty = _topk_case(V, K, B, variant, seed)
    top, idx, W, gaps = topk_reference(V, K, B, variant, seed)
    gaps.check(f"topk {V, K, B, variant, seed}")
    dev = "cuda"
    lg, sc, sq = logits.to(dev), scores.to(dev).contiguous(), seqs.to(dev)
    ws = torch.empty(ops.beam_topk_workspace_bytes(B * K, K, V), dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        cs = torch.full((B, 2 * K), float("nan"), device=dev)
        ci = torch.full((B, 2 * K), -7, dtype=torch.int32, device=dev)
        ws.random_(0, 256)      # the scratch carries no state between calls
        ops.beam_topk(lg, sc, sq, cur_len, K, cs, ci, ws, min_length=min_length, eos_id=EOS, repetition_penalty=penalty)
        runs.append((cs.cpu(), ci.cpu()))
    (cs, ci), (cs2, ci2) = runs
    assert torch.equal(ci, ci2) and torch.equal(cs.view(torch.int32), cs2.view(torch.int32)), "two runs differ in their bits"
    err = (cs.double() - top).abs()
    print(f"beam_topk V={V} K={K} B={B} {variant}: max score error {err.max().item():.3e}, W {W.min().item():.3e}")
    assert torch.equal(ci.long(), idx), (ci.tolist(), idx.tolist())
    assert bool((err <= W.view(B, 1)).all()), (err.max().item(), W.tolist())
    if variant == "step0":
        assert bool((ci < V).all()), "step 0: every candidate has to come from beam 0"
    if variant == "eos_masked":
        assert not bool(((ci % V) == EOS).any())


# ------------------------------------------------------------------------------------------------ (b) step-wise search against HF
def _t5(seed, eos_boost):
    """the tiny random T5 of tests/test_search_cpu.py::_model"""
    from transformers import T5Config, T5ForConditionalGeneration

    torch.manual_seed(seed)
    cfg = T5Config(vocab_size=48, d_model=32, d_kv=8, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=4, feed_forward_proj="gated-gelu",
                   tie_word_embeddings=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1, dropout_rate=0.0)
    m = T5ForConditionalGeneration(cfg).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(3.0)
        m.lm_head.weight[1] *= eos_boost
    return m


def _t5_inputs(m, seed_base, seed, B, S, short_clip):
    g = torch.Generator().manual_seed(seed_base + seed)
    emb = torch.randn(B, S, 32, generator=g)
    mask = torch.ones(B, S, dtype=torch.long)
    if short_clip:
        mask[1, 5:] = 0
    with torch.no_grad():
        enc = m.encoder(inputs_embeds=emb, attention_mask=mask).last_hidden_state

    def raw_logits(seqs):
        rep = seqs.shape[0] // B
        with torch.no_grad():
            out = m(encoder_outputs=(enc.repeat_interleave(rep, 0),), attention_mask=mask.repeat_interleave(rep, 0), decoder_input_ids=seqs)
        return out.logits[:, -1].float()

    return emb, mask, raw_logits


def _strip_hf(row):
    r = row.tolist()
    return r[: r.index(EOS, 1) + 1] if EOS in r[1:] else r


def _same_as_hf(mine, r):
    return mine == r[:len(mine)] and all(t == PAD for t in r[len(mine):])


def search_case(m, emb, mask, raw_logits, B, K, max_new, lp, pen, n_ret, on_device):
    """reference chain of one configuration (fp64 search == mrblip.search.beam_search == HF generate, gaps above W) and, on_device, the
    DeviceBeamSearch fed the same model's logits step by step.  Returns (number of hypotheses ending in EOS, a clip was done while
    another ran)"""
    from mrblip.search import beam_search, DeviceBeamSearch
    tag = f"K={K} lp={lp} max_new={max_new} pen={pen} n_ret={n_ret}"
    ref, gaps, done_hist = ref_search(raw_logits, B, K, max_new, 1, lp, pen, n_ret, 48)
    gaps.check(tag)
    host = beam_search(lambda seqs: torch.log_softmax(raw_logits(seqs), -1), B, K, max_new, min_length=1, length_penalty=lp, repetition_penalty=pen,
                       num_return=n_ret)
    assert [h.tolist() for h in host] == ref, (tag, "fp64 reference against mrblip.search.beam_search")
    with torch.no_grad():
        hf = m.generate(inputs_embeds=emb, attention_mask=mask, do_sample=False, num_beams=K, max_new_tokens=max_new, min_length=1, length_penalty=lp,
                        num_return_sequences=n_ret, repetition_penalty=pen, early_stopping=False)
    assert hf.shape[0] == B * n_ret
    for i in range(B * n_ret):
        assert _same_as_hf(ref[i], _strip_hf(hf[i])), (tag, i, ref[i], hf[i].tolist())
    if on_device:
        search = DeviceBeamSearch(B, K, max_new, min_length=1, length_penalty=lp, eos_id=EOS, pad_id=PAD, start_id=START, repetition_penalty=pen,
                                  num_return=n_ret, device="cuda")
        for step in range(max_new):
            search.step(raw_logits(search.sequences.cpu().long()).cuda())
            search.done_count_async()
            done = [bool(d) for d in search._done.cpu().tolist()]
            assert done == done_hist[step], (tag, step, done, done_hist[step])
            assert int(search._done_count.cpu()) == sum(done)
            if all(done):
                break
        got = [h.tolist() for h in search.finalize()]
        assert got == ref, (tag, got, ref)
    return sum(int(h[-1] == EOS) for h in ref), any(any(d) and not all(d) for d in done_hist)


# (tests/test_search_cpu.py's seeds, except (2, 4.0): with length_penalty 2 its pool scores, divided by up to 81, come within 0.5 W of each
# other — W is sized for the undivided candidate scores — so, by the rule above, another seed stands in for it)
GRID_SEEDS = [(0, 1.0), (1, 2.5), (10, 4.0)]
PEN_SEEDS = [(3, 1.0), (4, 2.5)]


def run_grid(seed, eos_boost, on_device):
    m = _t5(seed, eos_boost)
    B = 3
    emb, mask, raw_logits = _t5_inputs(m, 100, seed, B, 7, True)
    n_eos, staggered = 0, False
    for K in (1, 2, 5):
        for lp in (1.0, 0.5, 2.0):
            for max_new in (4, 9):
                e, s = search_case(m, emb, mask, raw_logits, B, K, max_new, lp, 1.0, 1, on_device)
                n_eos, staggered = n_eos + e, staggered or s
    return n_eos, staggered


def run_pen(seed, eos_boost, on_device):
    m = _t5(seed, eos_boost)
    B = 2
    emb, mask, raw_logits = _t5_inputs(m, 200, seed, B, 6, False)
    n_eos, staggered = 0, False
    for K, n_ret, pen in ((3, 1, 1.3), (4, 3, 1.0), (5, 2, 2.0)):
        e, s = search_case(m, emb, mask, raw_logits, B, K, 8, 1.0, pen, n_ret, on_device)
        n_eos, staggered = n_eos + e, staggered or s
    return n_eos, staggered


_staggered_seen = []


@pytest.mark.parametrize("seed,eos_boost", GRID_SEEDS)
def test_device_search_equals_hf_generate(seed, eos_boost):
    n_eos, staggered = run_grid(seed, eos_boost, True)
    assert eos_boost == 1.0 or n_eos > 0
    _staggered_seen.append(staggered)


@pytest.mark.parametrize("seed,eos_boost", PEN_SEEDS)
def test_device_search_repetition_penalty_and_num_return_equal_hf_generate(seed, eos_boost):
    run_pen(seed, eos_boost, True)


def test_a_clip_finishes_while_another_still_runs():
    """at least one configuration of the EOS-boosted grid reaches `done` for one clip while another clip is still running (the device
    search's done flags are compared with the reference's after every step in search_case)"""
    seen = any(_staggered_seen) if len(_staggered_seen) == len(GRID_SEEDS) else any(run_grid(s, e, True)[1] for s, e in GRID_SEEDS[1:])
    assert seen


# ------------------------------------------------------------------------------------------------ (c) kv_gather_rows
@pytest.mark.parametrize("t", [1, 7, 32])
def test_kv_gather_rows_equals_index_select(t):
    from mrblip import ops
    layers, R, Lmax, inner = 3, 10, 32, 64
    g = torch.Generator().manual_seed(t)
    src = torch.randn(2, layers, R, Lmax, inner, generator=g).bfloat16().cuda()
    parents = torch.tensor([0, 0, 3, 1, 1, 9, 9, 9, 2, 5], dtype=torch.int32)
    dst = torch.full_like(src, 7.0)
    ops.kv_gather_rows(src, dst, parents.cuda(), t)
    want = torch.full_like(src, 7.0)
    want[:, :, :, :t] = src[:, :, :, :t].index_select(2, parents.long().cuda())
    assert torch.equal(dst.view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------ (d), (e) model level
def _tiny_model(mean):
    from test_generate_gpu import _model_and_oracle
    model, _, _, samples = _model_and_oracle(mean)
    return model, samples


def _host_generate(model, samples, **kw):
    """generate on the host search, with the margin rule checked on its trace: returns (last_sequences, raw_prediction, steps run)"""
    model.generate_device_search = False
    model.generate_trace, model.generate_detail = [], []
    try:
        out = model.generate(samples, **kw)
        trace, detail = model.generate_trace, model.generate_detail
    finally:
        model.generate_trace = model.generate_detail = None
    B = samples["video"].shape[0]
    K, n_ret = max(1, int(kw.get("num_beams", 5))), max(1, int(kw.get("num_captions", 1)))
    V = model.engine.cfg.vocab
    gaps = Gaps()
    books = [ClipBook(K, V, float(kw.get("length_penalty", 1.0)), gaps) for _ in range(B)]
    running = [None] * B
    steps = len(detail)
    for step in range(steps):
        for b in range(B):
            d = detail[step][b]
            if d is None:
                continue
            assert not books[b].done
            kept = books[b].step(trace[step][b], d["idx"], d["next"], d["absmax"], step + 1)
            running[b] = [(sc, None) for _, _, sc in kept]
    for b in range(B):
        _, ranked = books[b].finalize(running[b], steps, n_ret)
        assert ranked == pytest.approx(trace[-1][b], rel=1e-6, abs=1e-6)      # the replay followed the host search
    worst = gaps.check(f"generate {kw}")
    print(f"generate {kw}: {steps} steps, smallest relevant gap of the host search {worst:.3g} W")
    return [s.tolist() for s in model.last_sequences], out["raw_prediction"], steps


def _device_generate(model, samples, **kw):
    model.generate_device_search = True
    try:
        out = model.generate(samples, **kw)
    finally:
        model.generate_device_search = False
    return [s.tolist() for s in model.last_sequences], out["raw_prediction"], model.last_generate_stats


# (max_length is this file's choice: 10, except one beam, whose greedy walk of the mean=False fixture meets a top-1 / top-2 gap of 0.39 W at
# step 9 — the fixture's random weights give nearly flat distributions — and therefore stops at 8)
GENERATE_CASES = [
    dict(num_beams=1, max_length=8, min_length=1),
    dict(num_beams=5, max_length=10, min_length=1),
    dict(num_beams=5, max_length=10, min_length=1, num_captions=3),
    dict(num_beams=5, max_length=10, min_length=1, length_penalty=0.5),
    dict(num_beams=5, max_length=10, min_length=1, length_penalty=2.0),
    dict(num_beams=5, max_length=10, min_length=1, repetition_penalty=1.3),
    dict(num_beams=5, max_length=10, min_length=3),
]


@pytest.mark.parametrize("mean", [False, True])
def test_generate_with_device_search_equals_host_search(mean):
    model, samples = _tiny_model(mean)
    for kw in GENERATE_CASES:
        seqs_h, raw_h, steps_h = _host_generate(model, samples, **kw)
        assert model.last_generate_stats is None
        seqs_d, raw_d, stats = _device_generate(model, samples, **kw)
        assert stats is not None, "the device path was not taken"
        assert seqs_d == seqs_h and raw_d == raw_h, (kw, seqs_d, seqs_h)


def test_generate_falls_back_to_the_host_search():
    """sampling calls, the greedy-with-penalty route and generate_self_cache = False keep the host path although the switch is on"""
    model, samples = _tiny_model(False)
    model.generate(samples, num_beams=5, max_length=8, min_length=2)
    want = [s.tolist() for s in model.last_sequences]
    model.generate_self_cache = False
    try:
        seqs, _, stats = _device_generate(model, samples, num_beams=5, max_length=8, min_length=2)
    finally:
        model.generate_self_cache = True
    assert stats is None and seqs == want
    runs = []
    for on in (False, True):
        model.sampling_generator = torch.Generator().manual_seed(7)
        model.generate_device_search = on
        try:
            model.generate(samples, use_nucleus_sampling=True, num_beams=1, top_p=0.9, temperature=0.7, repetition_penalty=1.2, num_captions=3,
                           max_length=8, min_length=2)
        finally:
            model.generate_device_search = False
        assert model.last_generate_stats is None
        runs.append([s.tolist() for s in model.last_sequences])
    assert runs[0] == runs[1]
    model.generate(samples, num_beams=1, repetition_penalty=1.5, max_length=8, min_length=2)
    want = [s.tolist() for s in model.last_sequences]
    seqs, _, stats = _device_generate(model, samples, num_beams=1, repetition_penalty=1.5, max_length=8, min_length=2)
    assert stats is None and seqs == want


def _tiny_model_eos(eos_scale):
    """the golden tiny model with the EOS row of the LM head scaled: the fixture's random weights never finish a hypothesis, so the plain
    model would run all max_length steps whatever the polling does; with the row scaled clips finish, and at different steps (CPU decode
    of the same weights: scale -4 -> 5 beams end after 8 steps and 2 beams after 4; scale 8 -> 2 beams end after 11)"""
    import lavis  # noqa: F401
    from lavis.common.registry import registry
    from mrblip.engine import EngineConfig
    from mrblip.tokenizer import FixtureTokenizer
    from test_model_gpu import _peft_sd, _samples
    from util import load_golden, golden_state_dict

    g = load_golden("mr_tiny")
    sdl = dict(_peft_sd(golden_state_dict(g)))
    key = "t5_model.base_model.model.lm_head.base_layer.weight"
    w = sdl[key].clone()
    w[EOS] *= eos_scale
    sdl[key] = w
    cls = registry.get_model_class("blip2_mr")
    model = cls(img_size=56, num_query_token=8, engine_config=EngineConfig.tiny(), weights=sdl, tokenizer=FixtureTokenizer(), interleave_data=True,
                task="qformer_freeze_lora", input_time_format="seconds_integers", frame_token_aggregation=None, seed=42).eval()
    return model, _samples(g)


@pytest.mark.parametrize("eos_scale,kw", [(-4.0, dict(num_beams=5, max_length=24, min_length=1)), (-4.0, dict(num_beams=2, max_length=24, min_length=1)),
                                          (8.0, dict(num_beams=2, max_length=24, min_length=1))])
def test_early_stop_is_only_an_optimisation(eos_scale, kw):
    """all max_length steps (polling off) give the polled run's output, and polling enqueues at most two steps more than the host search"""
    model, samples = _tiny_model_eos(eos_scale)
    seqs_h, raw_h, steps_h = _host_generate(model, samples, **kw)
    assert steps_h < kw["max_length"], "the case has to finish early, or it shows nothing"
    seqs_p, raw_p, stats_p = _device_generate(model, samples, **kw)
    model.generate_poll_done = False
    try:
        seqs_f, raw_f, stats_f = _device_generate(model, samples, **kw)
    finally:
        model.generate_poll_done = True
    print(f"early stop scale {eos_scale} {kw}: host {steps_h} steps, polled {stats_p}, unpolled {stats_f}")
    assert stats_f["steps"] == kw["max_length"] and stats_f["steps_after_done"] == kw["max_length"] - steps_h
    assert seqs_p == seqs_f == seqs_h and raw_p == raw_f == raw_h
    assert stats_p["steps"] <= steps_h + 2 and stats_p["steps_after_done"] == stats_p["steps"] - steps_h
