"""Beam search over a decoder step function — the host-side search of ``BLIP2_MR.generate`` (blip2_mr.py:883-899 calls HF
``t5_model.generate(num_beams=5, max_new_tokens=50, min_length=1, length_penalty=1.0, do_sample=False)``).

Semantics follow HF's beam search for an encoder-decoder (transformers 4.46 ``GenerationMixin._beam_search`` + ``BeamSearchScorer``,
early_stopping=False): scores are sums of log-probabilities; each step ranks the 2K best (beam, token) continuations of every batch
item; an EOS continuation ranked inside the first K becomes a finished hypothesis with score sum_logprobs / generated_len ** length_penalty
(generated_len counts the EOS, not the start token) — one ranked K..2K-1 is dropped; the first K non-EOS continuations are the next
beams; the hypothesis pool keeps the K best; a batch item is done when the pool is full and its worst score is at least
best_running_sum / generated_len ** length_penalty; at the length limit the running beams are added to the pool; the best hypothesis
wins.  HF itself is third-party (not in the reference tree): tests/test_search_cpu.py pins this module against the HF implementation
present in the image (transformers 5.x ``generate`` on a small random T5).
"""
from typing import Optional, Callable, List

import torch


def repetition_penalty_(scores: torch.Tensor, seqs: torch.Tensor, penalty: float) -> torch.Tensor:
    """HF RepetitionPenaltyLogitsProcessor (in place): every token id already in a row's sequence (the decoder input ids, start token
    included) gets score * penalty if its score is negative, score / penalty otherwise."""
    if penalty != 1.0:
        sc = scores.gather(1, seqs)
        scores.scatter_(1, seqs, torch.where(sc < 0, sc * penalty, sc / penalty))
    return scores


def top_p_filter_(scores: torch.Tensor, top_p: float, min_tokens_to_keep: int = 1) -> torch.Tensor:
    """HF TopPLogitsWarper (in place): the smallest set of most-probable tokens whose mass reaches top_p survives, the rest -> -inf"""
    if top_p < 1.0:
        sorted_scores, sorted_idx = torch.sort(scores, descending=False)
        cum = sorted_scores.softmax(dim=-1).cumsum(dim=-1)
        remove = cum <= (1 - top_p)
        remove[..., -min_tokens_to_keep:] = False
        scores.masked_fill_(remove.scatter(1, sorted_idx, remove), -float("inf"))
    return scores


def top_k_filter_(scores: torch.Tensor, top_k: int, min_tokens_to_keep: int = 1) -> torch.Tensor:
    """HF TopKLogitsWarper (in place): everything below the k-th largest logit of a row -> -inf (ties with the k-th survive)"""
    k = min(max(int(top_k), min_tokens_to_keep), scores.shape[-1])
    if k > 0 and k < scores.shape[-1]:
        kth = torch.topk(scores, k)[0][..., -1, None]
        scores.masked_fill_(scores < kth, -float("inf"))
    return scores


def sample_search(step_fn: Callable[[torch.Tensor], torch.Tensor], batch: int, num_return: int, max_new_tokens: int, min_length: int = 1,
                  top_p: float = 0.9, temperature: float = 1.0, repetition_penalty: float = 1.0, eos_id: int = 1, pad_id: int = 0,
                  start_id: int = 0, generator: Optional[torch.Generator] = None, greedy: bool = False,
                  top_k: int = 50) -> List[torch.Tensor]:
    """Multinomial ("nucleus") sampling, the reference's ``generate(use_nucleus_sampling=True, num_beams=1)`` -> HF ``_sample``
    (blip2_mr.py:883-899: do_sample=True, top_p, temperature, repetition_penalty, num_return_sequences=num_captions).  step_fn(seqs
    [batch * num_return, L]) -> RAW next-token logits [rows, V] (the repetition penalty depends on the logits' signs).  Order of the
    warps as in HF: repetition penalty, min-length EOS ban, temperature, top-k, top-p, softmax, one multinomial draw per row (top_k = 50
    is ``GenerationConfig``'s default in the reference's pinned transformers 4.46.1: the reference never overrides it, so HF puts
    TopKLogitsWarper(50) between the temperature and the top-p warps; 0 switches it off); a finished row
    keeps emitting the pad id.  greedy=True: HF's greedy decoding (do_sample=False, num_beams=1) — argmax of the penalised RAW logits,
    no temperature / top-p (HF ignores them without sampling); needed because with ONE beam HF applies the repetition penalty to raw
    logits, whose signs differ from the log-probabilities its beam search penalises.
    Returns batch * num_return sequences (item-major), start token first."""
    R = batch * max(1, int(num_return))
    seqs = torch.full((R, 1), start_id, dtype=torch.long)
    unfinished = torch.ones(R, dtype=torch.bool)
    takes_parents = bool(getattr(step_fn, "takes_parents", False))
    for _ in range(max_new_tokens):
        logits = (step_fn(seqs, None) if takes_parents else step_fn(seqs)).float().clone()
        repetition_penalty_(logits, seqs, float(repetition_penalty))
        if seqs.shape[1] < min_length:
            logits[:, eos_id] = -float("inf")
        if greedy:
            nxt = logits.argmax(dim=-1)
        else:
            if temperature != 1.0:
                logits = logits / temperature
            top_k_filter_(logits, int(top_k))
            top_p_filter_(logits, float(top_p))
            nxt = torch.multinomial(torch.softmax(logits, dim=-1), num_samples=1, generator=generator).squeeze(1)
        nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad_id))
        seqs = torch.cat([seqs, nxt[:, None]], dim=1)
        unfinished = unfinished & (nxt != eos_id)
        if not bool(unfinished.any()):
            break
    out = []
    for r in range(R):
        row = seqs[r]
        hit = (row[1:] == eos_id).nonzero()
        out.append(row[: int(hit[0]) + 2] if hit.numel() else row)
    return out


def beam_search(step_fn: Callable[[torch.Tensor], torch.Tensor], batch: int, num_beams: int, max_new_tokens: int, min_length: int = 1,
                length_penalty: float = 1.0, eos_id: int = 1, pad_id: int = 0, start_id: int = 0, trace: Optional[list] = None,
                repetition_penalty: float = 1.0, num_return: int = 1, detail: Optional[list] = None) -> List[torch.Tensor]:
    """step_fn(seqs [batch * K, L] int64) -> log-probabilities [batch * K, V] (float32, CPU) of the next token.
    A step function with a truthy ``takes_parents`` attribute is called as step_fn(seqs, parents): parents [batch * K] int64 names, for
    every row of ``seqs``, the row of the PREVIOUS call it extends (None on the first call) — what an incremental decoder needs to
    re-order its self-attention K/V cache (HF's ``_reorder_cache(beam_idx)``).
    trace (diagnostics, optional list): receives one entry per step — for every batch item the 2K best candidate scores, best first
    (entry[b][K-1] - entry[b][K] is the margin by which the K-th beam survived the pruning) — and a last entry with every item's final
    pool scores, best first; tests use it to tell a genuine tie from a wrong result.
    detail (diagnostics, optional list): one entry per step — for every batch item (None once it is done) a dict with ``idx`` (the flat
    indices beam * V + token of the 2K best, in ``trace``'s order), ``next`` (score of the (2K+1)-th candidate, -inf if there is none) and
    ``absmax`` (largest finite |candidate score| over the item's live beams, i.e. those not at the -1e9 placeholder).
    repetition_penalty: HF's processor on the log-probabilities of the tokens already in each beam.  num_return (<= num_beams): the
    ``num_return_sequences`` best hypotheses of every item, best first (HF's BeamSearchScorer.finalize).
    Returns num_return 1-D tensors per batch item (item-major): start token, generated tokens, EOS if the hypothesis ended with one."""
    B, K = batch, max(1, int(num_beams))
    seqs = torch.full((B * K, 1), start_id, dtype=torch.long)
    beam_scores = torch.zeros(B, K)
    beam_scores[:, 1:] = -1e9
    pools = [[] for _ in range(B)]          # per item: list of (score, tensor), at most K, any order
    worst = [1e9] * B
    done = [False] * B

    def pool_add(b, hyp, sum_logprobs, generated_len):
        score = sum_logprobs / (generated_len ** length_penalty)
        if len(pools[b]) < K or score > worst[b]:
            pools[b].append((score, hyp))
            if len(pools[b]) > K:
                pools[b].remove(min(pools[b], key=lambda t: t[0]))
            worst[b] = min(s for s, _ in pools[b])

    takes_parents = bool(getattr(step_fn, "takes_parents", False))
    parents = None
    for _ in range(max_new_tokens):
        cur_len = seqs.shape[1]                                  # includes the start token
        lp = (step_fn(seqs, parents) if takes_parents else step_fn(seqs)).float()
        V = lp.shape[-1]
        if repetition_penalty != 1.0:
            lp = repetition_penalty_(lp.clone(), seqs, float(repetition_penalty))
        if cur_len < min_length:
            lp[:, eos_id] = -float("inf")
        cand = (lp + beam_scores.view(B * K, 1)).view(B, K * V)
        top, idx = cand.topk(min(2 * K, K * V), dim=-1)
        if trace is not None:
            trace.append([None if done[b] else top[b].tolist() for b in range(B)])
        if detail is not None:
            nxt = cand.topk(2 * K + 1, dim=-1)[0][:, -1].tolist() if K * V > 2 * K else [-float("inf")] * B
            live = (beam_scores > -1e8).view(B, K, 1).expand(B, K, V).reshape(B, K * V) & torch.isfinite(cand)
            absmax = cand.abs().masked_fill(~live, 0.0).amax(-1).tolist()
            detail.append([None if done[b] else dict(idx=idx[b].tolist(), next=nxt[b], absmax=absmax[b]) for b in range(B)])
        new_seqs = torch.full((B * K, cur_len + 1), pad_id, dtype=torch.long)
        new_scores = torch.zeros(B, K)
        parents = torch.arange(B * K)
        for b in range(B):
            if done[b]:                                          # padded beams with score 0, like HF
                new_seqs[b * K:(b + 1) * K, :cur_len] = seqs[b * K:(b + 1) * K]
                continue
            kept = 0
            for rank, (sc, ix) in enumerate(zip(top[b].tolist(), idx[b].tolist())):
                beam, tok = ix // V, ix % V
                if tok == eos_id:
                    if rank >= K:
                        continue
                    pool_add(b, torch.cat([seqs[b * K + beam], torch.tensor([eos_id])]), sc, cur_len)   # cur_len + 1 - 1 generated tokens
                    continue
                new_seqs[b * K + kept, :cur_len] = seqs[b * K + beam]
                new_seqs[b * K + kept, cur_len] = tok
                new_scores[b, kept] = sc
                parents[b * K + kept] = b * K + beam
                kept += 1
                if kept == K:
                    break
            assert kept == K, "fewer than K live continuations among the 2K best (cannot happen: at most K of them are EOS)"
            if len(pools[b]) >= K:                                # early_stopping=False: can any running beam still beat the pool's worst?
                best_running = top[b].max().item()
                done[b] = worst[b] >= best_running / (cur_len ** length_penalty)
        seqs, beam_scores = new_seqs, new_scores
        if all(done):
            break
    out = []
    for b in range(B):
        if not done[b]:                                           # finalize: running beams join the pool
            for k in range(K):
                pool_add(b, seqs[b * K + k], beam_scores[b, k].item(), seqs.shape[1] - 1)
        ranked = sorted(pools[b], key=lambda t: t[0], reverse=True)   # (stable: ties keep pool order, as HF's sort of (score, hyp) does not matter here)
        assert 1 <= num_return <= K, "num_return_sequences has to be smaller or equal to num_beams"
        out.extend(h for _, h in ranked[:num_return])
    if trace is not None:
        trace.append([sorted((sc for sc, _ in pools[b]), reverse=True) for b in range(B)])
    return out


class DeviceBeamSearch:
    """``beam_search`` with its whole state in device memory (csrc/search.hip): the candidate selection over [B * K, V] logits, the beam /
    hypothesis-pool bookkeeping and the `done` rule run as HIP kernels, so a decoding loop never waits for the host:

        search = DeviceBeamSearch(B, K, max_new, ...)
        for _ in range(max_new):
            if search.finished():                       # polls an event, never waits
                break
            logits = decoder(search.tokens, search.parents)      # device int32 [B * K]: newest token / row of the previous step
            search.step(logits)                                   # RAW fp32 logits [B * K, V] (the log-softmax is part of the kernel)
            search.done_count_async()
        hyps = search.finalize()                                  # the one blocking transfer

    The constructor mirrors ``beam_search``; ``finalize`` returns what it returns.  Ties: equal candidate scores rank by lower flat index
    beam * V + token, equal pool scores by lower pool slot.  State comes from ``buf`` (a named-workspace allocator such as
    ``Engine.buf``: ``buf(name, shape, dtype)``) or from plain tensors on ``device``.

    State layout (int32 unless noted): seq [2, B * K, L] ping-pong halves of the running sequences (L = max_new + 1, start token first);
    scores fp32 [B, K]; parents / tokens [B * K]; pool_score fp32 / pool_len [B, K], pool_seq [B, K, L], pool_n [B]; done [B];
    done_count [1]; candidates of the current step: cand_score fp32 / cand_index [B, 2K]; selection scratch (bytes)."""

    def __init__(self, batch: int, num_beams: int, max_new_tokens: int, min_length: int = 1, length_penalty: float = 1.0, eos_id: int = 1,
                 pad_id: int = 0, start_id: int = 0, repetition_penalty: float = 1.0, num_return: int = 1, device=None, buf=None,
                 poll_lag: int = 2):
        from mrblip import ops
        self._ops = ops
        B, K = int(batch), max(1, int(num_beams))
        assert 1 <= K <= 16, "DeviceBeamSearch: 1..16 beams"
        assert 1 <= int(num_return) <= K, "num_return_sequences has to be smaller or equal to num_beams"
        assert int(max_new_tokens) >= 1
        self.B, self.K, self.R, self.max_new, self.L = B, K, B * K, int(max_new_tokens), int(max_new_tokens) + 1
        self.min_length, self.length_penalty, self.repetition_penalty = int(min_length), float(length_penalty), float(repetition_penalty)
        self.eos_id, self.pad_id, self.start_id, self.num_return = int(eos_id), int(pad_id), int(start_id), int(num_return)
        self.poll_lag = int(poll_lag)
        self.device = torch.device(device if device is not None else "cuda")
        self._buf = buf
        R, L = self.R, self.L
        i32, f32 = torch.int32, torch.float32
        # ONE int32 and ONE fp32 block, so that a reset is two fills
        n_int = [("seq", 2 * R * L), ("parents", R), ("tokens", R), ("pool_len", R), ("pool_seq", R * L), ("pool_n", B), ("done", B),
                 ("done_count", 1), ("cand_index", 2 * R), ("out", B * self.num_return * (L + 2))]
        n_f32 = [("scores", R), ("pool_score", R), ("cand_score", 2 * R)]
        self._ints = self._alloc("bs_ints", sum(n for _, n in n_int), i32)
        self._f32s = self._alloc("bs_f32s", sum(n for _, n in n_f32), f32)
        for block, parts in ((self._ints, n_int), (self._f32s, n_f32)):
            off = 0
            for name, n in parts:
                setattr(self, "_" + name, block[off:off + n])
                off += n
        self._seq = self._seq.view(2, R, L)
        self._pool_seq = self._pool_seq.view(B, K, L)
        self._out = self._out.view(B, self.num_return, L + 2)
        self._identity = torch.arange(R, dtype=i32, device=self.device)
        self._ws = None
        # early stop without blocking: the done counter of every step lands in a pinned slot of its own, behind an event
        self._slots = torch.full((self.max_new,), -1, dtype=i32).pin_memory()
        self._events = [torch.cuda.Event() for _ in range(self.max_new)]
        self.reset()

    def _alloc(self, name, n, dtype):
        if self._buf is not None:
            return self._buf(name, (n,), dtype)
        return torch.zeros(n, dtype=dtype, device=self.device)

    def reset(self):
        """back to the state before the first step (start token, beam 0 at score 0 and the others at -1e9, empty pools).  Only enqueues."""
        self._ints.zero_()
        self._f32s.zero_()
        if self.start_id != 0:
            self._seq[0, :, 0].fill_(self.start_id)
            self._tokens.fill_(self.start_id)
        if self.K > 1:
            self._scores.view(self.B, self.K)[:, 1:].fill_(-1e9)
        self._parents.copy_(self._identity)
        self._slots.fill_(-1)
        self.cur_len, self.steps, self._recorded, self._finalized, self.host_seconds = 1, 0, 0, False, 0.0

    # the decoder's inputs for the next step
    @property
    def tokens(self) -> torch.Tensor:
        return self._tokens

    @property
    def parents(self) -> torch.Tensor:
        return self._parents

    @property
    def sequences(self) -> torch.Tensor:
        """int32 [B * K, cur_len] view of the running sequences (start token first)"""
        return self._seq[self.steps & 1][:, :self.cur_len]

    def step(self, logits_dev: torch.Tensor):
        """raw fp32 next-token logits [B * K, V] of the current rows -> new beams; launches only"""
        import time
        t0 = time.perf_counter()
        ops = self._ops
        assert not self._finalized and self.steps < self.max_new, "DeviceBeamSearch.step: past max_new_tokens (or after finalize)"
        R, V = logits_dev.shape
        assert R == self.R
        if self._ws is None or self._ws.numel() < ops.beam_topk_workspace_bytes(R, self.K, V):
            self._ws = self._alloc("bs_ws", ops.beam_topk_workspace_bytes(R, self.K, V), torch.uint8)
        src, dst = self._seq[self.steps & 1], self._seq[(self.steps + 1) & 1]
        ops.beam_topk(logits_dev, self._scores, src, self.cur_len, self.K, self._cand_score, self._cand_index, self._ws, min_length=self.min_length,
                      eos_id=self.eos_id, repetition_penalty=self.repetition_penalty)
        ops.beam_advance(self._cand_score, self._cand_index, src, dst, self._scores, self._parents, self._tokens, self._pool_score, self._pool_len,
                         self._pool_seq, self._pool_n, self._done, self._done_count, self.B, self.K, V, self.cur_len,
                         float(self.cur_len) ** self.length_penalty, eos_id=self.eos_id, pad_id=self.pad_id)
        self.steps += 1
        self.cur_len += 1
        self.host_seconds += time.perf_counter() - t0

    def done_count_async(self):
        """enqueue the copy of the done counter after the last step into that step's pinned slot, and record the step's event"""
        i = self.steps - 1
        assert i >= 0 and self._recorded == i, "done_count_async: once after every step"
        self._slots[i:i + 1].copy_(self._done_count, non_blocking=True)
        self._events[i].record()
        self._recorded = i + 1

    def finished(self) -> bool:
        """True when the step ``poll_lag`` before the next one is known to have left every clip done (event QUERIED, never waited for)"""
        i = self.steps - self.poll_lag
        if i < 0 or i >= self._recorded or not self._events[i].query():
            return False
        return int(self._slots[i]) == self.B

    def steps_after_done(self) -> int:
        """after finalize: steps that were enqueued although every clip was already done (the price of not waiting)"""
        assert self._finalized
        for i in range(self._recorded):
            if int(self._slots[i]) == self.B:
                return self.steps - (i + 1)
        return 0

    def finalize(self) -> List[torch.Tensor]:
        import time
        t0 = time.perf_counter()
        assert not self._finalized and self.steps >= 1
        self._ops.beam_finalize(self._seq[self.steps & 1], self._scores, self._pool_score, self._pool_len, self._pool_seq, self._pool_n, self._done,
                                self.B, self.K, self.cur_len, float(self.cur_len - 1) ** self.length_penalty, self.num_return, self._out)
        self._finalized = True
        self.host_seconds += time.perf_counter() - t0
        out = self._out.cpu()                                    # the one blocking transfer: everything enqueued has run after it
        t0 = time.perf_counter()
        self.final_scores = out[:, :, 1].contiguous().view(torch.float32)
        hyps = [out[b, r, 2:2 + int(out[b, r, 0])].to(torch.long) for b in range(self.B) for r in range(self.num_return)]
        self.host_seconds += time.perf_counter() - t0
        return hyps


class DeviceSampleSearch:
    """``sample_search`` with its whole state in device memory (csrc/search.hip): the warp of the raw logits, the top-k selection, the
    top-p cut, the draw and the row bookkeeping run as HIP kernels, so a decoding loop never waits for the host:

        search = DeviceSampleSearch(B, num_return, max_new, ..., seed=seed)
        for _ in range(max_new):
            if search.finished():                       # polls an event, never waits
                break
            logits = decoder(search.tokens)             # device int32 [R]: newest token of every row (rows never re-order)
            search.step(logits)                         # RAW fp32 logits [R, V]
            search.done_count_async()
        seqs = search.finalize()                        # the one blocking transfer

    The constructor mirrors ``sample_search``; ``finalize`` returns what it returns (R = batch * num_return sequences, item-major, start
    token first, each trimmed after its first EOS).  greedy=True is HF's greedy decoding on penalised raw logits (no temperature, cut
    or draw).  Decisions (include/mrblip_hip.h, mrblip_sample_advance): the k = min(top_k, V) best warped logits, higher first, EQUAL
    logits by lower token id — HF's top-k keeps every tie with the k-th logit, the device keeps exactly k — then softmax at the
    temperature, HF's top-p cut and one draw per row in fp64.  The draws come from a counter hash of (row, step, seed), or from
    ``uniforms`` (fp32 [max_new_tokens, R] on the device, in [0, 1)) when the caller has a generator of its own.

    State: ONE int32 block — seq [R, L] (L = max_new + 1, start token first), tokens [R], unfinished [R], length [R] (position after the
    row's first EOS, 0 while it has none), done_count [1], cand_index [R, 64], cand_score [R, 64] (fp32 bits) — taken from ``buf`` (a
    named-workspace allocator such as ``Engine.buf``) when given; a reset is one fill plus setting the unfinished flags."""

    def __init__(self, batch: int, num_return: int, max_new_tokens: int, min_length: int = 1, top_p: float = 0.9, temperature: float = 1.0,
                 repetition_penalty: float = 1.0, eos_id: int = 1, pad_id: int = 0, start_id: int = 0, greedy: bool = False, top_k: int = 50,
                 seed: int = 0, device=None, buf=None, poll_lag: int = 2, uniforms: Optional[torch.Tensor] = None):
        from mrblip import ops
        self._ops = ops
        R = int(batch) * max(1, int(num_return))
        assert 1 <= R <= ops.SAMPLE_MAX_ROWS, f"DeviceSampleSearch: 1..{ops.SAMPLE_MAX_ROWS} rows"
        assert 1 <= int(top_k) <= ops.SAMPLE_MAX_K, f"DeviceSampleSearch: top_k 1..{ops.SAMPLE_MAX_K} (0, HF's 'no top-k', keeps the host path)"
        assert int(max_new_tokens) >= 1 and float(temperature) > 0 and float(top_p) > 0
        self.B, self.R, self.max_new, self.L = int(batch), R, int(max_new_tokens), int(max_new_tokens) + 1
        self.min_length, self.top_p, self.temperature = int(min_length), float(top_p), float(temperature)
        self.repetition_penalty, self.greedy = float(repetition_penalty), bool(greedy)
        self.top_k = 1 if self.greedy else int(top_k)            # (greedy: rank 0 is all the step needs)
        self.eos_id, self.pad_id, self.start_id = int(eos_id), int(pad_id), int(start_id)
        self.poll_lag, self.seed, self.uniforms = int(poll_lag), int(seed) & 0xFFFFFFFF, uniforms
        self.device = torch.device(device if device is not None else "cuda")
        self._buf = buf
        L, NK = self.L, ops.SAMPLE_MAX_K
        parts = [("seq", R * L), ("tokens", R), ("unfinished", R), ("length", R), ("done_count", 1), ("cand_index", R * NK), ("cand_score", R * NK)]
        self._ints = self._alloc("ss_ints", sum(n for _, n in parts), torch.int32)
        off = 0
        for name, n in parts:
            setattr(self, "_" + name, self._ints[off:off + n])
            off += n
        self._n_out = R * L + 3 * R                              # seq, tokens, unfinished, length: what finalize brings back
        self._seq = self._seq.view(R, L)
        self._cand_index = self._cand_index.view(R, NK)
        self._cand_score = self._cand_score.view(torch.float32).view(R, NK)
        self._ws = None
        # early stop without blocking: the done counter of every step lands in a pinned slot of its own, behind an event
        self._slots = torch.full((self.max_new,), -1, dtype=torch.int32).pin_memory()
        self._events = [torch.cuda.Event() for _ in range(self.max_new)]
        self.reset()

    def _alloc(self, name, n, dtype):
        if self._buf is not None:
            return self._buf(name, (n,), dtype)
        return torch.zeros(n, dtype=dtype, device=self.device)

    def reset(self, seed: Optional[int] = None):
        """back to the state before the first step (start token, every row unfinished); ``seed`` re-keys the draws.  Only enqueues."""
        if seed is not None:
            self.seed = int(seed) & 0xFFFFFFFF
        self._ints.zero_()
        self._unfinished.fill_(1)
        if self.start_id != 0:
            self._seq[:, 0].fill_(self.start_id)
            self._tokens.fill_(self.start_id)
        self._slots.fill_(-1)
        self.cur_len, self.steps, self._recorded, self._finalized, self.host_seconds = 1, 0, 0, False, 0.0

    @property
    def tokens(self) -> torch.Tensor:
        """the decoder's input for the next step: int32 [R] on the device"""
        return self._tokens

    @property
    def sequences(self) -> torch.Tensor:
        """int32 [R, cur_len] view of the running sequences (start token first)"""
        return self._seq[:, :self.cur_len]

    def step(self, logits_dev: torch.Tensor):
        """raw fp32 next-token logits [R, V] of the current rows -> one new token per row; launches only"""
        import time
        t0 = time.perf_counter()
        ops = self._ops
        assert not self._finalized and self.steps < self.max_new, "DeviceSampleSearch.step: past max_new_tokens (or after finalize)"
        R, V = logits_dev.shape
        assert R == self.R
        need = ops.sample_topk_workspace_bytes(R, self.top_k, V)
        if self._ws is None or self._ws.numel() < need:
            self._ws = self._alloc("ss_ws", need, torch.uint8)
        ops.sample_topk(logits_dev, self._seq, self.cur_len, self.top_k, self._cand_score, self._cand_index, self._ws, min_length=self.min_length,
                        eos_id=self.eos_id, repetition_penalty=self.repetition_penalty)
        ops.sample_advance(self._cand_score, self._cand_index, self._seq, self._tokens, self._unfinished, self._length, self._done_count, V,
                           self.top_k, self.cur_len, top_p=self.top_p, temperature=self.temperature, greedy=self.greedy, uniforms=self.uniforms,
                           seed=self.seed, eos_id=self.eos_id, pad_id=self.pad_id)
        self.steps += 1
        self.cur_len += 1
        self.host_seconds += time.perf_counter() - t0

    def done_count_async(self):
        """enqueue the copy of the done counter after the last step into that step's pinned slot, and record the step's event"""
        i = self.steps - 1
        assert i >= 0 and self._recorded == i, "done_count_async: once after every step"
        self._slots[i:i + 1].copy_(self._done_count, non_blocking=True)
        self._events[i].record()
        self._recorded = i + 1

    def finished(self) -> bool:
        """True when the step ``poll_lag`` before the next one is known to have left every row finished (event QUERIED, never waited for)"""
        i = self.steps - self.poll_lag
        if i < 0 or i >= self._recorded or not self._events[i].query():
            return False
        return int(self._slots[i]) == self.R

    def steps_after_done(self) -> int:
        """after finalize: steps that were enqueued although every row was already finished (the price of not waiting)"""
        assert self._finalized
        for i in range(self._recorded):
            if int(self._slots[i]) == self.R:
                return self.steps - (i + 1)
        return 0

    def finalize(self) -> List[torch.Tensor]:
        assert not self._finalized and self.steps >= 1
        self._finalized = True
        out = self._ints[:self._n_out].cpu()                     # the one blocking transfer: everything enqueued has run after it
        import time
        t0 = time.perf_counter()
        R, L = self.R, self.L
        seq, length = out[:R * L].view(R, L), out[R * L + 2 * R:].tolist()
        # surplus steps after a row's EOS only appended pads: trimming removes them; a row without EOS keeps all cur_len tokens
        seqs = [seq[r, :length[r] if length[r] > 0 else self.cur_len].to(torch.long) for r in range(R)]
        self.host_seconds += time.perf_counter() - t0
        return seqs
