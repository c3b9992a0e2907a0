"""The device-resident sampler (csrc/search.hip, mrblip.search.DeviceSampleSearch, BLIP2_MR.generate_device_sample) against a numpy
restatement of its decision rules and against the host sampler it replaces.

REFERENCE (this file).  The warp of the raw logits runs in float32, like the kernel's; the ranking is np.lexsort by (-score, token id);
everything after it is float64 with sequential np.cumsum, exactly as include/mrblip_hip.h states it for mrblip_sample_advance.  Both sides
decide in fp64, so they differ by about 1e-15 relative; the reference asserts for EVERY case that no decision is nearer than that by a wide
margin — every |Z - P_{i-1} - (1 - top_p) Z| / Z and every |P_i - target| / P_{n-1} is at least 1e-9, and the warped logits of rank k - 1
and rank k are at least 1e-6 apart — and inside these margins the device has to match EXACTLY.  No case is excused: the seeds below are
fixed so that the asserts hold.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mr-blip_amd"))

EOS, PAD, START = 1, 0, 0
NK = 64                      # row stride of the candidate buffers
SITE = 0x53414D50            # csrc/common.h MRB_SITE_SAMPLE
DECISION_MARGIN, RANK_GAP = 1e-9, 1e-6


# ------------------------------------------------------------------------------------------------ the reference
def mrb_hash(idx, seed, site):
    """csrc/common.h mrb_hash in Python integers"""
    m = 0xFFFFFFFF
    h = (((idx ^ seed) & m) * 0x9E3779B1 + site * 0x85EBCA77) & m
    h ^= h >> 15
    h = (h * 0xC2B2AE3D) & m
    return h ^ (h >> 13)


def hash_uniform(r, t, seed):
    return (mrb_hash(r * 256 + t, seed, SITE) >> 8) * 2.0 ** -24


def ref_topk(logits, seqs, cur_len, top_k, min_length, pen, tag=""):
    """logits float32 [R, V], seqs int [R, >= cur_len] -> (scores float32 [R, k], ids int64 [R, k]): the k best warped logits, best first"""
    R, V = logits.shape
    k = min(top_k, V)
    x = logits.astype(np.float32).copy()
    p32 = np.float32(pen)
    if pen != 1.0:
        for r in range(R):
            ids = np.unique(seqs[r, :cur_len])
            v = x[r, ids]
            x[r, ids] = np.where(v < 0, v * p32, v / p32).astype(np.float32)
    if cur_len < min_length:
        x[:, EOS] = -np.inf
    sc, ix = np.empty((R, k), np.float32), np.empty((R, k), np.int64)
    for r in range(R):
        order = np.lexsort((np.arange(V), -x[r]))            # by -score, equal scores by token id
        sc[r], ix[r] = x[r, order[:k]], order[:k]
        if k < V:
            gap = float(x[r, order[k - 1]]) - float(x[r, order[k]])
            assert gap >= RANK_GAP, f"{tag} row {r}: ranks {k - 1} / {k} are {gap:.3g} apart: pick another seed"
    return sc, ix


def ref_decide(cs, temperature, top_p, u, tag=""):
    """cs float32 [k] (descending) -> (rank drawn, n kept), fp64, with the margin asserts"""
    T, tp = float(np.float32(temperature)), float(np.float32(top_p))
    w = cs.astype(np.float64) / T
    with np.errstate(invalid="ignore"):
        p = np.exp(w - w[0])
    P = np.cumsum(p)                                          # sequential, in rank order
    Z, k = P[-1], len(cs)
    if tp >= 1.0:
        assert all(v == 0.0 or v > 1e-300 for v in p), f"{tag}: a probability in the denormal range decides the kept set"
        n = 1
        while n < k and p[n] > 0.0:
            n += 1
    else:
        thr = (1.0 - tp) * Z
        rest = Z - P[:-1]                                     # rest[i - 1] = Z - P_{i-1}: the mass of ranks >= i
        margin = np.abs(rest - thr) / Z
        assert k == 1 or margin.min() >= DECISION_MARGIN, f"{tag}: top-p cut decided by {margin.min():.3g}: pick another seed"
        n = 1
        while n < k and rest[n - 1] > thr:
            n += 1
    target = float(u) * P[n - 1]
    margin = np.abs(P[:n] - target) / P[n - 1]
    assert margin.min() >= DECISION_MARGIN, f"{tag}: draw decided by {margin.min():.3g}: pick another seed"
    hit = np.nonzero(P[:n] > target)[0]
    return (int(hit[0]) if len(hit) else n - 1), n


class RefState:
    """sample_search's rows in numpy: seq [R, L], unfinished, length, done_count"""

    def __init__(self, R, L):
        self.seq = np.zeros((R, L), np.int64)
        self.seq[:, 0] = START
        self.unfinished, self.length, self.done_count, self.cur_len = np.ones(R, np.int64), np.zeros(R, np.int64), 0, 1

    def advance(self, sc, ix, temperature, top_p, u, greedy=False, tag=""):
        R = sc.shape[0]
        tokens = np.zeros(R, np.int64)
        for r in range(R):
            rank = 0
            if not greedy and sc.shape[1] > 1:
                rank, _ = ref_decide(sc[r], temperature, top_p, u[r], f"{tag} row {r}")
            tok = int(ix[r, rank]) if self.unfinished[r] else PAD
            tokens[r] = self.seq[r, self.cur_len] = tok
            if self.unfinished[r] and tok == EOS:
                self.unfinished[r], self.length[r] = 0, self.cur_len + 1
        self.done_count = int((self.unfinished == 0).sum())
        self.cur_len += 1
        return tokens


# ------------------------------------------------------------------------------------------------ kernel level
SETTINGS = [(50, 0.9, 1.0), (50, 0.9, 0.7), (8, 0.5, 1.3), (64, 1.0, 1.0), (1, 0.9, 1.0), (50, 1e-6, 1.0)]
VS, RS, PENS = (40, 2048, 2085, 32128), (1, 3, 20), (1.0, 1.3)
CUR_LEN = 6
SEED_OVERRIDES = {}


def _case_seed(V, R, si, pen):
    key = (V, R, si, pen)
    return SEED_OVERRIDES.get(key, 9000 + 97 * VS.index(V) + 31 * RS.index(R) + 7 * si + (3 if pen != 1.0 else 0))


def _kernel_case(V, R, si, pen):
    """logits N(0, 3); with a penalty, every row's sequence repeats tokens of different chunks whose logits have both signs"""
    g = torch.Generator().manual_seed(_case_seed(V, R, si, pen))
    logits = (torch.randn(R, V, generator=g) * 3.0).numpy()
    seqs = torch.randint(2, V, (R, 8), generator=g).numpy()
    seqs[:, 0] = START
    if pen != 1.0:
        far = [t for t in (5, 17, 2050, 30000) if t < V]       # chunk 0, chunk 0, chunk 1, chunk 14
        for r in range(R):
            a, b = far[-1], far[0] if len(far) < 3 else far[-2]
            seqs[r, 1], seqs[r, 2], seqs[r, 3], seqs[r, 4] = a, b, a, b     # repeated
            logits[r, a], logits[r, b] = 14.0 + 0.125 * r, -1.5 - 0.125 * r   # 14 / 1.3 stays among the best; the negative one grows
            logits[r, START] = abs(logits[r, START]) + 13.0                 # the start token is in the set as well
    u = torch.rand(CUR_LEN, R, generator=g).numpy().astype(np.float32)
    return logits.astype(np.float32), seqs, u


def _run_topk(logits, seqs, cur_len, top_k, min_length=1, pen=1.0, ldl=None):
    """-> (cand_score, cand_index) device tensors [R, 64] of two runs, asserted equal in their bits"""
    from mrblip import ops
    R, V = logits.shape
    dev = "cuda"
    if ldl is None:
        lg = torch.from_numpy(logits).to(dev)
    else:
        full = torch.full((R, ldl), 99.0, device=dev)           # (what lies between the rows would win every selection)
        full[:, :V] = torch.from_numpy(logits).to(dev)
        lg = full[:, :V]
        assert lg.stride(0) == ldl and not lg.is_contiguous()
    sq = torch.from_numpy(seqs).to(torch.int32).to(dev)
    ws = torch.empty(ops.sample_topk_workspace_bytes(R, top_k, V), dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        cs = torch.full((R, NK), float("nan"), device=dev)
        ci = torch.full((R, NK), -7, dtype=torch.int32, device=dev)
        ws.random_(0, 256)                                      # the scratch carries no state between calls
        ops.sample_topk(lg, sq, cur_len, top_k, cs, ci, ws, min_length=min_length, eos_id=EOS, repetition_penalty=pen)
        runs.append((cs, ci))
    (cs, ci), (cs2, ci2) = runs
    assert torch.equal(ci, ci2) and torch.equal(cs.view(torch.int32), cs2.view(torch.int32)), "two runs differ in their bits"
    return cs, ci


def _assert_topk(cs, ci, sc, ix):
    k = sc.shape[1]
    got_s, got_i = cs.cpu().numpy(), ci.cpu().numpy()
    assert np.array_equal(got_i[:, :k], ix), (got_i[:, :k].tolist(), ix.tolist())
    assert np.array_equal(got_s[:, :k].view(np.int32), sc.view(np.int32)), "scores differ in their bits"
    assert np.all(np.isneginf(got_s[:, k:])) and np.all(got_i[:, k:] == -1)


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("si", range(len(SETTINGS)))
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("V", VS)
def test_sample_topk_and_one_step_equal_the_reference(V, R, si, pen):
    from mrblip import ops
    top_k, top_p, T = SETTINGS[si]
    tag = f"V={V} R={R} {SETTINGS[si]} pen={pen}"
    logits, seqs, u = _kernel_case(V, R, si, pen)
    sc, ix = ref_topk(logits, seqs, CUR_LEN, top_k, 1, pen, tag)
    ref = RefState(R, 8)
    ref.seq[:, :CUR_LEN], ref.cur_len = seqs[:, :CUR_LEN], CUR_LEN
    done_row = R - 1 if R > 1 else None                          # one row has finished before: it emits the pad id
    if done_row is not None:
        ref.unfinished[done_row] = 0
    want = ref.advance(sc, ix, T, top_p, u[CUR_LEN - 1], tag=tag)
    kept = [ref_decide(sc[r], T, top_p, u[CUR_LEN - 1, r])[1] if top_k > 1 else 1 for r in range(R)]
    if si == 5:
        assert kept == [1] * R
    if si == 3 and V == 40:
        assert sc.shape[1] == 40                                 # V < top_k: every entry is ranked

    cs, ci = _run_topk(logits, seqs, CUR_LEN, top_k, pen=pen)
    _assert_topk(cs, ci, sc, ix)
    dev = "cuda"
    seq = torch.from_numpy(ref.seq).to(torch.int32).to(dev)
    seq[:, CUR_LEN] = -3
    tokens = torch.full((R,), -3, dtype=torch.int32, device=dev)
    unfinished = torch.ones(R, dtype=torch.int32, device=dev)
    if done_row is not None:
        unfinished[done_row] = 0
    length, done_count = torch.zeros(R, dtype=torch.int32, device=dev), torch.full((1,), -3, dtype=torch.int32, device=dev)
    ops.sample_advance(cs, ci, seq, tokens, unfinished, length, done_count, V, top_k, CUR_LEN, top_p=top_p, temperature=T,
                       uniforms=torch.from_numpy(u).to(dev), eos_id=EOS, pad_id=PAD)
    print(f"{tag}: kept {min(kept)}..{max(kept)} of {sc.shape[1]} candidates")
    assert tokens.cpu().tolist() == want.tolist()
    assert seq.cpu().tolist() == ref.seq.tolist()
    assert unfinished.cpu().tolist() == ref.unfinished.tolist() and length.cpu().tolist() == ref.length.tolist()
    assert int(done_count.cpu()) == ref.done_count


@pytest.mark.parametrize("V", [2085, 32128])
def test_sample_topk_bans_an_eos_that_would_be_rank_0(V):
    g = torch.Generator().manual_seed(41 + V)
    logits = (torch.randn(3, V, generator=g) * 3.0).numpy().astype(np.float32)
    logits[:, EOS] = 40.0
    seqs = np.zeros((3, 8), np.int64)
    sc, ix = ref_topk(logits, seqs, 2, 50, 3, 1.0)
    assert not (ix == EOS).any() and (ref_topk(logits, seqs, 3, 50, 3, 1.0)[1][:, 0] == EOS).all()
    _assert_topk(*_run_topk(logits, seqs, 2, 50, min_length=3), sc, ix)
    sc, ix = ref_topk(logits, seqs, 3, 50, 3, 1.0)              # cur_len == min_length: the ban is over
    _assert_topk(*_run_topk(logits, seqs, 3, 50, min_length=3), sc, ix)


def test_sample_topk_ranks_an_exact_tie_by_lower_token_id():
    """two equal logits at ranks 0 and 1, in one chunk and in different chunks; with V = 40 < top_k and the EOS banned the one -inf
    entry comes last, and a row of which only 3 entries are finite carries its -inf tail in index order"""
    V = 2085
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(3, V, generator=g) * 3.0).numpy().astype(np.float32)
    logits[0, [700, 90]] = 30.0
    logits[1, [2070, 12]] = 30.0
    logits[2, [2049, 2050]] = 30.0
    seqs = np.zeros((3, 8), np.int64)
    sc, ix = ref_topk(logits, seqs, 1, 50, 1, 1.0)
    assert ix[:, :2].tolist() == [[90, 700], [12, 2070], [2049, 2050]]
    _assert_topk(*_run_topk(logits, seqs, 1, 50), sc, ix)
    small = (torch.randn(2, 40, generator=g) * 3.0).numpy().astype(np.float32)
    small[1] = -np.inf
    small[1, [30, 4, 17]] = [1.0, 2.0, 2.0]
    sc, ix = ref_topk(small, seqs[:2], 1, 50, 2, 1.0)
    assert ix[0, -1] == EOS and ix[1, :3].tolist() == [4, 17, 30] and ix[1, 3:].tolist() == [v for v in range(40) if v not in (4, 17, 30)]
    _assert_topk(*_run_topk(small, seqs[:2], 1, 50, min_length=2), sc, ix)


def test_sample_topk_reads_rows_with_a_leading_dimension():
    logits, seqs, _ = _kernel_case(2085, 3, 0, 1.3)
    sc, ix = ref_topk(logits, seqs, CUR_LEN, 50, 1, 1.3)
    _assert_topk(*_run_topk(logits, seqs, CUR_LEN, 50, pen=1.3, ldl=2085 + 27), sc, ix)


# ------------------------------------------------------------------------------------------------ chained steps
CHAIN = dict(R=3, V=2085, steps=6, top_k=50, top_p=0.9, T=0.7, pen=1.2, min_length=2)


def _chain_logits(seed):
    g = torch.Generator().manual_seed(seed)
    c = CHAIN
    lg = (torch.randn(c["steps"], c["R"], c["V"], generator=g) * 3.0).numpy().astype(np.float32)
    lg[2, 1, EOS] = 60.0                                        # row 1 draws EOS at step 2 (its share of the mass is 1 - 1e-20) and pads afterwards
    return lg, torch.rand(c["steps"], c["R"], generator=g).numpy().astype(np.float32)


def _chain_reference(lg, uniform_of):
    c = CHAIN
    ref = RefState(c["R"], c["steps"] + 1)
    hist = []
    for t in range(c["steps"]):
        sc, ix = ref_topk(lg[t], ref.seq, ref.cur_len, c["top_k"], c["min_length"], c["pen"], f"chain step {t}")
        u = [uniform_of(r, t) for r in range(c["R"])]
        tok = ref.advance(sc, ix, c["T"], c["top_p"], u, tag=f"chain step {t}")
        hist.append((tok.tolist(), ref.seq.copy(), ref.unfinished.tolist(), ref.length.tolist(), ref.done_count))
    return ref, hist


def _chain_device(lg, uniforms, seed):
    """DeviceSampleSearch fed the chain's logits; after every step its state as the reference records it"""
    from mrblip.search import DeviceSampleSearch
    c = CHAIN
    search = DeviceSampleSearch(1, c["R"], c["steps"], min_length=c["min_length"], top_p=c["top_p"], temperature=c["T"], repetition_penalty=c["pen"],
                                eos_id=EOS, pad_id=PAD, start_id=START, top_k=c["top_k"], seed=seed, device="cuda",
                                uniforms=None if uniforms is None else torch.from_numpy(uniforms).cuda())
    hist = []
    for t in range(c["steps"]):
        search.step(torch.from_numpy(lg[t]).cuda())
        search.done_count_async()
        hist.append((search.tokens.cpu().tolist(), search._seq.cpu().numpy().astype(np.int64), search._unfinished.cpu().tolist(),
                     search._length.cpu().tolist(), int(search._done_count.cpu())))
    return search, hist


def _assert_chain(got, want):
    for t, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], (t, "tokens", g[0], w[0])
        assert np.array_equal(g[1], w[1]), (t, "sequences", g[1].tolist(), w[1].tolist())
        assert g[2] == w[2] and g[3] == w[3] and g[4] == w[4], (t, "unfinished / length / done_count", g[2:], w[2:])


def _trimmed(ref):
    return [ref.seq[r, :ref.length[r] if ref.length[r] > 0 else ref.cur_len].tolist() for r in range(ref.seq.shape[0])]


def test_six_chained_steps_with_explicit_uniforms_equal_the_reference():
    lg, u = _chain_logits(77)
    ref, want = _chain_reference(lg, lambda r, t: u[t, r])
    assert want[2][0][1] == EOS and [w[0][1] for w in want[3:]] == [PAD] * 3 and ref.length[1] == 4, "row 1 has to finish at step 2"
    assert want[-1][4] < CHAIN["R"], "the other rows keep running"
    search, got = _chain_device(lg, u, seed=0)
    _assert_chain(got, want)
    assert not search.finished()
    assert [s.tolist() for s in search.finalize()] == _trimmed(ref)


def test_six_chained_steps_with_the_built_in_draws_equal_the_reference():
    lg, _ = _chain_logits(78)
    seed = 0xC0FFEE11
    ref, want = _chain_reference(lg, lambda r, t: hash_uniform(r, t, seed))
    assert want[2][0][1] == EOS and ref.length[1] == 4
    search, got = _chain_device(lg, None, seed)
    _assert_chain(got, want)
    first = [s.tolist() for s in search.finalize()]
    assert first == _trimmed(ref)
    search.reset()                                              # same seed: the same bits
    for t in range(CHAIN["steps"]):
        search.step(torch.from_numpy(lg[t]).cuda())
        search.done_count_async()
    assert np.array_equal(search._seq.cpu().numpy(), got[-1][1])
    assert [s.tolist() for s in search.finalize()] == first
    search.reset(seed=seed + 1)                                 # another seed: other draws
    for t in range(CHAIN["steps"]):
        search.step(torch.from_numpy(lg[t]).cuda())
        search.done_count_async()
    assert not np.array_equal(search._seq.cpu().numpy(), got[-1][1])


def test_greedy_mode_takes_rank_0_and_all_rows_finishing_is_polled():
    """greedy: the argmax of the penalised logits whatever temperature / top_p say; when every row has drawn EOS the polled counter
    equals R, and surplus steps only append pads that finalize trims"""
    from mrblip.search import DeviceSampleSearch
    R, V, steps = 3, 2085, 5
    g = torch.Generator().manual_seed(3)
    lg = (torch.randn(steps, R, V, generator=g) * 3.0).numpy().astype(np.float32)
    lg[1, :, EOS] = 60.0
    ref = RefState(R, steps + 1)
    for t in range(steps):
        sc, ix = ref_topk(lg[t], ref.seq, ref.cur_len, 1, 1, 1.5)
        ref.advance(sc, ix, 1.0, 0.9, None, greedy=True)
    assert ref.length.tolist() == [3] * R
    search = DeviceSampleSearch(R, 1, steps, min_length=1, top_p=0.3, temperature=0.5, repetition_penalty=1.5, eos_id=EOS, pad_id=PAD, start_id=START,
                                greedy=True, device="cuda")
    for t in range(steps):
        search.step(torch.from_numpy(lg[t]).cuda())
        search.done_count_async()
    torch.cuda.synchronize()
    assert search.finished()
    assert search._seq.cpu().tolist() == ref.seq.tolist()
    assert [s.tolist() for s in search.finalize()] == _trimmed(ref) and search.steps_after_done() == steps - 2


# ------------------------------------------------------------------------------------------------ model level
def _tiny(mean=False):
    from test_beam_device_gpu import _tiny_model
    return _tiny_model(mean)


def _generate(model, samples, device, **kw):
    model.generate_device_sample = device
    try:
        out = model.generate(samples, **kw)
    finally:
        model.generate_device_sample = False
    return [s.tolist() for s in model.last_sequences], out, model.last_generate_stats


PEN_GREEDY = dict(num_beams=1, repetition_penalty=1.5, max_length=8, min_length=2)
NUCLEUS_0 = dict(use_nucleus_sampling=True, num_beams=1, top_p=1e-6, max_length=8, min_length=2)
NUCLEUS = dict(use_nucleus_sampling=True, num_beams=1, top_p=0.9, temperature=0.7, repetition_penalty=1.2, num_captions=3, max_length=8, min_length=2)


@pytest.mark.parametrize("fused", [False, True])
def test_penalised_greedy_on_the_device_equals_the_host_route(fused):
    """both routes run the same decoder kernels on the same tokens, so their logits are the same bits and the sequences have to be equal
    token for token whatever the margins of the decode are"""
    model, samples = _tiny()
    model.generate_fused_decode = fused
    try:
        host, out_h, stats_h = _generate(model, samples, False, **PEN_GREEDY)
        assert stats_h is None
        dev, out_d, stats_d = _generate(model, samples, True, **PEN_GREEDY)
    finally:
        model.generate_fused_decode = False
    assert stats_d is not None and stats_d["steps"] >= 1 and stats_d["search_host_s"] > 0, "the device route was not taken"
    assert dev == host and out_d["raw_prediction"] == out_h["raw_prediction"], (dev, host)


def test_a_vanishing_nucleus_on_the_device_reproduces_the_greedy_decode():
    model, samples = _tiny()
    model.generate(samples, num_beams=1, max_length=8, min_length=2)
    greedy = [s.tolist() for s in model.last_sequences]
    dev, _, stats = _generate(model, samples, True, **NUCLEUS_0)
    assert stats is not None and dev == greedy


def test_device_sampling_is_reproducible_seeded_and_stays_inside_the_kept_set():
    model, samples = _tiny()
    eng = model.engine
    B = samples["video"].shape[0]
    captured = []
    inner = eng.t5_decode_step

    def recording(state, tokens, parents, *a, **k):
        logits = inner(state, tokens, parents, *a, **k)
        captured.append(logits.float().cpu().numpy().copy())
        return logits

    runs = []
    for seed in (7, 7, 8):
        model.sampling_generator = torch.Generator().manual_seed(seed)
        del captured[:]
        eng.t5_decode_step = recording
        try:
            seqs, out, stats = _generate(model, samples, True, **NUCLEUS)
        finally:
            del eng.t5_decode_step                               # (the instance attribute: the class's method is back)
        assert stats is not None and len(captured) == stats["steps"]
        assert len(seqs) == B * 3 and len(out["prediction"]) == len(out["raw_prediction"]) == B * 3 and len(out["duration"]) == B
        runs.append((seqs, [c.copy() for c in captured]))
    model.sampling_generator = None
    assert runs[0][0] == runs[1][0], "the same seed has to give the same sequences"
    assert runs[0][0] != runs[2][0], "another seed has to give other sequences"
    assert len({tuple(s) for s in runs[0][0]}) > 1, "really sampling"
    for seqs, steps in (runs[0], runs[2]):
        for r, s in enumerate(seqs):
            assert s[0] == START
            for t in range(len(s) - 1):
                prefix = np.array([s[:t + 1]], np.int64)
                sc, ix = ref_topk(steps[t][r:r + 1], prefix, t + 1, 50, NUCLEUS["min_length"], NUCLEUS["repetition_penalty"], f"row {r} step {t}")
                _, n = ref_decide(sc[0], NUCLEUS["temperature"], NUCLEUS["top_p"], 0.5, f"row {r} step {t}")
                assert s[t + 1] in ix[0, :n].tolist(), (r, t, s, ix[0, :n].tolist())


@pytest.mark.parametrize("kw", [PEN_GREEDY, NUCLEUS_0, NUCLEUS], ids=["penalised_greedy", "nucleus_0", "nucleus"])
def test_with_the_switch_off_every_call_takes_the_host_route(kw):
    model, samples = _tiny()
    assert model.generate_device_sample is False
    model.generate_device_search = True                          # (the beam switch does not move sampling off the host either)
    try:
        model.sampling_generator = torch.Generator().manual_seed(7)
        model.generate(samples, **kw)
        first = [s.tolist() for s in model.last_sequences]
        assert model.last_generate_stats is None
        model.sampling_generator = torch.Generator().manual_seed(7)
        model.generate(samples, **kw)
        assert model.last_generate_stats is None and [s.tolist() for s in model.last_sequences] == first
    finally:
        model.generate_device_search = False
        model.sampling_generator = None


def test_early_stop_of_penalised_greedy_on_the_device_is_only_an_optimisation():
    """all max_length steps (polling off) give the polled run's sequences, and polling enqueues at most poll_lag = 2 steps more than the
    host route, which stops as soon as every row has drawn its EOS (EOS row of the LM head scaled by -4: the host route ends after 3
    of 24 steps)"""
    from test_beam_device_gpu import _tiny_model_eos
    kw = dict(PEN_GREEDY, max_length=24, min_length=1)
    model, samples = _tiny_model_eos(-4.0)
    host, out_h, _ = _generate(model, samples, False, **kw)
    steps_h = max(len(s) for s in host) - 1
    assert all(s[-1] == EOS for s in host) and steps_h < kw["max_length"], "the case has to finish early, or it shows nothing"
    polled, out_p, stats_p = _generate(model, samples, True, **kw)
    model.generate_poll_done = False
    try:
        full, out_f, stats_f = _generate(model, samples, True, **kw)
    finally:
        model.generate_poll_done = True
    print(f"early stop, penalised greedy: host {steps_h} steps, polled {stats_p}, unpolled {stats_f}")
    assert stats_f["steps"] == kw["max_length"] and stats_f["steps_after_done"] == kw["max_length"] - steps_h
    assert polled == full == host and out_p["raw_prediction"] == out_f["raw_prediction"] == out_h["raw_prediction"]
    assert stats_p["steps"] <= steps_h + 2 and stats_p["steps_after_done"] == stats_p["steps"] - steps_h


def test_early_stop_of_device_sampling_is_only_an_optimisation():
    """the same on the sampling route with 3 rows per clip.  (With top_p 0.9 the -4 fixture's six rows do not all draw an EOS within 24
    steps; a vanishing nucleus with the repetition penalty walks the penalised greedy path of the test above, which ends early.)"""
    from test_beam_device_gpu import _tiny_model_eos
    kw = dict(NUCLEUS_0, repetition_penalty=1.5, num_captions=3, max_length=24, min_length=1)
    model, samples = _tiny_model_eos(-4.0)
    B = samples["video"].shape[0]
    model.generate_poll_done = False
    try:
        full, out_f, stats_f = _generate(model, samples, True, **kw)
    finally:
        model.generate_poll_done = True
    needed = stats_f["steps"] - stats_f["steps_after_done"]
    assert stats_f["steps"] == kw["max_length"] and needed < kw["max_length"], "the case has to finish early, or it shows nothing"
    assert len(full) == B * 3 and all(s[-1] == EOS for s in full) and max(len(s) for s in full) - 1 == needed
    polled, out_p, stats_p = _generate(model, samples, True, **kw)
    print(f"early stop, sampling route: {needed} steps needed, polled {stats_p}, unpolled {stats_f}")
    assert polled == full and out_p["raw_prediction"] == out_f["raw_prediction"]
    assert stats_p["steps"] <= needed + 2 and stats_p["steps_after_done"] == stats_p["steps"] - needed
