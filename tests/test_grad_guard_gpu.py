"""The gradient guard on the GPU (csrc/optim.hip, mrblip/grad_guard.py): the fp64-accumulated global norm against an fp64
CPU reference, bit reproducibility, the non-finite skip, the device-side optimizer clock, the bias terms, clipping by global norm, and the
user-visible behaviour through FlatAdamW, MrBlipEngine.optimizer_step and the train loop.

Bounds.  Norm, clip and bias terms: 1 ulp of fp32 at the reference value — derived, not measured: the squares are exact in fp64, an fp64
sum of n terms errs by at most n * 2^-53 relative (< 2e-9 for every n here), pow / sqrt / the division in double err by a few 2^-53, so the
only visible rounding is the final cast to fp32 (which can land on the other neighbour when the exact value sits within 2e-9 of a tie).
AdamW results: the ``rel`` metric and the 1e-6 bound of the AdamW row of tests/test_kernels_gpu.py::test_cast_gelu_ce_adamw, against
torch.optim.AdamW in fp64 on the CPU.  The fused AdamW kernel takes beta1 / beta2 as fp32 arguments of the C ABI, so the reference is
given the betas the kernel is given — 0.9 and 0.999 rounded to fp32: with the unrounded doubles the kernel's 1 - fp32(0.999) alone is
1.3e-5 away from the reference's 1 - 0.999 in ``v``, which says nothing about the guard.
Nothing here provokes a fault: "guard word set" writes a 1 into a plain tensor, "poisoned" writes a NaN into a gradient."""
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 16384                                   # ops.GRAD_CHUNK
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))
NS = (0, 1, 3, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5, 2 ** 20 + 17)
NMAX = max(NS)
INF_BITS = 0x7F800000


def dev():
    return torch.device("cuda:0")


def rel(a, b):                              # tests/test_kernels_gpu.py
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def ulps(got, ref):
    """|got - ref| in units of the fp32 spacing at ref"""
    r = np.float32(ref)
    return float(abs(np.float64(np.float32(got)) - np.float64(r)) / np.float64(np.spacing(np.abs(r))))


def f32_of(word):
    return float(np.array([int(word) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])


def state_of(state):
    w = [int(x) & 0xFFFFFFFF for x in state.cpu().tolist()]
    return dict(skip=w[0], applied=w[1], skipped=w[2], nonfinite=w[3], norm=f32_of(w[4]), norm_bits=w[4], clip=f32_of(w[5]), consecutive=w[6],
                reserved=w[7])


def poisoned_slice(data, off):
    """data on the device at ``off`` floats past a 16-byte line, NaN in front of and behind it: a read outside [g, g + n) shows up as a
    non-finite count"""
    n = data.numel()
    buf = torch.full((4 + off + n + 8,), float("nan"), device=dev())
    buf[4 + off: 4 + off + n] = data.to(dev())
    g = buf[4 + off: 4 + off + n]
    assert n == 0 or g.data_ptr() % 16 == 4 * off
    return g


def prepare(g, state=None, lr=3e-4, gs=1.0, betas=(B1, B2), max_norm=0.0, guard=None):
    from mrblip import ops
    ws = torch.zeros(ops.grad_stats_workspace_bytes(g.numel()), dtype=torch.uint8, device=dev())
    state = torch.zeros(8, dtype=torch.int32, device=dev()) if state is None else state
    hin = torch.tensor([lr, gs], dtype=torch.float32, device=dev())
    hout = torch.full((4,), float("nan"), device=dev())
    ops.grad_sumsq(g, ws)
    ops.optim_prepare(ws, g.numel(), hin, state, hout, betas[0], betas[1], max_norm, guard=guard)
    return ws, state, hout


def guarded_step(p, g, m, v, nd, state, lr=3e-4, gs=1.0, betas=(B1, B2), eps=1e-8, wd=0.05, max_norm=0.0, guard=None):
    """the sequence FlatAdamW and the engine run: partials over the WHOLE buffer, prepare, two guarded AdamW launches on the verdict"""
    from mrblip import ops
    _, state, hout = prepare(g, state, lr, gs, betas, max_norm, guard)
    ops.adamw(p[:nd], g[:nd], m[:nd], v[:nd], hout, betas[0], betas[1], eps, wd, guard=state[0:1])
    ops.adamw(p[nd:], g[nd:], m[nd:], v[nd:], hout, betas[0], betas[1], eps, 0.0, guard=state[0:1])
    return hout


# ------------------------------------------------------------------------------------------------------------ 1. norm against fp64
_values, _refs = {}, {}


def values(kind):
    if kind not in _values:
        gen = torch.Generator().manual_seed(1234)
        if kind == "normal":
            x = torch.randn(NMAX, generator=gen)
        elif kind == "zeros":
            x = torch.zeros(NMAX)
        elif kind == "tiny":                # squares underflow fp32: an fp32 accumulator returns 0
            x = torch.full((NMAX,), 1e-30)
        elif kind == "huge":                # squares overflow fp32: the norm must stay finite
            x = torch.full((NMAX,), 1e25)
        else:                               # magnitudes from 1e-6 to 1e6
            x = torch.randn(NMAX, generator=gen) * 10.0 ** (torch.rand(NMAX, generator=gen) * 12.0 - 6.0)
        _values[kind] = x
    return _values[kind]


def ref_norm(kind, n):
    if (kind, n) not in _refs:
        _refs[(kind, n)] = float(values(kind)[:n].double().pow(2).sum().sqrt().float())
    return _refs[(kind, n)]


@pytest.mark.parametrize("kind", ["normal", "zeros", "tiny", "huge", "mix"])
def test_norm_matches_fp64_within_one_ulp(kind):
    from mrblip import ops, torch_ops  # noqa: F401
    worst = 0.0
    for n in NS:
        ref = ref_norm(kind, n)
        assert math.isfinite(ref)
        for off in (0, 1, 2, 3):
            g = poisoned_slice(values(kind)[:n], off)
            _, state, hout = prepare(g)
            st = state_of(state)
            assert st["nonfinite"] == 0, (kind, n, off, st)          # nothing outside [g, g + n) was read
            u = ulps(st["norm"], ref)
            worst = max(worst, u)
            assert u <= 1.0, (kind, n, off, st["norm"], ref, u)
            assert st["skip"] == 0 and st["applied"] == 1 and st["skipped"] == 0 and st["clip"] == 1.0 and st["consecutive"] == 0, (kind, n, off, st)
            if kind in ("tiny", "huge") and n > 0:
                assert st["norm"] > 0.0 and math.isfinite(st["norm"])
    print(f"grad norm [{kind}]: worst error {worst:.3f} ulp over {len(NS)} sizes x 4 offsets")
    # the public operator: same kernels, same bits
    g = poisoned_slice(values(kind)[:3 * C + 5], 3)
    norm, bad = torch.ops.mrblip.grad_norm(g)
    assert norm.dtype == torch.float32 and bad.dtype == torch.int32 and int(bad) == 0
    assert f32_of(norm.view(torch.int32).item()) == state_of(prepare(g)[1])["norm"]
    norm, bad = ops.grad_norm(g, grad_scale=-0.125)                # |grad_scale| is part of the norm
    assert ulps(float(norm), 0.125 * np.float64(values(kind)[:3 * C + 5].double().pow(2).sum().sqrt())) <= 1.0


# ------------------------------------------------------------------------------------------------------------ 2. bit reproducibility
def test_same_input_gives_the_same_bits():
    x, other = values("mix")[:3 * C + 5], values("normal")[:2 ** 20 + 17]
    for off in (0, 3):
        g = poisoned_slice(x, off)
        runs = []
        for k in range(3):
            ws, state, hout = prepare(g, max_norm=1.0)
            runs.append((ws.cpu(), state.cpu(), hout.view(torch.int32).cpu()))
            if k == 1:
                prepare(poisoned_slice(other, 1))                  # a call on other data in between
        for ws, state, hout in runs[1:]:
            assert torch.equal(ws, runs[0][0]) and torch.equal(state, runs[0][1]) and torch.equal(hout, runs[0][2])
        rec = runs[0][0].view(torch.float64).view(-1, 2)[:, 0]     # {fp64 sum of squares, u32 count, u32 reserved} per chunk
        for c in range(4):
            want = x[c * C: (c + 1) * C].double().pow(2).sum().item()
            assert abs(rec[c].item() - want) <= 2 * C * 2.0 ** -53 * want, (c, rec[c].item(), want)   # chunk c is [c C, min((c + 1) C, n))
        assert runs[0][0].view(torch.int32).view(-1, 4)[:, 2:].abs().sum().item() == 0


# ------------------------------------------------------------------------------------------------------------ 3. non-finite
N3, OFF3, ND3 = 3 * C + 5, 1, C + 7
# offset 1 float past a 16-byte line: every chunk starts with 3 scalar head elements; chunk 0 ends with 1 scalar tail element, the last with 2
PLANT = {"first (head)": 0, "head": 1, "chunk 0's last (tail)": C - 1, "chunk 1's first (head)": C, "a vector": 2 * C + 1001, "tail": N3 - 2,
         "last (tail)": N3 - 1}


def _pmv(n, seed=7):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=gen).to(dev()), (torch.randn(n, generator=gen) * 0.1).to(dev()), (torch.rand(n, generator=gen) * 0.01).to(dev()))


def _check_skipped(p, m, v, before, state, applied, skipped, nonfinite):
    st = state_of(state)
    assert st["skip"] == 1 and st["applied"] == applied and st["skipped"] == skipped and st["nonfinite"] == nonfinite, st
    assert st["norm_bits"] == INF_BITS                             # +inf
    for a, b in zip((p, m, v), before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))   # bit-identical


def test_nonfinite_gradient_skips_the_step():
    p, m, v = _pmv(N3)
    before = (p.clone(), m.clone(), v.clone())
    base = values("normal")[:N3]
    state = torch.tensor([0, 3, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev())
    skipped = 1
    for bad in (float("nan"), float("inf"), -float("inf")):
        for where, idx in PLANT.items():
            x = base.clone()
            x[idx] = bad
            guarded_step(p, poisoned_slice(x, OFF3), m, v, ND3, state)
            skipped += 1
            _check_skipped(p, m, v, before, state, 3, skipped, 1)
        x = base.clone()
        x[list(PLANT.values())] = bad
        guarded_step(p, poisoned_slice(x, OFF3), m, v, ND3, state)
        skipped += 1
        _check_skipped(p, m, v, before, state, 3, skipped, len(PLANT))
    assert state_of(state)["consecutive"] == skipped - 1
    # a finite gradient afterwards is applied, counted and ends the run of skips
    guarded_step(p, poisoned_slice(base, OFF3), m, v, ND3, state)
    st = state_of(state)
    assert st["skip"] == 0 and st["applied"] == 4 and st["skipped"] == skipped and st["consecutive"] == 0 and st["nonfinite"] == 0
    assert not torch.equal(p, before[0]) and torch.isfinite(p).all()


def test_norm_beyond_fp32_and_a_set_guard_word_skip_the_step():
    p, m, v = _pmv(4)
    before = (p.clone(), m.clone(), v.clone())
    state = torch.zeros(8, dtype=torch.int32, device=dev())
    guarded_step(p, torch.full((4,), 3e38, device=dev()), m, v, 2, state)      # every value finite, the norm 6e38 is not an fp32
    _check_skipped(p, m, v, before, state, 0, 1, 0)
    # a non-zero guard word skips a finite gradient in the same way (the norm is still reported)
    n = 1000
    p, m, v = _pmv(n)
    before = (p.clone(), m.clone(), v.clone())
    g = values("normal")[:n].to(dev())
    word = torch.zeros(1, dtype=torch.int32, device=dev())
    word.fill_(1)
    state = torch.zeros(8, dtype=torch.int32, device=dev())
    guarded_step(p, g, m, v, 600, state, guard=word)
    st = state_of(state)
    assert st["skip"] == 1 and st["applied"] == 0 and st["skipped"] == 1 and st["nonfinite"] == 0 and ulps(st["norm"], ref_norm("normal", n)) <= 1.0
    for a, b in zip((p, m, v), before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    word.zero_()
    guarded_step(p, g, m, v, 600, state, guard=word)
    assert state_of(state)["skip"] == 0 and state_of(state)["applied"] == 1 and not torch.equal(p, before[0])


# ------------------------------------------------------------------------------------------------------------ 4., 6., 7. AdamW
N4, ND4, LR, WD, EPS = 1000, 600, 3e-4, 0.05, 1e-8


class RefAdamW:
    """torch.optim.AdamW in fp64 on the CPU over a decay and a no-decay segment"""

    def __init__(self, p0):
        self.a = p0[:ND4].double().cpu().clone().requires_grad_(True)
        self.b = p0[ND4:].double().cpu().clone().requires_grad_(True)
        self.opt = torch.optim.AdamW([{"params": [self.a], "weight_decay": WD}, {"params": [self.b], "weight_decay": 0.0}], lr=LR, betas=(B1, B2), eps=EPS)

    def step(self, g, scale=1.0, max_norm=None):
        self.a.grad, self.b.grad = g[:ND4].double().cpu() * scale, g[ND4:].double().cpu() * scale
        norm = None
        if max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_([self.a, self.b], max_norm))
        self.opt.step()
        return norm

    def p(self):
        return torch.cat([self.a.detach(), self.b.detach()])

    def moment(self, key):
        return torch.cat([self.opt.state[self.a][key], self.opt.state[self.b][key]])


def _grads(k, seed=21):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(N4, generator=gen).to(dev()) for _ in range(k)]


def _fresh():
    p0 = torch.randn(N4, generator=torch.Generator().manual_seed(3)).to(dev())
    return p0, p0.clone(), torch.zeros(N4, device=dev()), torch.zeros(N4, device=dev()), torch.zeros(8, dtype=torch.int32, device=dev())


def test_skipped_steps_do_not_count():
    """5 steps, NaN gradients at steps 2 and 4: parameters and moments equal AdamW run on the 3 finite gradients only.  (With a host-side
    clock that counted 5 steps the bias terms of the last two applied steps would be those of steps 3 and 5.)"""
    p0, p, m, v, state = _fresh()
    ref = RefAdamW(p0)
    for step, g in enumerate(_grads(5), 1):
        if step in (2, 4):
            g = g.clone()
            g[(17 if step == 2 else 700)] = float("nan")
        else:
            ref.step(g)
        guarded_step(p, g, m, v, ND4, state, lr=LR, wd=WD, eps=EPS)
    st = state_of(state)
    assert st["applied"] == 3 and st["skipped"] == 2 and st["consecutive"] == 0
    errs = rel(p, ref.p()), rel(m, ref.moment("exp_avg")), rel(v, ref.moment("exp_avg_sq"))
    print("skipped steps: rel of p, m, v vs fp64 AdamW on the 3 finite gradients: %.3e %.3e %.3e" % errs)
    assert max(errs) < 1e-6, errs


@pytest.mark.parametrize("max_norm,clipped", [(1.0, True), (100.0, False)])
def test_clipping_matches_clip_grad_norm(max_norm, clipped):
    """4 steps against clip_grad_norm_(max_norm) + AdamW in fp64; grad_scale = 0.125 (the accumulation case): the norm includes the scale"""
    gs = 0.125
    p0, p, m, v, state = _fresh()
    ref = RefAdamW(p0)
    for g in _grads(4, seed=22):
        norm = ref.step(g, scale=gs, max_norm=max_norm)
        hout = guarded_step(p, g, m, v, ND4, state, lr=LR, gs=gs, wd=WD, eps=EPS, max_norm=max_norm)
        st = state_of(state)
        assert st["skip"] == 0 and ulps(st["norm"], norm) <= 1.0, (st, norm)
        want = min(1.0, max_norm / (norm + 1e-6))
        h3 = hout.view(torch.int32)[3].item()
        if clipped:
            assert want < 1.0 and st["clip"] < 1.0 and ulps(st["clip"], want) <= 1.0, (st["clip"], want)
            assert f32_of(h3) == float(np.float32(gs) * np.float32(st["clip"]))
        else:
            assert st["clip"] == 1.0 and f32_of(h3) == gs                      # bit for bit: 0.125 is an fp32
    assert state_of(state)["applied"] == 4
    errs = rel(p, ref.p()), rel(m, ref.moment("exp_avg")), rel(v, ref.moment("exp_avg_sq"))
    print("clipping (max_norm %g): rel of p, m, v vs fp64 clip_grad_norm_ + AdamW: %.3e %.3e %.3e" % ((max_norm,) + errs))
    assert max(errs) < 1e-6, errs


def test_guard_with_nothing_to_do_matches_the_unguarded_path():
    """3 finite gradients, no clipping: the guarded sequence against ops.adamw driven by host-side bias terms.  The two may differ in the
    last bit of a bias term (host pow against device pow in double, each rounded to fp32): within the AdamW bound, not bit-equal."""
    from mrblip import ops
    p0, p, m, v, state = _fresh()
    q, qm, qv = p0.clone(), torch.zeros_like(m), torch.zeros_like(v)
    for t, g in enumerate(_grads(3, seed=23), 1):
        guarded_step(p, g, m, v, ND4, state, lr=LR, wd=WD, eps=EPS)
        hyper = torch.tensor([LR, 1.0 / (1 - B1 ** t), 1.0 / math.sqrt(1 - B2 ** t), 1.0], device=dev())
        ops.adamw(q[:ND4], g[:ND4], qm[:ND4], qv[:ND4], hyper, B1, B2, EPS, WD)
        ops.adamw(q[ND4:], g[ND4:], qm[ND4:], qv[ND4:], hyper, B1, B2, EPS, 0.0)
    assert state_of(state)["applied"] == 3 and state_of(state)["skipped"] == 0
    errs = rel(p, q), rel(m, qm), rel(v, qv)
    assert max(errs) < 1e-6, errs


# ------------------------------------------------------------------------------------------------------------ 5. bias terms
def test_bias_terms_match_the_double_formulas():
    g = values("normal")[:1000].to(dev())
    lr = 3e-4
    for b1, b2 in ((0.9, 0.999), (B1, B2), (0.0, 0.5)):
        for applied in (0, 1, 2, 9, 999, 10 ** 6 - 1):
            state = torch.tensor([0, applied, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev())
            _, state, hout = prepare(g, state, lr=lr, betas=(b1, b2))
            t = applied + 1
            assert state_of(state)["applied"] == t
            h = [f32_of(w) for w in hout.view(torch.int32).cpu().tolist()]
            assert h[0] == float(np.float32(lr))                               # bit for bit
            w1, w2 = 1.0 / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)
            assert ulps(h[1], w1) <= 1.0 and ulps(h[2], w2) <= 1.0, (b1, b2, t, h, w1, w2)
            assert h[3] == 1.0


# ------------------------------------------------------------------------------------------------------------ 8. - 10. model level
@pytest.fixture(scope="module")
def tiny():
    import lavis  # noqa: F401
    from lavis.common.config import load_yaml
    from lavis.common.registry import registry
    from lavis.datasets import SyntheticMomentRetrievalDataset, collate

    cls = registry.get_model_class("blip2_mr")
    mcfg = load_yaml(cls.default_config_path("tiny_synthetic")).model
    mcfg.update(dict(task="qformer_freeze_lora", input_time_format="seconds_integers", interleave_data=True, seed=11))
    model = cls.from_config(mcfg)
    model.train()
    model.begin_accumulation(1.0)           # what RunnerBase does: gradients accumulate in the engine's flat buffer
    ds = SyntheticMomentRetrievalDataset(n_items=2, n_frms=4, image_size=56, duration=60.0)
    return types.SimpleNamespace(model=model, eng=model.train_engine, w0=model.train_engine.flat.clone(), batch=lambda: collate([ds[0], ds[1]]))


def _reset(tiny):
    tiny.eng.flat.copy_(tiny.w0)
    tiny.eng.refresh_trainable()
    tiny.model.zero_grad()


def _three_steps(tiny, opt):
    """a normal step, a step with a NaN written into the gradient between backward() and step(), a normal step"""
    model, eng = tiny.model, tiny.eng
    out = types.SimpleNamespace()
    model(tiny.batch())["loss"].backward()
    opt.step()
    opt.zero_grad()
    out.w1 = eng.flat.clone()
    model(tiny.batch())["loss"].backward()
    model.grad_buffer()[5] = float("nan")
    opt.step()
    opt.zero_grad()
    out.w2 = eng.flat.clone()
    loss = model(tiny.batch())["loss"]
    loss.backward()
    opt.step()
    opt.zero_grad()
    out.loss3, out.w3 = loss.item(), eng.flat.clone()
    return out


def test_model_level_nan_gradient_is_skipped(tiny):
    from lavis.runners.runner_base import FlatAdamW
    _reset(tiny)
    opt = FlatAdamW(tiny.model, lr=1e-3, weight_decay=0.05, grad_guard=True)
    r = _three_steps(tiny, opt)
    assert not torch.equal(r.w1, tiny.w0)
    assert torch.isfinite(r.w2).all() and torch.equal(r.w2.view(torch.int32), r.w1.view(torch.int32))   # the poisoned step changed nothing
    assert math.isfinite(r.loss3) and torch.isfinite(r.w3).all() and not torch.equal(r.w3, r.w2)
    st = opt.stats(block=True)
    assert st["skipped_steps"] == 1 and st["applied_steps"] == 2 and st["skipped_step"] is False and st["nonfinite"] == 0
    assert math.isfinite(st["grad_norm"]) and st["grad_norm"] > 0 and st["clip"] == 1.0
    assert set(st) == {"grad_norm", "clip", "nonfinite", "skipped_step", "applied_steps", "skipped_steps"}
    # what the switch buys: the same sequence without the guard ends with non-finite weights
    _reset(tiny)
    plain = FlatAdamW(tiny.model, lr=1e-3, weight_decay=0.05)
    assert plain.stats() is None
    r = _three_steps(tiny, plain)
    assert not torch.isfinite(r.w3).all()
    _reset(tiny)


def test_engine_optimizer_step_with_the_guard(tiny):
    _reset(tiny)
    model, eng = tiny.model, tiny.eng
    samples = tiny.batch()
    video = model._frames_to_device(samples["video"])
    layout = model._layout(dict(samples, relevant_windows=[str(w) for w in samples["relevant_windows"]]))
    eng.grad_guard().set_clock(0, 0)
    m0, v0 = eng.adam_m.clone(), eng.adam_v.clone()
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    ws = []
    for step in range(3):
        eng.zero_grad()
        loss = eng.forward_backward(video, layout)
        if step == 1:
            eng.grad[5] = float("nan")
        eng.optimizer_step(lr=1e-3, weight_decay=0.05, grad_guard=True)
        ws.append(eng.flat.clone())
    assert not torch.equal(ws[0], tiny.w0) and torch.equal(ws[1].view(torch.int32), ws[0].view(torch.int32))
    assert math.isfinite(loss.item()) and torch.isfinite(ws[2]).all() and not torch.equal(ws[2], ws[1])
    st = eng.grad_guard().stats(block=True)
    assert st["skipped_steps"] == 1 and st["applied_steps"] == 2 and math.isfinite(st["grad_norm"])
    assert eng.grad_guard().read()["applied_steps"] == 2
    eng.adam_m.copy_(m0)
    eng.adam_v.copy_(v0)
    eng.zero_grad()
    _reset(tiny)


def test_train_loop_logs_the_norm_and_stops_a_run_that_trains_nothing(tiny):
    import lavis  # noqa: F401
    from lavis.common.registry import registry
    from lavis.runners.runner_base import FlatAdamW
    _reset(tiny)
    task = registry.get_task_class("moment_retrieval")()
    sched = types.SimpleNamespace(step=lambda cur_epoch, cur_step: None)
    opt = FlatAdamW(tiny.model, lr=1e-3, weight_decay=0.05, max_grad_norm=0.5)
    calls, real_stats = [], opt.stats

    def counting_stats(block=False):
        calls.append(block)
        return real_stats(block=block)

    opt.stats = counting_stats
    stats = task.train_epoch(epoch=0, model=tiny.model, data_loader=[tiny.batch() for _ in range(4)], optimizer=opt, lr_scheduler=sched,
                             log_freq=50, accum_grad_iters=1)
    assert "grad_norm" in stats and math.isfinite(float(stats["grad_norm"])) and float(stats["grad_norm"]) > 0, stats
    assert float(stats["skipped_steps"]) == 0
    assert calls and not any(calls), calls                                     # the loop never waits for a state
    st = real_stats(block=True)
    assert st["applied_steps"] == 4 and 0 < st["clip"] <= 1.0
    # every gradient poisoned: the run must not look healthy
    _reset(tiny)
    opt = FlatAdamW(tiny.model, lr=1e-3, weight_decay=0.05, grad_guard=True, max_consecutive_skips=2)
    real_step, steps = opt.step, []

    def poisoned_step():
        steps.append(1)
        tiny.model.grad_buffer()[3] = float("nan")
        real_step()

    opt.step = poisoned_step
    with pytest.raises(RuntimeError, match="in a row"):
        task.train_epoch(epoch=0, model=tiny.model, data_loader=[tiny.batch() for _ in range(6)], optimizer=opt, lr_scheduler=sched, log_freq=50,
                         accum_grad_iters=1)
    assert len(steps) <= 4, len(steps)
    assert torch.equal(tiny.eng.flat.view(torch.int32), tiny.w0.view(torch.int32))   # nothing was applied
    torch.cuda.synchronize()
    _reset(tiny)


def test_checkpoint_round_trip(tiny):
    from lavis.runners.runner_base import FlatAdamW
    _reset(tiny)
    model, eng = tiny.model, tiny.eng
    opt = FlatAdamW(model, lr=1e-3, weight_decay=0.05, grad_guard=True)
    _three_steps(tiny, opt)
    sd = opt.state_dict()
    assert sd["t"] == 2 and sd["skipped"] == 1
    sd = {k: (x.clone() if torch.is_tensor(x) else x) for k, x in sd.items()}
    w = eng.flat.clone()
    model(tiny.batch())["loss"].backward()
    grad = model.grad_buffer().clone()
    after = []
    for kw in (dict(grad_guard=True), dict()):
        eng.flat.copy_(w)
        eng.refresh_trainable()
        model.grad_buffer().copy_(grad)
        fresh = FlatAdamW(model, lr=1e-3, weight_decay=0.05, **kw)
        fresh.load_state_dict(sd)
        fresh.step()
        after.append(eng.flat.clone())
        if kw:
            assert fresh.state_dict()["t"] == 3 and fresh.state_dict()["skipped"] == 1
        else:
            assert fresh.t == 3
    assert not torch.equal(after[0], w)
    assert rel(after[0], after[1]) < 1e-6
    _reset(tiny)
