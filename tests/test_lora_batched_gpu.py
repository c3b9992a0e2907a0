"""The batched LoRA entry points (mrblip.ops lora_grads_batched / lora_rows_batched / lora_dx_add_batched) at the kernel level, against
fp64 references computed from the same bf16 operands with the oracle's dropout masks, at the shapes the train step runs (a whole XL
encoder layer's weight-gradient jobs, the stacked cross-attention K / V adapters of up to 24 decoder layers) and at the edges (1..17-row
decoder jobs, odd M, adapter segments that do not start on a 64-column tile, a job whose width is not a multiple of 64).

Besides the global relative error every product reports its WORST ROW (a rank row of dA / dB^T, a matrix row of u and dx): a global L2
norm over [2012 x 4096] outputs hides a wrong tail tile or one wrong group.  Outputs are allocated with padding filled with NaN and the
padding must come back bit-unchanged; where the library documents "the same bits" as another launch (one lora_grads call per job, one
lora_rows call per group) that is asserted bitwise."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from util import check, relerr  # noqa: E402

SEED = 4242


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from mrblip import ops as _ops

    return _ops


def dev():
    return torch.device("cuda:0")


def randn(*shape, scale=1.0, gen=None):
    return (torch.randn(*shape, generator=gen) * scale).to(dev())


def keep(shape, site, p):
    """the oracle's keep mask (0 / 1) of call site `site` under SEED, fp32 on the device"""
    from oracle.mrblip_oracle import dropout_keep

    return dropout_keep(shape, SEED, site, p).to(dev())


def inv_keep(p):
    """the kernels' 1 / (1 - p), evaluated in fp32 as they do"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def rowerr(out, ref):
    """worst relative L2 error over the rows of a 2-D output"""
    out, ref = out.double(), ref.double()
    return ((out - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max().item()


def bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


def nan_buf(rows, ld, dtype):
    return torch.full((rows, ld), float("nan"), dtype=dtype, device=dev())


# ------------------------------------------------------------------------------------------------ a) lora_grads_batched
def _job(M, N, K, segs, p, site, gen):
    """operands of one fused LoRA group: segs = [(b_col0, b_ncols)] per adapter.  dy / x sit in wider buffers (ld > N / K), u / g carry
    garbage in the columns >= R that no product may read, the outputs start non-zero (+=) inside NaN-padded rows (ld > cols)."""
    R = 8 * len(segs)
    dyb = randn(M, N + 8, gen=gen).bfloat16()
    xb = randn(M, K + 8, gen=gen).bfloat16()
    u = torch.full((M, 64), 1e4, dtype=torch.bfloat16, device=dev())
    g = torch.full((M, 64), -1e4, dtype=torch.bfloat16, device=dev())
    u[:, :R] = randn(M, R, gen=gen).bfloat16()
    g[:, :R] = randn(M, R, gen=gen).bfloat16()
    s = float(M) ** 0.5
    dB, dA = [], []
    for _, nc in segs:
        b = nan_buf(8, nc + 8, torch.float32)
        b[:, :nc] = randn(8, nc, scale=s, gen=gen)
        dB.append(b)
        a = nan_buf(8, K + 16, torch.float32)
        a[:, :K] = randn(8, K, scale=s, gen=gen)
        dA.append(a)
    return dict(M=M, N=N, K=K, segs=segs, p=p, site=site, dy=dyb[:, :N], x=xb[:, :K], u=u, g=g, dB=dB, dA=dA)


def _args(ops, j, seed, dB, dA):
    drop = ops.Dropout(seed, j["site"], j["p"]) if j["p"] > 0 else None
    segs = j["segs"]
    return ((j["dy"], j["u"], j["x"], j["g"], dB, [c for c, _ in segs], [n for _, n in segs], dA, j["K"]),
            dict(drop=drop, b_lds=[n + 8 for _, n in segs], a_lds=[j["K"] + 16] * len(segs)))


def _grads_refs(j):
    """fp64: dB^T_a = init + u_a^T dy[:, cols_a];  dA_a = init + g_a^T bf16(x * mask / (1 - p))"""
    x = j["x"]
    if j["p"] > 0:
        x = (x.float() * keep((j["M"], j["K"]), j["site"], j["p"]) * inv_keep(j["p"])).bfloat16()
    xd, dy = x.double(), j["dy"].double()
    rb, ra = [], []
    for a, (c0, nc) in enumerate(j["segs"]):
        rb.append(j["dB"][a][:, :nc].double() + j["u"][:, 8 * a: 8 * a + 8].double().t() @ dy[:, c0: c0 + nc])
        ra.append(j["dA"][a][:, :j["K"]].double() + j["g"][:, 8 * a: 8 * a + 8].double().t() @ xd)
    return rb, ra


ENC_LAYER = [  # (M, N, K, adapter segments, p, site): the XL encoder layer's four groups, one launch in the step
    (2012, 6144, 2048, [(0, 2048), (2048, 2048), (4096, 2048)], 0.1, 101),   # q / k / v
    (2012, 2048, 2048, [(0, 2048)], 0.0, 102),                               # o
    (2012, 10240, 2048, [(0, 5120), (5120, 5120)], 0.1, 103),                # wi_0 / wi_1
    (2012, 2048, 5120, [(0, 2048)], 0.05, 104),                              # wo
]
EIGHT_JOBS = [  # decoder rows and short inputs; segments whose start / width are not multiples of 64 while N is
    (1, 128, 256, [(0, 64), (64, 64)], 0.1, 201),
    (8, 192, 128, [(0, 96), (96, 96)], 0.0, 202),
    (15, 320, 64, [(0, 40), (40, 200), (240, 80)], 0.1, 203),
    (17, 256, 512, [(0, 256)], 0.05, 204),
    (72, 384, 192, [(0, 128), (128, 136), (264, 120)], 0.1, 205),
    (333, 512, 320, [(0, 100), (100, 156), (256, 200), (456, 56)], 0.1, 206),
    (333, 2048, 2048, [(0, 2048)], 0.0, 207),
    (72, 64, 64, [(0, 64)], 0.1, 208),
]
ONE_JOB = [(500, 1024, 768, [(0, 512), (512, 512)], 0.1, 301)]
CT1_JOBS = [  # a width that is not a multiple of 64 sends the whole launch to the one-tile body (lora_tn_multi_kernel<1>)
    (333, 200, 256, [(0, 200)], 0.1, 401),
    (72, 512, 232, [(0, 256), (256, 256)], 0.05, 402),
    (17, 128, 128, [(0, 128)], 0.0, 403),
]


@pytest.mark.parametrize("name,specs", [("encoder layer M=2012, 4 jobs", ENC_LAYER), ("8 jobs, M=1..333", EIGHT_JOBS),
                                        ("1 job", ONE_JOB), ("3 jobs, one width % 64 != 0", CT1_JOBS)])
def test_lora_grads_batched_against_fp64_and_per_group_launches(ops, name, specs):
    gen = torch.Generator().manual_seed(len(specs) * 1000 + specs[0][0])
    seed = torch.tensor([SEED], dtype=torch.int32, device=dev())
    jobs = [_job(*s, gen=gen) for s in specs]
    refs = [_grads_refs(j) for j in jobs]
    single = [([b.clone() for b in j["dB"]], [a.clone() for a in j["dA"]]) for j in jobs]
    batched_jobs = []
    for j in jobs:
        a, kw = _args(ops, j, seed, j["dB"], j["dA"])
        batched_jobs.append(ops.lora_grads_job(*a, **kw))
    pads = [[bits(b[:, n:]).clone() for b, (_, n) in zip(j["dB"], j["segs"])] + [bits(a[:, j["K"]:]).clone() for a in j["dA"]] for j in jobs]
    ops.lora_grads_batched(batched_jobs)
    for j, (dB, dA) in zip(jobs, single):    # the documented contract: the same bits as one lora_grads launch per group
        a, kw = _args(ops, j, seed, dB, dA)
        ops.lora_grads(*a, **kw)
    torch.cuda.synchronize()
    eb = ea = rb = ra = 0.0
    for i, (j, (refb, refa), (dB, dA), pad) in enumerate(zip(jobs, refs, single, pads)):
        tag = f"job {i} (M={j['M']} N={j['N']} K={j['K']} p={j['p']})"
        for a, (_, nc) in enumerate(j["segs"]):
            assert torch.equal(bits(j["dB"][a]), bits(dB[a])), f"{tag}: dB^T of adapter {a} differs from the lora_grads launch"
            assert torch.equal(bits(j["dA"][a]), bits(dA[a])), f"{tag}: dA of adapter {a} differs from the lora_grads launch"
            eb, rb = max(eb, relerr(j["dB"][a][:, :nc], refb[a])), max(rb, rowerr(j["dB"][a][:, :nc], refb[a]))
            ea, ra = max(ea, relerr(j["dA"][a][:, :j["K"]], refa[a])), max(ra, rowerr(j["dA"][a][:, :j["K"]], refa[a]))
        now = [bits(b[:, n:]) for b, (_, n) in zip(j["dB"], j["segs"])] + [bits(a[:, j["K"]:]) for a in j["dA"]]
        assert all(torch.equal(x, y) for x, y in zip(now, pad)), f"{tag}: a write outside the output columns"
    tag = f"lora_grads_batched {name}: "
    check(tag + "dB^T vs fp64", eb, 2e-7)                  # (measured 5.2e-8 ... 7.8e-8: fp32 accumulation over M rows)
    check(tag + "dB^T worst rank row vs fp64", rb, 2e-7)   # (measured 5.8e-8 ... 8.0e-8)
    check(tag + "dA vs fp64", ea, 2e-7)                    # (measured 5.3e-8 ... 7.9e-8)
    check(tag + "dA worst rank row vs fp64", ra, 2e-7)     # (measured 6.0e-8 ... 8.2e-8)


def test_lora_grads_batched_refuses_bad_job_lists(ops):
    gen = torch.Generator().manual_seed(5)
    j = _job(17, 64, 64, [(0, 64)], 0.1, 9, gen)
    s1, s2 = torch.tensor([1], dtype=torch.int32, device=dev()), torch.tensor([2], dtype=torch.int32, device=dev())
    a, kw = _args(ops, j, s1, j["dB"], j["dA"])
    job = ops.lora_grads_job(*a, **kw)
    before = [bits(b).clone() for b in j["dB"] + j["dA"]]
    with pytest.raises(ops.MrblipError, match="1..8 jobs"):
        ops.lora_grads_batched([])
    with pytest.raises(ops.MrblipError, match="1..8 jobs"):
        ops.lora_grads_batched([job] * 9)
    a, kw = _args(ops, j, s2, j["dB"], j["dA"])
    with pytest.raises(ops.MrblipError, match="one device seed"):
        ops.lora_grads_batched([job, ops.lora_grads_job(*a, **kw)])
    torch.cuda.synchronize()
    assert all(torch.equal(bits(b), x) for b, x in zip(j["dB"] + j["dA"], before)), "a refused launch wrote"


# ------------------------------------------------------------------------------------------------ b) lora_rows_batched
ROWS_CASES = [  # (form, G, R, M, K): "fwd" = x_gstride 0 (one encoder output, a mask per group), "bwd" = x_gstride = K (dy column blocks, p = 0)
    ("fwd", 24, 16, 2012, 2048), ("fwd", 8, 8, 511, 4096), ("fwd", 2, 24, 17, 128), ("fwd", 10, 32, 1, 2048), ("fwd", 1, 16, 16, 128),
    ("fwd", 8, 16, 15, 2048), ("fwd", 10, 8, 72, 4096), ("fwd", 2, 32, 2012, 4096),
    ("bwd", 10, 16, 2012, 2048), ("bwd", 8, 24, 600, 128), ("bwd", 2, 32, 17, 128), ("bwd", 24, 8, 72, 128), ("bwd", 1, 8, 2012, 4096),
]


@pytest.mark.parametrize("form,G,R,M,K", ROWS_CASES)
def test_lora_rows_batched_against_fp64(ops, form, G, R, M, K):
    gen = torch.Generator().manual_seed(G * 100000 + M * 10 + R)
    fwd = form == "fwd"
    p, site0, ss = (0.1 if fwd else 0.0), 300 + G, 7
    seed = torch.tensor([SEED], dtype=torch.int32, device=dev())
    xw = K if fwd else G * K
    xb = torch.full((M, xw + 64), 1e4, dtype=torch.bfloat16, device=dev())     # (ld > the columns read; the pad must not be read)
    xb[:, :xw] = randn(M, xw, gen=gen).bfloat16()
    a = randn(G * R, K, scale=0.05, gen=gen).bfloat16()
    u = nan_buf(M, G * 64 + 64, torch.bfloat16)
    drop = ops.Dropout(seed, site0, p) if fwd else None
    ops.lora_rows_batched(xb, a, u, K, G, x_gstride=0 if fwd else K, a_gstride=R * K, u_gstride=64, R=R, drop=drop, site_stride=ss)
    torch.cuda.synchronize()
    e = re = 0.0
    outs, refs = [], []
    for g in range(G):
        xg = xb[:, :K] if fwd else xb[:, g * K:(g + 1) * K]
        xd = xg.double()
        if fwd:
            xd = xd * keep((M, K), site0 + g * ss, p).double()
        ref = xd @ a[g * R:(g + 1) * R].double().t() * (inv_keep(p) if fwd else 1.0)
        out = u[:, 64 * g: 64 * g + R]
        outs.append(out)
        refs.append(ref)
        re = max(re, rowerr(out, ref))
        assert torch.isnan(u[:, 64 * g + R: 64 * g + 64].float()).all(), f"group {g}: a write into the K-extension columns past R"
        if M >= 512:   # both launches run lora_thin_body: the same bits as a lora_rows call on the group's slices
            us = nan_buf(M, 64, torch.bfloat16)
            ops.lora_rows(xg, a[g * R:(g + 1) * R], us, K, drop=ops.Dropout(seed, site0 + g * ss, p) if fwd else None)
            torch.cuda.synchronize()
            assert torch.equal(bits(us[:, :R]), bits(out)), f"group {g}: differs from the lora_rows launch"
    assert torch.isnan(u[:, G * 64:].float()).all(), "a write past the last group"
    e = relerr(torch.cat(outs, 1), torch.cat(refs, 1))
    tag = f"lora_rows_batched {form} G={G} R={R} M={M} K={K}: "
    check(tag + "u vs fp64", e, 3.4e-3)           # (measured 1.6e-3 ... 1.7e-3: the bf16 rounding of u)
    check(tag + "u worst row vs fp64", re, 4e-3)  # (measured 1.9e-3 ... 3.4e-3; a row's bound is bf16's unit roundoff 2^-8 = 3.9e-3)


# ------------------------------------------------------------------------------------------------ c) lora_dx_add_batched
DX_CASES = [(10, 2012, 2048, 16, 0.1), (10, 2012, 2048, 16, 0.0), (8, 2012, 2048, 16, 0.1), (3, 333, 128, 24, 0.1), (1, 17, 64, 8, 0.1),
            (24, 511, 256, 32, 0.0)]


@pytest.mark.parametrize("G,M,K,R,p", DX_CASES)
def test_lora_dx_add_batched_against_fp64(ops, G, M, K, R, p):
    gen = torch.Generator().manual_seed(G * 1000 + M + R)
    site0, ss = 500 + G, 3
    seed = torch.tensor([SEED], dtype=torch.int32, device=dev())
    dxb = nan_buf(M, K + 16, torch.float32)
    dxb[:, :K] = randn(M, K, scale=0.2, gen=gen)
    dx0 = dxb[:, :K].clone()
    g = torch.full((M, G * 64), 1e4, dtype=torch.bfloat16, device=dev())      # (columns >= R of every group must not be read)
    for j in range(G):
        g[:, 64 * j: 64 * j + R] = randn(M, R, gen=gen).bfloat16()
    a = randn(G * R, K, scale=0.05, gen=gen).bfloat16()
    drop = ops.Dropout(seed, site0, p) if p > 0 else None
    ops.lora_dx_add_batched(dxb[:, :K], g, a, K, G, g_gstride=64, a_gstride=R * K, R=R, drop=drop, site_stride=ss)
    ref = dx0.double()
    for j in range(G):
        t = g[:, 64 * j: 64 * j + R].double() @ a[j * R:(j + 1) * R].double()
        if p > 0:
            t = t * keep((M, K), site0 + j * ss, p).double() * inv_keep(p)
        ref = ref + t
    torch.cuda.synchronize()
    assert torch.isnan(dxb[:, K:]).all(), "a write past K"
    tag = f"lora_dx_add_batched G={G} M={M} K={K} R={R} p={p}: "
    check(tag + "dx vs fp64", relerr(dxb[:, :K], ref), 2.6e-7)               # (measured 3.1e-8 ... 1.0e-7)
    check(tag + "dx worst row vs fp64", rowerr(dxb[:, :K], ref), 2.6e-7)     # (measured 3.7e-8 ... 1.3e-7)


# ------------------------------------------------------------------------------------------------ d) the stacked cross K / V chain
@pytest.mark.parametrize("G", [8, 10])
def test_stacked_cross_kv_lora_chain_against_fp64_peft_autograd(ops, G):
    """G decoder layers' EncDecAttention.k / .v adapters (peft lora.Linear, r = 8, one lora_dropout(x) per Linear call) on one encoder
    output: y_g = base(x) + s * dropout_g(x) A_g^T B_g^T for the k and v adapters of layer g.  The engine's chunk (engine.py cross_kv_all /
    ckv_chunk_bwd): u = lora_rows_batched (forward), g = dy (s B) by lora_rows_batched over dy's column blocks, the weight gradients per
    layer (lora_grads), the rank-16 input-gradient terms of all layers in one lora_dx_add_batched.  Against float64 autograd of the
    LoRA terms (the frozen base projection contributes nothing to dA, dB or the LoRA part of dx).  The forward's mask of layer g and the
    backward's mask of layer g must be the same draw."""
    gen = torch.Generator().manual_seed(70 + G)
    M, K, inner, R, p, s = 2012, 2048, 512, 16, 0.1, 1.0      # s = lora_alpha / r = 8 / 8 (blip2_mr.py LoraConfig)
    N = 2 * inner
    site0, ss = 1000, 11
    seed = torch.tensor([SEED], dtype=torch.int32, device=dev())
    x = randn(M, K, gen=gen).bfloat16()
    A = [randn(8, K, scale=0.05, gen=gen).bfloat16() for _ in range(2 * G)]         # adapter 2g = layer g's k, 2g + 1 = its v
    B = [randn(inner, 8, scale=0.05, gen=gen).bfloat16() for _ in range(2 * G)]
    dy = randn(M, G * N, gen=gen).bfloat16()
    # engine operand layout: acat = s A stacked per layer [G * 16, K]; bblk = block-diagonal s B^T per layer [G * 16, N]
    acat = torch.cat([(A[i].float() * s).bfloat16() for i in range(2 * G)], 0)
    bblk = torch.zeros(G * R, N, dtype=torch.bfloat16, device=dev())
    for i in range(2 * G):
        l, h = divmod(i, 2)
        bblk[16 * l + 8 * h: 16 * l + 8 * h + 8, h * inner:(h + 1) * inner] = (B[i].float().t() * s).bfloat16()
    u_all = nan_buf(M, G * 64, torch.bfloat16)
    g_all = nan_buf(M, G * 64, torch.bfloat16)
    ops.lora_rows_batched(x, acat, u_all, K, G, a_gstride=R * K, u_gstride=64, R=R, drop=ops.Dropout(seed, site0, p), site_stride=ss)
    ops.lora_rows_batched(dy, bblk, g_all, N, G, x_gstride=N, a_gstride=R * N, u_gstride=64, R=R)
    dBt = [torch.zeros(8, inner, device=dev()) for _ in range(2 * G)]
    dA = [torch.zeros(8, K, device=dev()) for _ in range(2 * G)]
    for l in range(G):
        ops.lora_grads(dy[:, l * N:(l + 1) * N], u_all[:, 64 * l: 64 * l + 64], x, g_all[:, 64 * l: 64 * l + 64], dBt[2 * l: 2 * l + 2],
                       [0, inner], [inner, inner], dA[2 * l: 2 * l + 2], K, drop=ops.Dropout(seed, site0 + l * ss, p))
    dx = torch.zeros(M, K, device=dev())
    ops.lora_dx_add_batched(dx, g_all, acat, K, G, g_gstride=64, a_gstride=R * K, R=R, drop=ops.Dropout(seed, site0, p), site_stride=ss)
    # float64 peft
    xr = x.double().requires_grad_(True)
    Ar = [a.double().requires_grad_(True) for a in A]
    Br = [b.double().requires_grad_(True) for b in B]
    loss, hs = 0.0, []
    for l in range(G):
        xd = xr * keep((M, K), site0 + l * ss, p).double() / (1 - p)   # peft: one lora_dropout(x) per Linear call, shared by nothing else
        for h in range(2):
            i = 2 * l + h
            hh = xd @ Ar[i].t()
            hs.append(hh.detach() * s)
            loss = loss + ((s * hh @ Br[i].t()) * dy[:, l * N + h * inner: l * N + (h + 1) * inner].double()).sum()
    loss.backward()
    torch.cuda.synchronize()
    eu = ru = eb = rb = ea = ra = 0.0
    for l in range(G):
        u = u_all[:, 64 * l: 64 * l + 16]
        uref = torch.cat(hs[2 * l: 2 * l + 2], 1)
        eu, ru = max(eu, relerr(u, uref)), max(ru, rowerr(u, uref))
        for h in range(2):
            i = 2 * l + h
            eb, rb = max(eb, relerr(dBt[i], Br[i].grad.t())), max(rb, rowerr(dBt[i], Br[i].grad.t()))
            ea, ra = max(ea, relerr(dA[i], Ar[i].grad)), max(ra, rowerr(dA[i], Ar[i].grad))
    tag = f"stacked cross K/V LoRA chain G={G} vs fp64 peft autograd: "
    # (measured, G = 8 / 10: u 1.7e-3 / worst row 3.1e-3 / 3.2e-3, dB^T 1.7e-3 / 1.9e-3, dA 2.4e-3 / 2.6e-3, dx 1.7e-3 / 2.1e-3: the bf16
    # roundings of u, g and dropout(x); a wrong mask for one layer moves these by O(1))
    check(tag + "u (worst layer)", eu, 3.4e-3)
    check(tag + "u worst row", ru, 6.5e-3)
    check(tag + "dB^T (worst adapter)", eb, 3.4e-3)
    check(tag + "dB^T worst rank row", rb, 3.8e-3)
    check(tag + "dA (worst adapter)", ea, 4.8e-3)
    check(tag + "dA worst rank row", ra, 5.2e-3)
    check(tag + "LoRA part of dx", relerr(dx, xr.grad), 3.4e-3)
    check(tag + "LoRA part of dx, worst row", rowerr(dx, xr.grad), 4.2e-3)
