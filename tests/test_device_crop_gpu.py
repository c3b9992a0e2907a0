"""The device-side crop + bicubic resize (csrc/augment.hip, ops.crop_resize_u8) on the GPU: every output level against an fp64 restatement
of torch's bicubic formula, bit-exact identity, the loader's CPU path, determinism, and the ``crop_box`` key through the model and the
train loop's look-ahead."""
import json
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

A = -0.75


def _axis64(n_in, n_out):
    """tap indices [n_out,4] (clamped to the crop) and cubic-convolution weights [n_out,4] of one axis, float64"""
    o = np.arange(n_out, dtype=np.float64)
    s = (n_in / n_out) * (o + 0.5) - 0.5
    i0 = np.floor(s)
    t = s - i0
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1          # noqa: E731
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A    # noqa: E731
    w = np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], 1)
    idx = np.clip(i0[:, None].astype(np.int64) + np.arange(-1, 3)[None], 0, n_in - 1)
    return idx, w


def ref64(src, box, out):
    """src uint8 [..., H, W] (numpy) -> float64 [..., out, out]: the bicubic value BEFORE clamp and cast"""
    i, j, h, w = box
    crop = src[..., i:i + h, j:j + w].astype(np.float64)
    yi, yw = _axis64(h, out)
    xi, xw = _axis64(w, out)
    tmp = (crop[..., :, xi] * xw).sum(-1)                        # [..., h, out]
    return (tmp[..., yi, :] * yw[:, :, None]).sum(-2)            # [..., out, out]


def trunc_u8(v64):
    return np.clip(v64, 0.0, 255.0).astype(np.uint8)             # (astype truncates toward zero)


def _frames(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, shape, dtype=np.uint8))


def _check_against_fp64(name, src, boxes, out, got):
    """every level equals trunc(clamp(v64)) unless v64 lies within 1e-3 of an integer (then one level off is allowed); at most 0.5 % of
    the pixels may lie in that window"""
    n_near = n_tot = 0
    for c, box in enumerate(boxes):
        v = ref64(src[c].numpy(), box, out)
        want = trunc_u8(v).astype(np.int64)
        g = got[c].cpu().numpy().astype(np.int64)
        near = np.abs(v - np.rint(v)) < 1e-3
        diff = np.abs(g - want)
        n_near += int(near.sum())
        n_tot += near.size
        bad = (diff != 0) & ~near
        print(f"{name} clip {c} box {tuple(box)}: {int((diff != 0).sum())} of {near.size} levels differ, {int(near.sum())} within 1e-3 of an integer, "
              f"max level difference {int(diff.max())}, outside the window {int(bad.sum())}")
        assert not bad.any(), (name, c, box, np.argwhere(bad)[:5], v[bad][:5], g[bad][:5])
        assert diff.max() <= 1, (name, c, box, int(diff.max()))
    share = n_near / n_tot
    print(f"{name}: {100 * share:.3f} % of the pixels within 1e-3 of an integer")
    assert share <= 0.005, (name, share)


# (H, W, OUT, frames per clip, one box per clip).  240 x 320 -> 224 (a decoder-sized frame): down- and up-scale per axis, every border touched,
# a 1-pixel-high box, widths that are not multiples of 4, odd left edges, two clips with different boxes in every call.
CASES = [
    ("full frame (down-scale both axes, all four borders) | up-scale both axes", 240, 320, 224, 3, [(0, 0, 240, 320), (10, 7, 100, 150)]),
    ("down x up y, w = 317 | up x down y, w = 101, top and bottom borders", 240, 320, 224, 3, [(5, 3, 120, 317), (0, 100, 240, 101)]),
    ("1-pixel-high box on the bottom border | right border", 240, 320, 224, 3, [(239, 37, 1, 283), (60, 189, 131, 131)]),
    ("left and bottom borders | 1-pixel-wide box", 240, 320, 224, 2, [(150, 0, 90, 200), (3, 319, 200, 1)]),
    ("224 x 224 -> 224: sub-frame boxes at unit-ish scale", 224, 224, 224, 3, [(1, 2, 223, 221), (17, 30, 190, 160)]),
    ("strong down-scale: a band needs more source rows than the LDS tile holds (sub-bands)", 1200, 500, 224, 1, [(3, 5, 1190, 490), (0, 0, 1200, 37)]),
    ("OUT % 4 != 0 (byte stores) and an odd frame size", 57, 83, 30, 2, [(0, 0, 57, 83), (20, 11, 9, 70)]),
    ("tiny config: -> 56", 72, 96, 56, 4, [(8, 13, 51, 67), (0, 0, 72, 96)]),
]


@pytest.mark.parametrize("name,H,W,OUT,T,boxes", CASES, ids=[c[0].split(":")[0].split(" |")[0] for c in CASES])
def test_every_level_against_fp64(name, H, W, OUT, T, boxes):
    from mrblip import ops

    src = _frames((len(boxes), T, 3, H, W), seed=H * 7 + W)
    got = ops.crop_resize_u8(src.cuda(), boxes, OUT)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(boxes), T, 3, OUT, OUT)
    _check_against_fp64(name, src, boxes, OUT, got)
    # the flat [F,3,H,W] form with frames_per_clip, an int32 tensor of boxes and a caller-provided output: the same bytes
    out = torch.full((len(boxes) * T, 3, OUT, OUT), 7, dtype=torch.uint8, device="cuda")
    r = ops.crop_resize_u8(src.cuda().view(-1, 3, H, W), torch.tensor(boxes, dtype=torch.int32), OUT, out=out, frames_per_clip=T)
    assert r is out and torch.equal(out.view_as(got), got)
    # ... and through torch.ops
    from mrblip import torch_ops  # noqa: F401
    assert torch.equal(torch.ops.mrblip.crop_resize_u8(src.cuda(), torch.tensor(boxes, dtype=torch.int32), OUT), got)


def test_identity_and_constant_images():
    from mrblip import ops

    for n, T, S in ((2, 3, 224), (1, 2, 56), (1, 1, 30)):
        src = _frames((n, T, 3, S, S), seed=S).cuda()
        assert torch.equal(ops.crop_resize_u8(src, [(0, 0, S, S)] * n, S), src), S      # full-frame box at H = W = OUT: bit for bit
    for val in (0, 1, 127, 254, 255):
        src = torch.full((2, 2, 3, 240, 320), val, dtype=torch.uint8, device="cuda")
        for boxes in ([(0, 0, 240, 320), (10, 7, 100, 150)], [(239, 37, 1, 283), (5, 3, 120, 317)], [(0, 100, 240, 101), (3, 319, 200, 1)]):
            got = ops.crop_resize_u8(src, boxes, 224)
            assert bool((got == val).all()), (val, boxes, got.unique().tolist())


def test_against_the_loader_cpu_path():
    """same box, same frames: no level differs from random_resized_crop_u8 by more than one, and the share that differs is at most twice the
    share at which the CPU path itself differs from the fp64 reference"""
    from lavis.datasets.data_utils import random_resized_crop_params, random_resized_crop_u8
    from mrblip import ops

    for seed, (H, W, OUT) in enumerate([(240, 320, 224), (224, 224, 224), (180, 320, 224)]):
        src = _frames((4, 3, H, W), seed=100 + seed)
        box = random_resized_crop_params(H, W, scale=(0.5, 1.0), rng=random.Random(seed))
        cpu = random_resized_crop_u8(src, OUT, scale=(0.5, 1.0), rng=random.Random(seed))         # draws the same box
        got = ops.crop_resize_u8(src.cuda(), [box], OUT, frames_per_clip=4).cpu()
        want = trunc_u8(ref64(src.numpy(), box, OUT))
        d = (got.int() - cpu.int()).abs()
        share_gpu_cpu = float((d != 0).float().mean())
        share_cpu_ref = float((cpu.numpy() != want).mean())
        share_gpu_ref = float((got.numpy() != want).mean())
        print(f"{H}x{W}->{OUT} box {box}: GPU vs CPU path {100 * share_gpu_cpu:.4f} % of levels differ (max {int(d.max())}); "
              f"CPU path vs fp64 {100 * share_cpu_ref:.4f} %; GPU vs fp64 {100 * share_gpu_ref:.4f} %")
        assert int(d.max()) <= 1
        assert share_gpu_cpu <= 2 * share_cpu_ref, (share_gpu_cpu, share_cpu_ref)


def test_two_launches_give_equal_bytes():
    from mrblip import ops

    src = _frames((2, 30, 3, 240, 320), seed=9).cuda()
    boxes = [(5, 3, 120, 317), (33, 40, 200, 210)]
    a = ops.crop_resize_u8(src, boxes, 224)
    b = ops.crop_resize_u8(src, boxes, 224)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ model and train loop
def _tiny(seed=11):
    import lavis  # noqa: F401
    from lavis.common.config import load_yaml
    from lavis.common.registry import registry

    cls = registry.get_model_class("blip2_mr")
    mcfg = load_yaml(cls.default_config_path("tiny_synthetic")).model
    mcfg.update(dict(task="qformer_freeze_lora", input_time_format="seconds_integers", interleave_data=True, seed=seed))
    return cls.from_config(mcfg)


def _samples(video, crop_box=None):
    from lavis.datasets import SyntheticMomentRetrievalDataset, collate

    ds = SyntheticMomentRetrievalDataset(n_items=2, n_frms=4, image_size=56, duration=60.0)
    s = collate([ds[0], ds[1]])
    s["video"] = video
    if crop_box is not None:
        s["crop_box"] = crop_box
    return s


def _loss_and_grad(samples):
    model = _tiny().train()
    loss = model(samples)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu().clone(), model.trainable_decay.grad.detach().cpu().clone(), model.trainable_no_decay.grad.detach().cpu().clone()


@pytest.mark.parametrize("H,W", [(56, 56), (72, 96)])
def test_model_crop_box_equals_precropped_frames(H, W):
    from mrblip import ops

    frames = _frames((2, 4, 3, H, W), seed=3)
    boxes = torch.tensor([(5, 9, 40, 33), (0, 2, H, W - 2)], dtype=torch.int32)
    pre = ops.crop_resize_u8(frames.cuda(), boxes, 56).cpu()
    assert not torch.equal(pre[:, :, :, :, :], frames[:, :, :, :56, :56])
    l_box, gd_box, gn_box = _loss_and_grad(_samples(frames, boxes))
    l_pre, gd_pre, gn_pre = _loss_and_grad(_samples(pre))
    assert gd_box.abs().sum() > 0
    assert torch.equal(l_box, l_pre) and torch.equal(gd_box, gd_pre) and torch.equal(gn_box, gn_pre)
    if (H, W) == (56, 56):          # the same frames WITHOUT the key are a valid (uncropped) input: a model that ignored crop_box would give this
        l_raw, gd_raw, _ = _loss_and_grad(_samples(frames))
        assert not torch.equal(l_box, l_raw) and not torch.equal(gd_box, gd_raw)


def test_crop_box_with_normalised_frames_is_refused():
    model = _tiny().train()
    frames = torch.randn(2, 4, 3, 56, 56)
    with pytest.raises(ValueError, match="uint8"):
        model(_samples(frames, torch.tensor([(0, 0, 56, 56)] * 2, dtype=torch.int32)))


def test_generate_ignores_crop_box():
    model = _tiny().eval()
    frames = _frames((2, 4, 3, 56, 56), seed=4)
    boxes = torch.tensor([(5, 9, 40, 33), (0, 2, 56, 54)], dtype=torch.int32)
    a = model.generate(_samples(frames), num_beams=2, max_length=6)["raw_prediction"]
    assert model.generate(_samples(frames, boxes), num_beams=2, max_length=6)["raw_prediction"] == a


def _native_loader(path, n_frms, size, sampling="uniform", clip_proposal=None):
    from lavis.datasets.data_utils import load_video

    return load_video(path, n_frms=n_frms, sampling=sampling, clip_proposal=clip_proposal)


def test_train_epoch_look_ahead_crops_each_clip_once(tmp_path, monkeypatch):
    """three steps of MomentRetrievalTask.train_epoch over a .npy dataset with device_crop=True: per-step losses bit-equal to the same loop
    fed the pre-cropped tensors (look-ahead on in both), and one crop launch per clip"""
    import lavis  # noqa: F401
    from lavis.datasets import MomentRetrievalDataset, collate
    from lavis.runners.runner_base import FlatAdamW
    from lavis.tasks.moment_retrieval import MomentRetrievalTask
    from mrblip import ops
    from mrblip.engine import MrBlipEngine

    rs = np.random.RandomState(2)
    for v in range(3):
        np.save(tmp_path / f"vid{v}.npy", rs.randint(0, 256, (40, 72, 96, 3), dtype=np.uint8))
    ann = [{"video": f"vid{k}", "qid": k, "query": ["a person opens the door", "someone sits down", "a dog runs"][k], "duration": 1.3,
            "relevant_windows": [[0, 1]]} for k in range(3)]
    json.dump(ann, open(tmp_path / "train.json", "w"))
    ds = MomentRetrievalDataset(str(tmp_path / "train.json"), str(tmp_path), n_frms=4, image_size=56, frame_loader=_native_loader,
                                crop_scale=(0.5, 1.0), device_crop=True)
    random.seed(21)
    batches = [collate([ds[k]]) for k in range(3)]
    assert all(tuple(b["video"].shape) == (1, 4, 3, 72, 96) and tuple(b["crop_box"].shape) == (1, 4) for b in batches)
    assert len({tuple(b["crop_box"][0].tolist()) for b in batches}) == 3
    # (the frame dump is [N,H,W,3]: without a resize the loader hands on a permuted view, which the op itself refuses)
    pre = [dict(b, video=ops.crop_resize_u8(b["video"].cuda().contiguous(), b["crop_box"], 56).cpu()) for b in batches]
    for b in pre:
        del b["crop_box"]

    real, calls = ops.crop_resize_u8, []

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "crop_resize_u8", counted)

    class Sched:
        def step(self, cur_epoch, cur_step):
            pass

    class Task(MomentRetrievalTask):
        def train_step(self, model, samples):
            loss = super().train_step(model, samples)
            self.losses.append(loss.detach().clone())
            return loss

    def run(loader):
        model = _tiny()
        model.begin_accumulation(1.0)
        task = Task()
        task.losses = []
        hits0, miss0 = MrBlipEngine.vit_prefetch_hits, MrBlipEngine.vit_prefetch_misses
        task.train_epoch(0, model, [dict(b) for b in loader], FlatAdamW(model, lr=1e-3, weight_decay=0.05), Sched(), log_freq=1)
        torch.cuda.synchronize()
        assert MrBlipEngine.vit_prefetch_hits - hits0 == 2 and MrBlipEngine.vit_prefetch_misses == miss0      # the look-ahead was on
        return [l.cpu() for l in task.losses]

    la = run(batches)
    assert len(calls) == 3, len(calls)                  # step 0 crops its own clip and the next one, step 1 the third, step 2 nothing
    lb = run(pre)
    assert len(calls) == 3                              # pre-cropped frames never reach the op
    print("losses with crop_box", [float(x) for x in la], "pre-cropped", [float(x) for x in lb])
    assert len(la) == len(lb) == 3 and all(torch.equal(x, y) for x, y in zip(la, lb))
    assert not torch.equal(la[0], la[1])
