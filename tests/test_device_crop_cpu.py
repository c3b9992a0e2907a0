"""The device-side crop + bicubic resize (csrc/augment.hip) without a GPU: the export, the host-side argument validation of the C ABI,
the dataset's ``device_crop`` mode (same boxes as the loader-side crop, frames handed on uncropped), the builder key, collate, and the
torch.ops registration."""
import argparse
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096  # a non-null, 4-B aligned "device pointer": every call below is refused before anything could read it


def test_export_in_header_bindings_and_library():
    from mrblip import ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrblip_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mrblip_crop_resize_u8\s*\(", hdr)
    assert "mrblip_crop_resize_u8" in ops.EXPORTS
    assert hasattr(ctypes.CDLL(ops.LIB_PATH), "mrblip_crop_resize_u8")
    assert callable(ops.crop_resize_u8)


def _call(F, H, W, boxes, n_clips, fpc, OUT):
    from mrblip import ops

    flat = [int(v) for b in boxes for v in b]
    ops._chk(ops._crop_resize_u8(FAKE, F, H, W, (ctypes.c_int * max(len(flat), 4))(*flat), n_clips, fpc, FAKE, OUT, None))


@pytest.mark.parametrize("what,args,msg", [
    ("box below the frame", (4, 32, 48, [(20, 0, 13, 48)], 1, 4, 16), "leaves the 32 x 48 frame"),
    ("box right of the frame", (4, 32, 48, [(0, 40, 8, 9)], 1, 4, 16), "leaves the 32 x 48 frame"),
    ("negative corner", (4, 32, 48, [(-1, 0, 8, 8)], 1, 4, 16), "leaves the 32 x 48 frame"),
    ("second box outside", (4, 32, 48, [(0, 0, 32, 48), (1, 0, 32, 48)], 2, 2, 16), "box 1"),
    ("h = 0", (4, 32, 48, [(0, 0, 0, 8)], 1, 4, 16), "height 0"),
    ("w = 0", (4, 32, 48, [(0, 0, 8, 0)], 1, 4, 16), "width 0"),
    ("n_clips > 64", (65, 32, 48, [(0, 0, 8, 8)] * 65, 65, 1, 16), "n_clips = 65"),
    ("n_clips = 0", (4, 32, 48, [], 0, 4, 16), "n_clips = 0"),
    ("F != n_clips * frames_per_clip", (7, 32, 48, [(0, 0, 8, 8)] * 2, 2, 3, 16), "F = 7 is not"),
    ("H > 4096", (1, 4097, 48, [(0, 0, 8, 8)], 1, 1, 16), "4096"),
    ("OUT = 0", (1, 32, 48, [(0, 0, 8, 8)], 1, 1, 0), "OUT = 0"),
])
def test_argument_validation_needs_no_gpu(what, args, msg):
    from mrblip.ops import MrblipError

    with pytest.raises(MrblipError) as e:
        _call(*args)
    assert msg in str(e.value), (what, str(e.value))


def test_python_wrapper_checks_shapes_before_the_device():
    from mrblip import ops

    with pytest.raises(ops.MrblipError, match="frames are not n_clips"):
        ops.crop_resize_u8(torch.zeros(7, 3, 8, 8, dtype=torch.uint8), [[0, 0, 8, 8], [0, 0, 8, 8]], 8, frames_per_clip=3)
    with pytest.raises(ops.MrblipError, match="boxes must be"):
        ops.crop_resize_u8(torch.zeros(2, 2, 3, 8, 8, dtype=torch.uint8), [0, 0, 8, 8], 8)
    with pytest.raises(ops.MrblipError, match="boxes must be"):
        ops.crop_resize_u8(torch.zeros(1, 2, 3, 8, 8, dtype=torch.uint8), torch.tensor([[0.0, 0.0, 8.0, 8.0]]), 8)
    with pytest.raises(ops.MrblipError, match="cuda"):     # a valid request on CPU tensors: refused, there is no CPU fallback
        ops.crop_resize_u8(torch.zeros(1, 2, 3, 8, 8, dtype=torch.uint8), [[0, 0, 8, 8]], 8)


def _clip(tmp_path, H=40, W=56):
    rs = np.random.RandomState(0)
    np.savez(tmp_path / "v.npz", frames=rs.randint(0, 256, (40, H, W, 3), dtype=np.uint8), fps=np.float64(10.0))
    json.dump([{"video": "v", "qid": k, "query": "q", "duration": 4.0, "relevant_windows": [[1, 2]]} for k in range(3)], open(tmp_path / "a.json", "w"))
    return str(tmp_path / "a.json"), str(tmp_path)


def _native_loader(path, n_frms, size, sampling="uniform", clip_proposal=None):
    """frames at their decoded size (the device crop takes any H x W)"""
    from lavis.datasets.data_utils import load_video

    return load_video(path, n_frms=n_frms, sampling=sampling, clip_proposal=clip_proposal)


def test_dataset_device_crop_returns_uncropped_frames_and_the_same_box(tmp_path):
    import lavis  # noqa: F401
    from lavis.datasets import MomentRetrievalDataset, collate
    from lavis.datasets.data_utils import random_resized_crop_params, random_resized_crop_u8

    ann, root = _clip(tmp_path)
    kw = dict(n_frms=4, image_size=32, frame_loader=_native_loader)
    ev = MomentRetrievalDataset(ann, root, **kw)
    host = MomentRetrievalDataset(ann, root, crop_scale=(0.5, 1.0), **kw)
    dev = MomentRetrievalDataset(ann, root, crop_scale=(0.5, 1.0), device_crop=True, **kw)
    assert dev.device_crop is True and host.device_crop is False and ev.device_crop is False
    raw = ev[0]["video"]
    assert tuple(raw.shape) == (4, 3, 40, 56) and "crop_box" not in ev[0]
    for seed in (5, 6, 7):
        random.seed(seed)
        s = dev[0]
        assert torch.equal(s["video"], raw) and s["video"].dtype == torch.uint8          # uncropped
        assert s["crop_box"].dtype == torch.int32 and tuple(s["crop_box"].shape) == (4,)
        assert tuple(s["crop_box"].tolist()) == random_resized_crop_params(40, 56, scale=(0.5, 1.0), rng=random.Random(seed))
        # the loader-side mode is unchanged: same seed, same box, cropped frames, no extra key
        random.seed(seed)
        h = host[0]
        assert "crop_box" not in h and tuple(h["video"].shape) == (4, 3, 32, 32)
        assert torch.equal(h["video"], random_resized_crop_u8(raw, 32, scale=(0.5, 1.0), rng=random.Random(seed)))
        i, j, hh, ww = s["crop_box"].tolist()
        ref = torch.nn.functional.interpolate(raw[:, :, i:i + hh, j:j + ww].float(), size=(32, 32), mode="bicubic", align_corners=False)
        assert torch.equal(h["video"], ref.clamp_(0, 255).to(torch.uint8))              # ... and it is the box the device mode reports
    # device_crop without crop_scale (eval splits) is inert
    assert "crop_box" not in MomentRetrievalDataset(ann, root, device_crop=True, **kw)[0]
    random.seed(1)
    b = collate([dev[0], dev[1]])
    assert b["crop_box"].dtype == torch.int32 and tuple(b["crop_box"].shape) == (2, 4)
    assert tuple(b["video"].shape) == (2, 4, 3, 40, 56)


@pytest.mark.parametrize("flag", [None, False, True])
def test_builder_reads_device_crop(tmp_path, flag):
    import lavis  # noqa: F401
    from lavis.common.config import Config
    from lavis.common.registry import registry

    ann, root = _clip(tmp_path)
    for split in ("train", "val", "test"):
        json.dump(json.load(open(ann)), open(tmp_path / f"{split}.json", "w"))
    path = os.path.join(ROOT, "mr-blip_amd", "lavis", "projects", "mr_BLIP", "train", "qvh.yaml")
    opts = [f"datasets.qvh.build_info.annotations.{s}.storage={tmp_path}/{s}.json" for s in ("train", "val", "test")]
    opts += [f"datasets.qvh.build_info.videos.storage={root}"]
    dcfg = Config(argparse.Namespace(cfg_path=path, options=opts)).datasets_cfg["qvh"]
    assert "device_crop" not in dcfg.vis_processor.train                              # the shipped yaml stays at the default
    if flag is not None:
        dcfg.vis_processor.train.device_crop = flag
    ds = registry.get_builder_class("qvh")(dcfg).build_datasets()
    assert ds["train"].device_crop is bool(flag) and ds["train"].crop_scale == (0.5, 1.0)
    assert ds["val"].device_crop is False and ds["test"].device_crop is False           # eval splits are never cropped


def test_torch_op_schema_fake_shape_and_cpu_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mrblip import torch_ops

    assert "crop_resize_u8" in torch_ops.OPS
    sch = torch.ops.mrblip.crop_resize_u8.default._schema
    assert sch.name == "mrblip::crop_resize_u8" and "!" not in str(sch), str(sch)     # nothing mutated
    assert [a.name for a in sch.arguments] == ["src", "boxes", "out_size", "frames_per_clip"]
    with FakeTensorMode():
        boxes = torch.empty(2, 4, dtype=torch.int32)
        y = torch.ops.mrblip.crop_resize_u8(torch.empty(2, 5, 3, 240, 320, dtype=torch.uint8), boxes, 224)
        assert y.shape == (2, 5, 3, 224, 224) and y.dtype == torch.uint8
        y = torch.ops.mrblip.crop_resize_u8(torch.empty(10, 3, 240, 320, dtype=torch.uint8), boxes, 56, 5)
        assert y.shape == (10, 3, 56, 56) and y.dtype == torch.uint8
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.mrblip.crop_resize_u8(torch.zeros(1, 2, 3, 8, 8, dtype=torch.uint8), torch.tensor([[0, 0, 8, 8]], dtype=torch.int32), 8)
