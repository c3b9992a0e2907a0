"""The train processor's crop + bicubic resize on the loader's CPU against the device kernel (csrc/augment.hip), at the QVH shape
(one clip = 60 x 3 x 224 x 224 uint8) with boxes at scale 0.5, 0.75 and 1.0:

    python tools/crop_bench.py [--launches 30] [--cpu-reps 5] [--step-reps 3] [--steps 8] [--no-step] [--out profiles/device_crop.json]

Records (nothing is asserted; the switch stays opt-in whatever the numbers say):
  * CPU milliseconds per clip of lavis.datasets.data_utils.random_resized_crop_u8 with 1 and with 16 threads, on this host;
  * microseconds of ops.crop_resize_u8 from HIP events: warm-up, then the median of --launches launches;
  * microseconds of ops.patchify (uint8 frames) from the same run — the yardstick for an HBM-bound side kernel on this box;
  * the whole train step (Blip2MR.forward + backward + AdamW, flan-t5-xl geometry, random weights) fed uncropped frames + ``crop_box``
    against the same step fed frames pre-cropped by the op, interleaved, --step-reps repetitions of --steps steps each."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mr-blip_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

T, IMG = 60, 224
SCALES = (0.5, 0.75, 1.0)


def event_us(fn, launches, warmup=5):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return dict(median_us=statistics.median(us), min_us=us[0], max_us=us[-1], launches=launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--no-step", action="store_true", help="kernels and CPU only (skips building the flan-t5-xl sized model)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_crop.json"))
    args = ap.parse_args()
    assert args.launches >= 20 and args.step_reps >= 3

    from lavis.datasets.data_utils import random_resized_crop_params, random_resized_crop_u8
    from mrblip import ops

    dev = torch.device("cuda:0")
    frames = torch.randint(0, 256, (T, 3, IMG, IMG), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))
    result = {"shape": dict(frames=T, H=IMG, W=IMG, out=IMG, dtype="uint8"), "device": torch.cuda.get_device_name(0),
              "host_cpus_used": [1, 16], "boxes": []}

    d_frames = frames.to(dev)
    d_out = torch.empty_like(d_frames)
    for s in SCALES:
        box = random_resized_crop_params(IMG, IMG, scale=(s, s), rng=random.Random(0))
        row = dict(scale=s, box=list(box))
        for nt in (1, 16):
            torch.set_num_threads(nt)
            random_resized_crop_u8(frames, IMG, scale=(s, s), rng=random.Random(0))
            ms = []
            for _ in range(args.cpu_reps):
                t0 = time.perf_counter()
                ref = random_resized_crop_u8(frames, IMG, scale=(s, s), rng=random.Random(0))    # (draws the same box)
                ms.append((time.perf_counter() - t0) * 1e3)
            row[f"cpu_ms_per_clip_{nt}_threads"] = dict(median=statistics.median(ms), min=min(ms), max=max(ms), reps=args.cpu_reps)
        row["kernel"] = event_us(lambda: ops.crop_resize_u8(d_frames, [box], IMG, out=d_out, frames_per_clip=T), args.launches)
        d = (d_out.cpu().int() - ref.int()).abs()
        row["levels_differing_from_cpu_path"] = dict(share=float((d != 0).float().mean()), max=int(d.max()))
        row["kernel_GBps_read_plus_written"] = (T * 3 * (box[2] * box[3] + IMG * IMG)) / (row["kernel"]["median_us"] * 1e-6) / 1e9
        result["boxes"].append(row)
        print(json.dumps(row))

    patches = torch.empty(T * (IMG // 14) ** 2, 640, dtype=torch.bfloat16, device=dev)
    result["patchify_u8"] = event_us(lambda: ops.patchify(d_frames, patches, 14), args.launches)
    result["patchify_u8"]["GBps_read_plus_written"] = (d_frames.numel() + patches.numel() * 2) / (result["patchify_u8"]["median_us"] * 1e-6) / 1e9
    print(json.dumps(dict(patchify_u8=result["patchify_u8"])))

    if not args.no_step:
        import bench
        import lavis  # noqa: F401
        from lavis.common.registry import registry
        from lavis.runners.runner_base import FlatAdamW
        from mrblip.engine import EngineConfig
        from mrblip.tokenizer import FixtureTokenizer

        wl = bench.WORKLOADS["qvh"]
        cls = registry.get_model_class("blip2_mr")
        model = cls(engine_config=EngineConfig.flan_t5_xl_qvh(mean_pool=False), synthetic_weights=True, tokenizer=FixtureTokenizer(),
                    interleave_data=True, task="qformer_freeze_lora", input_time_format="seconds_integers", seed=42, device=dev).train()
        model.begin_accumulation(1.0)
        opt = FlatAdamW(model, lr=3e-4, weight_decay=0.05)
        base = bench.synthetic_samples(1, wl["T"], wl["duration"], torch.device("cpu"), 1234)
        box = torch.tensor([random_resized_crop_params(IMG, IMG, scale=(0.75, 0.75), rng=random.Random(0))], dtype=torch.int32)
        raw = frames.unsqueeze(0).contiguous().pin_memory()
        pre = ops.crop_resize_u8(raw.to(dev), box, IMG).cpu().pin_memory()
        feeds = {"crop_box": dict(base, video=raw, crop_box=box), "pre_cropped": dict(base, video=pre)}

        def run(feed, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                loss = model(dict(feed))["loss"]
                loss.backward()
                opt.step()
                opt.zero_grad()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n, float(loss.detach())

        for feed in feeds.values():      # warm-up: workspaces, graph capture
            run(feed, 6)
        ms = {k: [] for k in feeds}
        for _ in range(args.step_reps):
            for k, feed in feeds.items():   # interleaved: both feeds see the same clock and cache history
                ms[k].append(run(feed, args.steps)[0])
        step = {k: dict(ms_per_step_median=statistics.median(v), ms_per_step_all=[round(x, 3) for x in v]) for k, v in ms.items()}
        step["steps_per_repetition"] = args.steps
        step["box"] = box[0].tolist()
        step["pre_cropped_spread_ms"] = max(ms["pre_cropped"]) - min(ms["pre_cropped"])
        step["crop_box_minus_pre_cropped_ms"] = step["crop_box"]["ms_per_step_median"] - step["pre_cropped"]["ms_per_step_median"]
        step["note"] = "both feeds upload 9 MB of uint8 frames per step from pinned host memory; no look-ahead (one resident clip)"
        result["train_step"] = step
        print(json.dumps(dict(train_step=step)))

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
