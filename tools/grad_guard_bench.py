"""What the gradient guard (csrc/optim.hip) costs per optimizer step, at the real size: the benched engine's flat trainable
buffer (bench.py's flan-t5-xl / QVH engine, random weights), its own gradient / moment buffers, MrBlipEngine.optimizer_step with

    off    the parent's step: hyper upload + 2 AdamW launches (+ refresh_trainable)
    on     grad_guard=True: + grad_sumsq over the flat gradient + optim_prepare
    clip   max_grad_norm below the gradient's norm: the same launches, clip < 1

    python tools/grad_guard_bench.py [--rounds 30] [--burst 10] [--warmup 5] [--out profiles/grad_guard.json]

The three settings are interleaved in ONE process (the order rotates from round to round); a round times, per setting, a burst of --burst
back-to-back steps between two HIP events (so one number covers ~ms of work, not one launch), after --warmup untimed rounds.  The host time
to enqueue a step is recorded beside it: a burst runs at the slower of the two.  The two new kernels are also timed on their own (events
around --burst launches).  Nothing is asserted and no default changes on these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mr-blip_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_COPY_TBPS = 6.29    # MI355X float4 copy, measured (8.0 TB/s spec): the yardstick for one streaming read of the gradient


def summary(us):
    us = sorted(us)
    return dict(median_us=statistics.median(us), min_us=us[0], max_us=us[-1], n=len(us))


def burst_us(fn, burst):
    """(device microseconds per call from two events around `burst` calls, host microseconds per call to enqueue them)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    for _ in range(burst):
        fn()
    host = (time.perf_counter() - t0) * 1e6 / burst
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / burst, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="the tiny engine (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_guard.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "grad_guard_bench needs the GPU: a CPU run measures nothing"

    from mrblip import ops
    from mrblip.engine import EngineConfig, MrBlipEngine, RandomSource

    dev = torch.device("cuda:0")
    cfg = EngineConfig.tiny() if args.tiny else EngineConfig.flan_t5_xl_qvh(mean_pool=False)
    eng = MrBlipEngine(cfg, RandomSource(dev, seed=1234), dev, seed=42)
    n = eng.flat.numel()
    eng.grad.copy_(torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 1e-3)
    norm = float(eng.grad.double().norm())
    settings = {"off": dict(), "on": dict(grad_guard=True), "clip": dict(max_grad_norm=0.5 * norm)}
    calls = {}
    for name, kw in settings.items():       # C-ABI calls of one step
        c0 = ops.launch_count
        eng.optimizer_step(lr=1e-5, weight_decay=0.05, **kw)
        calls[name] = ops.launch_count - c0
    torch.cuda.synchronize()

    dev_us = {k: [] for k in settings}
    host_us = {k: [] for k in settings}
    names = list(settings)
    for r in range(args.warmup + args.rounds):
        for k in range(len(names)):
            name = names[(r + k) % len(names)]
            d, h = burst_us(lambda: eng.optimizer_step(lr=1e-5, weight_decay=0.05, **settings[name]), args.burst)
            if r >= args.warmup:
                dev_us[name].append(d)
                host_us[name].append(h)
    eng.optimizer_step(lr=1e-5, weight_decay=0.05, **settings["clip"])
    st = eng.grad_guard().read()
    assert st["skipped_steps"] == 0 and 0.0 < st["clip"] < 1.0, st      # (a clipping step; none was skipped)

    # the two new launches on their own
    ws = torch.empty(ops.grad_stats_workspace_bytes(n), dtype=torch.uint8, device=dev)
    state = torch.zeros(ops.OPTIM_STATE_WORDS, dtype=torch.int32, device=dev)
    hin, hout = torch.tensor([1e-5, 1.0], device=dev), torch.zeros(4, device=dev)
    k_sumsq, k_prep = [], []
    for r in range(args.warmup + args.rounds):
        a = burst_us(lambda: ops.grad_sumsq(eng.grad, ws), args.burst)[0]
        b = burst_us(lambda: ops.optim_prepare(ws, n, hin, state, hout), args.burst)[0]
        if r >= args.warmup:
            k_sumsq.append(a)
            k_prep.append(b)

    res = {"device": torch.cuda.get_device_name(0), "engine": "tiny (rehearsal)" if args.tiny else "flan-t5-xl / QVH (bench.py's), random weights",
           "flat_numel": n, "n_decay": eng.n_decay, "gradient_MB": 4 * n / 1e6, "chunks": (n + ops.GRAD_CHUNK - 1) // ops.GRAD_CHUNK,
           "gradient_norm": norm, "rounds": args.rounds, "burst": args.burst, "warmup_rounds": args.warmup,
           "timing": "HIP events around a burst of back-to-back optimizer steps; settings interleaved in one process, order rotated per round",
           "settings": {}}
    for name in names:
        res["settings"][name] = dict(c_abi_calls_per_step=calls[name], device_us_per_step=summary(dev_us[name]), host_enqueue_us_per_step=summary(host_us[name]))
    off = res["settings"]["off"]["device_us_per_step"]["median_us"]
    for name in ("on", "clip"):
        res["settings"][name]["median_over_off_us"] = res["settings"][name]["device_us_per_step"]["median_us"] - off
    s = summary(k_sumsq)
    res["kernels"] = {"grad_sumsq": dict(s, read_GBps_at_median=4 * n / (s["median_us"] * 1e-6) / 1e9,
                                         hbm_copy_yardstick_us=4 * n / (HBM_COPY_TBPS * 1e12) * 1e6,
                                         yardstick=f"{HBM_COPY_TBPS} TB/s: measured float4 copy rate of the MI355X (8.0 TB/s spec); a gradient that the "
                                                   "backward has just written may also be served by the 256 MB Infinity Cache"),
                      "optim_prepare": summary(k_prep)}
    print(json.dumps(res, indent=1))
    if not args.tiny:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
