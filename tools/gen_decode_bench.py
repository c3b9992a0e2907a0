"""Whole ``BLIP2_MR.generate`` calls at the QVH shape (60 frames, flan-t5-xl geometry, random weights; 5 beams, max_length 50) with the
device-resident search (the baseline), with the fused cached self-attention of the decode step on top (``generate_fused_decode``) and
with the decoder part of every step replayed as a captured graph on top of that (``generate_graph_decode``), interleaved in one process —
the protocol of tools/gen_search_bench.py:

    python tools/gen_decode_bench.py [--reps 7] [--warmup 2] [--batches 1,4] [--out profiles/gen_fused_decode.json]

Per setting and batch size: wall milliseconds per generate call (median, min, max over the repetitions), decoding steps run, C-ABI
calls the host makes per decoder step (a replayed step makes none: its launches are the graph's), host milliseconds spent enqueueing the
decoder steps, host milliseconds of the whole decoding loop (search launches, polling and the one blocking transfer of finalize included)
and the graph captures / replays of the call.  Nothing is asserted: the defaults stay off whatever the numbers say."""
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

SETTINGS = (("device", False, False), ("device+fused", True, False), ("device+fused+graph", True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--max-length", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_fused_decode.json"))
    args = ap.parse_args()

    import bench
    import lavis  # noqa: F401
    from lavis.common.registry import registry
    from mrblip import ops
    from mrblip.engine import EngineConfig
    from mrblip.tokenizer import FixtureTokenizer

    dev = torch.device("cuda:0")
    wl = bench.WORKLOADS["qvh"]
    cls = registry.get_model_class("blip2_mr")
    model = cls(engine_config=EngineConfig.flan_t5_xl_qvh(mean_pool=False), synthetic_weights=True, tokenizer=FixtureTokenizer(),
                interleave_data=True, task="qformer_freeze_lora", input_time_format="seconds_integers", seed=42, device=dev).eval()
    eng = model.engine

    # decoder steps: host time and C-ABI calls inside them; decoding loop: host time of the whole of _device_beam_search
    acc = {"step_s": 0.0, "launches": 0, "steps": 0, "loop_s": 0.0}

    def timed(fn):
        def wrapped(*a, **kw):
            n0, t0 = ops.launch_count, time.perf_counter()
            r = fn(*a, **kw)
            acc["step_s"] += time.perf_counter() - t0
            acc["launches"] += ops.launch_count - n0
            acc["steps"] += 1
            return r
        return wrapped

    eng.t5_decode_step = timed(eng.t5_decode_step)
    eng.t5_decode_step_graph = timed(eng.t5_decode_step_graph)
    plain_loop = model._device_beam_search

    def timed_loop(*a, **kw):
        t0 = time.perf_counter()
        r = plain_loop(*a, **kw)
        acc["loop_s"] = time.perf_counter() - t0
        return r

    model._device_beam_search = timed_loop
    model.generate_device_search = True
    result = {"shape": dict(workload="qvh", frames=wl["T"], beams=args.beams, max_length=args.max_length, weights="random (seeded)"),
              "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "runs": []}
    for B in [int(b) for b in args.batches.split(",")]:
        samples = bench.synthetic_samples(B, wl["T"], wl["duration"], dev, 1234)
        rows = {name: [] for name, _, _ in SETTINGS}
        seqs = {}
        for rep in range(args.warmup + args.reps):
            for name, fused, graph in SETTINGS:          # interleaved: every setting sees the same clock and cache history
                model.generate_fused_decode, model.generate_graph_decode = fused, graph
                acc.update(step_s=0.0, launches=0, steps=0, loop_s=0.0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.generate(samples, num_beams=args.beams, max_length=args.max_length, min_length=1)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                st = model.last_generate_stats
                seqs[name] = [s.tolist() for s in model.last_sequences]
                if rep >= args.warmup:
                    rows[name].append(dict(ms=ms, steps=st["steps"], launches_per_step=acc["launches"] / max(acc["steps"], 1),
                                           decode_host_ms=acc["step_s"] * 1e3, loop_host_ms=acc["loop_s"] * 1e3,
                                           search_host_ms=st["search_host_s"] * 1e3, captures=st["graph_captures"], replays=st["graph_replays"]))
        model.generate_fused_decode = model.generate_graph_decode = False
        base = statistics.median(r["ms"] for r in rows["device"])
        for name, _, _ in SETTINGS:
            ms = [r["ms"] for r in rows[name]]
            last = rows[name][-1]
            entry = dict(setting=name, B=B, wall_ms_median=statistics.median(ms), wall_ms_min=min(ms), wall_ms_max=max(ms),
                         over_device_search=statistics.median(ms) / base, steps=last["steps"], c_abi_calls_per_decoder_step=last["launches_per_step"],
                         decode_host_ms_median=statistics.median(r["decode_host_ms"] for r in rows[name]),
                         loop_host_ms_median=statistics.median(r["loop_host_ms"] for r in rows[name]),
                         search_host_ms_median=statistics.median(r["search_host_ms"] for r in rows[name]),
                         graph_captures_last_call=last["captures"], graph_replays_last_call=last["replays"],
                         same_token_ids_as_device_search=seqs[name] == seqs["device"], wall_ms_all=[round(m, 2) for m in ms])
            result["runs"].append(entry)
            print(json.dumps(entry))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
