"""Whole ``BLIP2_MR.generate`` calls at the QVH shape (60 frames, flan-t5-xl geometry, random weights; max_length 50) on the two decoding
modes that the host sampler serves — nucleus sampling (top_p 0.9, temperature 0.7, repetition penalty 1.2, ``num_captions`` rows per clip)
and one-beam greedy decoding with a repetition penalty — with the host sampler (the default) and with the device-resident sampler
(``generate_device_sample``), interleaved in one process, with the fused decode step off and on:

    python tools/gen_sample_bench.py [--reps 7] [--warmup 2] [--batches 1,4] [--captions 1,5] [--out profiles/gen_device_sample.json]

Per setting: wall milliseconds per generate call (median, min, max over the repetitions), per decoding step, decoding steps run, host
time spent inside the sampler (host path: sample_search minus its step function, i.e. the warps, the full-vocabulary sort and the draw —
the blocking .cpu() of the logits is counted with the step function; device path: the launches of search.step plus finalize's
unpacking), and for the device path the steps that were enqueued after every row had finished.  The two samplers draw from different
generators, so their sequences (and step counts) differ; the penalised greedy sequences must be equal.  Nothing is asserted: the number
decides later whether the default changes."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--captions", default="1,5")
    ap.add_argument("--max-length", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_device_sample.json"))
    args = ap.parse_args()

    import bench
    import lavis  # noqa: F401
    from lavis.common.registry import registry
    from mrblip import search as S
    from mrblip.engine import EngineConfig
    from mrblip.tokenizer import FixtureTokenizer

    dev = torch.device("cuda:0")
    wl = bench.WORKLOADS["qvh"]
    cls = registry.get_model_class("blip2_mr")
    model = cls(engine_config=EngineConfig.flan_t5_xl_qvh(mean_pool=False), synthetic_weights=True, tokenizer=FixtureTokenizer(),
                interleave_data=True, task="qformer_freeze_lora", input_time_format="seconds_integers", seed=42, device=dev).eval()

    # host sampler: time inside sample_search that is not spent in its step function, and its step count
    host = {"search_s": 0.0, "steps": 0}
    plain_sample_search = S.sample_search

    def timed_sample_search(step_fn, *a, **kw):
        inner = [0.0, 0]

        def timed_step(*sa):
            t = time.perf_counter()
            r = step_fn(*sa)
            inner[0] += time.perf_counter() - t
            inner[1] += 1
            return r

        timed_step.takes_parents = getattr(step_fn, "takes_parents", False)
        t0 = time.perf_counter()
        out = plain_sample_search(timed_step, *a, **kw)
        host["search_s"], host["steps"] = time.perf_counter() - t0 - inner[0], inner[1]
        return out

    S.sample_search = timed_sample_search
    result = {"shape": dict(workload="qvh", frames=wl["T"], max_length=args.max_length, weights="random (seeded)",
                            sampling=dict(top_p=0.9, temperature=0.7, repetition_penalty=1.2, top_k=50), greedy=dict(repetition_penalty=1.5)),
              "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "runs": []}
    cases = [("sampling", n) for n in (int(c) for c in args.captions.split(","))] + [("greedy_pen", 1)]
    for B in [int(b) for b in args.batches.split(",")]:
        samples = bench.synthetic_samples(B, wl["T"], wl["duration"], dev, 1234)
        for what, n_cap in cases:
            if what == "sampling":
                kw = dict(use_nucleus_sampling=True, num_beams=1, top_p=0.9, temperature=0.7, repetition_penalty=1.2, num_captions=n_cap)
            else:
                kw = dict(num_beams=1, repetition_penalty=1.5)
            for fused in (False, True):
                model.generate_fused_decode = fused
                rows = {"host": [], "device": []}
                seqs = {}
                for rep in range(args.warmup + args.reps):
                    for mode in ("host", "device"):          # interleaved: both settings see the same clock and cache history
                        model.generate_device_sample = mode == "device"
                        model.sampling_generator = torch.Generator().manual_seed(1000 + rep)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        model.generate(samples, max_length=args.max_length, min_length=1, **kw)
                        torch.cuda.synchronize()
                        ms = (time.perf_counter() - t0) * 1e3
                        st = model.last_generate_stats
                        assert (st is not None) == (mode == "device"), "the setting did not take the route it names"
                        seqs[mode] = [s.tolist() for s in model.last_sequences]
                        if rep >= args.warmup:
                            rows[mode].append(dict(ms=ms, steps=st["steps"] if st else host["steps"],
                                                   search_host_ms=(st["search_host_s"] if st else host["search_s"]) * 1e3,
                                                   steps_after_done=st["steps_after_done"] if st else 0))
                model.generate_device_sample = False
                for mode in ("host", "device"):
                    ms = [r["ms"] for r in rows[mode]]
                    entry = dict(setting=mode, mode=what, B=B, num_captions=n_cap, rows=B * n_cap, fused_decode=fused,
                                 wall_ms_median=statistics.median(ms), wall_ms_min=min(ms), wall_ms_max=max(ms),
                                 steps=[r["steps"] for r in rows[mode]],
                                 wall_ms_per_step_median=statistics.median(r["ms"] / r["steps"] for r in rows[mode]),
                                 search_host_ms_per_step_median=statistics.median(r["search_host_ms"] / r["steps"] for r in rows[mode]),
                                 steps_after_done=rows[mode][-1]["steps_after_done"], wall_ms_all=[round(m, 2) for m in ms])
                    result["runs"].append(entry)
                    print(json.dumps(entry))
                summary = dict(mode=what, B=B, num_captions=n_cap, fused_decode=fused,
                               device_over_host=statistics.median(r["ms"] for r in rows["device"]) / statistics.median(r["ms"] for r in rows["host"]))
                if what == "greedy_pen":
                    summary["same_token_ids"] = seqs["host"] == seqs["device"]
                result["runs"].append(summary)
                print(json.dumps(summary))
        model.generate_fused_decode = False
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
