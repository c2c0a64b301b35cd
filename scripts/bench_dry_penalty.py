"""What the DRY penalty costs, on the 8B int4 model.

1. The stand-alone kernel (k_logits_dry, one 1024-thread workgroup) at V = 128256, microseconds per launch, for four windows:
       random64 / random1024   ids over a 50000-id alphabet: no candidate
       alphabet4               1024 ids over 4 symbols: about 256 candidates, short matches
       all_equal               1024 equal ids: 1023 candidates, every one matched to the cap of 64 -- the degenerate case
   next to pie_logprobs_argmax on the same vector (k_logits_stats + k_logits_finish: the tail's own two launches).
2. The replayed decode step with DRY armed against the same step without: ms per step and kernel nodes of the captured graph.
3. step_batch at 8 and 32 sequences with every row armed, against the same step with nothing armed.
Method: every figure is the median of --windows windows; the forms of one comparison alternate inside every window, in an order that
flips from window to window, in this one process.  The spread (min .. max over the windows) is reported beside each median.

    python scripts/bench_dry_penalty.py [--batches 8,32] [--windows 7] [--steps 16] [--out profiles/dry_penalty_bench.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from proxy_inference_engine_amd import hip_ops  # noqa: E402
from proxy_inference_engine_amd.models.llama import Model, ModelArgs  # noqa: E402
from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint  # noqa: E402

DRY = (0.8, 1.75, 2, 1024, ())


def stat(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def kernel_times(V: int, windows: int) -> dict:
    g = torch.Generator().manual_seed(3)
    wins = {"random64": torch.randint(0, 50000, (64,), generator=g), "random1024": torch.randint(0, 50000, (1024,), generator=g),
            "alphabet4": torch.randint(0, 4, (1024,), generator=g), "all_equal": torch.full((1024,), 7)}
    wins = {k: v.to(torch.int32).cuda() for k, v in wins.items()}
    logits = torch.randn(V, device="cuda").to(torch.bfloat16)
    forms = {k: (lambda w=w: hip_ops.logits_dry_penalty(logits, w, 1e-3, 1.0, 2)) for k, w in wins.items()}   # (a tiny penalty with base 1: the logits stay finite over the launches)
    forms["logprobs_argmax"] = lambda: hip_ops.logprobs_argmax(logits)
    samples = {k: [] for k in forms}
    names = list(forms)
    for f in forms.values():
        for _ in range(20):
            f()
    for wnd in range(windows):
        for name in (names if wnd % 2 == 0 else names[::-1]):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(100):
                forms[name]()
            t1.record()
            torch.cuda.synchronize()
            samples[name].append(t0.elapsed_time(t1) * 1e3 / 100)
    return {k: stat(v) for k, v in samples.items()}


def alternate(forms: dict, arm, step, windows: int, steps: int) -> dict:
    """forms: name -> argument of arm(); per window every form is armed (4 untimed steps re-capture), then `steps` steps are timed."""
    ms, launches = {k: [] for k in forms}, {}
    names = list(forms)
    for wnd in range(windows):
        for name in (names if wnd % 2 == 0 else names[::-1]):
            launches[name] = arm(forms[name])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    return {k: {"ms_per_step": stat(v), "launches_per_step": launches[k]} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cfg = dict(LLAMA3_8B)
    if args.layers:
        cfg["num_hidden_layers"] = args.layers
    V = cfg["vocab_size"]
    out = {"model": "llama3-8b int4 g64 bf16 (synthetic weights)", "prompt": args.prompt, "steps": args.steps, "windows": args.windows, "dry": list(DRY[:4])}
    out["kernel_us"] = kernel_times(V, args.windows)
    print(json.dumps({"kernel_us": out["kernel_us"]}), flush=True)
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    batches = [int(b) for b in args.batches.split(",")]
    positions = args.prompt + 2 * args.windows * (args.steps + 4) + 16
    pages_per_seq = (positions + 63) // 64 + 1
    g = torch.Generator().manual_seed(1)
    pattern = torch.randint(0, V, (8,), generator=g)
    prompt = pattern.repeat(args.prompt // 8 + 1)[:args.prompt].tolist()     # a periodic prompt: the armed rows have matches to find

    cache = model.make_cache()
    state = {"tokens": model.step(torch.tensor(prompt, dtype=torch.int32), cache)[0].clone()}

    def step1():
        state["tokens"] = model.step(None, cache)[0]

    def arm1(dry):
        model.set_step_tail(dry=dry)
        for _ in range(4):
            step1()
        return model.graph_launches()

    out["step"] = alternate({"none": None, "dry": DRY}, arm1, step1, args.windows, args.steps)
    model.set_step_tail()
    print(json.dumps({"step": out["step"]}), flush=True)

    model.enable_paged_kv(num_pages=max(batches) * pages_per_seq + 4, max_blocks=pages_per_seq)
    out["step_batch"] = {}
    for B in batches:
        caches = [model.make_cache() for _ in range(B)]
        fed = [list(prompt) for _ in range(B)]
        state["tokens"] = model.prefill_batch(fed, caches)[0].clone()

        def stepb():
            state["tokens"] = model.step_batch(state["tokens"], caches)[0].clone()

        def armb(on):
            if on:
                model.set_batch_dry_penalty(B)
                model.write_batch_dry_penalty(list(range(B)), [DRY] * B, fed)   # (the rings restart from the prompt: a timing run, not a generation)
            else:
                model.clear_batch_dry_penalty()
            for _ in range(4):
                stepb()
            return model.batch_graph_launches()

        out["step_batch"][str(B)] = alternate({"none": False, "dry": True}, armb, stepb, args.windows, args.steps)
        model.clear_batch_dry_penalty()
        print(json.dumps({"step_batch": {B: out["step_batch"][str(B)]}}), flush=True)
        for c in caches:
            c[0].page_manager.release()
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
