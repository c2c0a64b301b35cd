"""What per-row token masks and logit biases cost inside the multi-sequence step and what they replace, on the 8B int4
model: ms per step and kernel launches per step of pie_decoder_step_batch at B sequences with
    none          nothing armed (the greedy tail)
    static_mask   a static mask (every other id) in every row
    fresh_mask    every row's mask rewritten and uploaded before every step, after reading the step's tokens (a grammar's traffic)
    bias          a 300-entry logit_bias in every row
    host_mask     the host form of static_mask: the unarmed step, then hip_ops.logprobs_argmax_masked per row
    host_bias     the host form of bias: the unarmed step, then hip_ops.logits_bias + hip_ops.logprobs_argmax per row
the variants alternating in one process on the one device, best of --rounds rounds of --steps steps.  Launches: the kernel nodes of the
captured graph, plus for the host forms the launches of the ops they call per step (pie_logprobs_argmax_masked 2, pie_logits_bias 1,
pie_logprobs_argmax 2).  No speed-up is promised; the one condition is that `none` does not move.

    python scripts/bench_batch_edits.py [--batches 8,32] [--steps 64] [--rounds 3] [--out profiles/batch_edits_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from proxy_inference_engine_amd import hip_ops  # noqa: E402
from proxy_inference_engine_amd.models.llama import Model, ModelArgs  # noqa: E402
from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint  # noqa: E402

BIAS_ENTRIES = 300
VARIANTS = ["none", "static_mask", "fresh_mask", "bias", "host_mask", "host_bias"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cfg = dict(LLAMA3_8B)
    if args.layers:
        cfg["num_hidden_layers"] = args.layers
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    batches = [int(b) for b in args.batches.split(",")]
    V = cfg["vocab_size"]
    # every timed loop advances the sequences: 6 variants x rounds x (steps + 6 warm-up steps) positions
    positions = args.prompt + 16 + len(VARIANTS) * args.rounds * (args.steps + 6)
    pages_per_seq = (positions + 63) // 64 + 1
    model.enable_paged_kv(num_pages=max(batches) * pages_per_seq + 4, max_blocks=pages_per_seq)
    g = torch.Generator().manual_seed(1)
    even = hip_ops.pack_token_mask(torch.arange(V) % 2 == 0, V)
    odd = hip_ops.pack_token_mask(torch.arange(V) % 2 == 1, V)
    bias_ids = torch.randperm(V, generator=g)[:BIAS_ENTRIES].to(torch.int32)
    bias_vals = torch.randn(BIAS_ENTRIES, generator=g)
    results = []
    for B in batches:
        prompts = [torch.randint(0, V, (args.prompt + (i % 7),), generator=g).tolist() for i in range(B)]
        caches = [model.make_cache() for _ in range(B)]
        tokens, _, _ = model.prefill_batch(prompts, caches)
        state = {"tokens": tokens.clone(), "flip": 0}
        rows = list(range(B))
        dev_even, dev_ids, dev_vals = even.to(model.device), bias_ids.to(model.device), bias_vals.to(model.device)

        def fused_step():
            state["tokens"], _, _ = model.step_batch(state["tokens"], caches)

        def fresh_mask_step():
            state["tokens"].tolist()                                              # a grammar reads the tokens before it can say what comes next
            state["flip"] ^= 1
            model.write_batch_edits(rows, masks=[odd if state["flip"] else even] * B)
            fused_step()

        def host_mask_step():
            nxt, _, logits = model.step_batch(state["tokens"], caches)
            nxt = nxt.clone()
            for i in range(B):
                nxt[i:i + 1] = hip_ops.logprobs_argmax_masked(logits[i], dev_even)[0]
            state["tokens"] = nxt

        def host_bias_step():
            nxt, _, logits = model.step_batch(state["tokens"], caches)
            nxt = nxt.clone()
            for i in range(B):
                hip_ops.logits_bias(logits[i], dev_ids, dev_vals)
                nxt[i:i + 1] = hip_ops.logprobs_argmax(logits[i])[0]
            state["tokens"] = nxt

        def timed(step):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps

        def arm(variant):
            """The edits of a variant (host forms and `none`: off), warmed until the step replays its graph; -> its kernel nodes."""
            if variant in ("static_mask", "fresh_mask"):
                model.set_batch_edits(B, masks=True)
                model.write_batch_edits(rows, masks=[even] * B)
            elif variant == "bias":
                model.set_batch_edits(B, masks=False, bias_cap=BIAS_ENTRIES)
                model.write_batch_edits(rows, biases=[(bias_ids.tolist(), bias_vals.tolist())] * B)
            else:
                model.clear_batch_edits()
            for _ in range(4):
                fused_step()
            return model.batch_graph_launches()

        steps = {"none": fused_step, "static_mask": fused_step, "fresh_mask": fresh_mask_step, "bias": fused_step, "host_mask": host_mask_step,
                 "host_bias": host_bias_step}
        extra = {"host_mask": 2 * B, "host_bias": 3 * B}
        best, launches = {}, {}
        for rnd in range(args.rounds):
            for variant in VARIANTS:                                              # the variants alternate inside every round
                launches[variant] = arm(variant) + extra.get(variant, 0)
                for _ in range(2):
                    steps[variant]()
                best[variant] = min(best.get(variant, 1e9), timed(steps[variant]))
        model.clear_batch_edits()
        for variant in VARIANTS:
            t = best[variant]
            row = {"sequences": B, "variant": variant, "ms_per_step": round(t * 1e3, 3), "tokens_per_s": round(B / t, 1),
                   "launches_per_step": launches[variant], "vs_none": round(t / best["none"], 3)}
            results.append(row)
            print(json.dumps(row), flush=True)
        for c in caches:
            c[0].page_manager.release()
    if args.out:
        Path(args.out).write_text(json.dumps({"model": "llama3-8b int4 g64 bf16 (synthetic weights)", "prompt": args.prompt, "steps": args.steps,
                                              "rounds": args.rounds, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
