"""What the frequency / presence penalties cost inside the passes and what they replace, on the 8B int4 model with 128-token
prompts: ms per step and kernel launches per step at B sequences, every request with frequency_penalty 0.5 and presence_penalty 0.5, in
three forms that alternate on the one device inside every round:
    none    nothing set (B = 1: Model.step's greedy graph; B > 1: step_batch's)
    fused   the penalties inside the pass (B = 1: Model.set_step_tail; B > 1: Model.set_batch_count_penalty), one graph replay per step
    host    today's alternative for the same requests: the unconfigured step, then per row hip_ops.logits_count_penalty_rows on the row
            (its counts kept on the device by the op's own counting rule) and hip_ops.logprobs_argmax of the processed row
Best of --rounds rounds of --steps steps, the forms interleaved in chunks of 16 steps whose order flips (a step's attention grows with the
context, and every timed step advances it: this way every form sees the same mean context).  Launches: the kernel nodes of the captured graph, plus for `host` the launches of the ops it
calls per step (the op 1, pie_logprobs_argmax 2, per row).  `op_us`: the stand-alone op on a [B, V] block, 200 launches back to back between
two events -- an upper bound of the kernel's own time next to its traffic (8 bytes per vocabulary element and row); where it does not grow
with B the host's launch rate is what it shows.

    python scripts/bench_count_penalty.py [--batches 1,8,32] [--steps 64] [--rounds 3] [--out profiles/count_penalty_bench.json]
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

FREQ, PRES = 0.5, 0.5


def op_alone_us(B: int, V: int, dtype) -> float:
    """The op on a [B, V] block whose counts are a tenth non-zero, nothing counted: microseconds per launch."""
    logits = torch.randn((B, V), device="cuda").to(dtype)
    counts = (torch.rand((B, V), device="cuda") < 0.1).to(torch.int32)
    records = hip_ops.count_penalty_records([hip_ops.count_penalty_pack(FREQ, PRES, 0)] * B, "cuda")
    for _ in range(20):
        hip_ops.logits_count_penalty_rows(logits, records, counts)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(200):
        hip_ops.logits_count_penalty_rows(logits, records, counts)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
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
    # every timed loop advances the sequences: 3 forms x rounds x chunks x (16 timed + 5 untimed steps), plus the last re-arming
    positions = args.prompt + 16 + 3 * args.rounds * max(2, args.steps // 32 * 2) * 21
    pages_per_seq = (positions + 63) // 64 + 1
    model.enable_paged_kv(num_pages=max(batches) * pages_per_seq + 4, max_blocks=pages_per_seq)
    g = torch.Generator().manual_seed(1)
    results = []

    for B in batches:
        prompts = [torch.randint(0, V, (args.prompt,), generator=g).tolist() for i in range(B)]
        state = {}
        if B == 1:
            cache = model.make_cache()
            state["tokens"] = model.step(torch.tensor(prompts[0], dtype=torch.int32), cache)[0].clone()

            def plain_step():
                state["tokens"], state["logprobs"], state["logits"] = model.step(None, cache)

            def fed_step():   # the host form feeds the token it chose: an explicit id, copied into the replayed step's state
                state["tokens"], state["logprobs"], state["logits"] = model.step(state["tokens"].reshape(1), cache)

            def arm(on: bool) -> int:
                if on:  # (the counting state follows the sequence: from here on, nothing generated before)
                    model.set_step_tail(frequency_penalty=FREQ, presence_penalty=PRES, count_start=int(cache[0].offset))
                else:
                    model.set_step_tail()
                for _ in range(4):
                    plain_step()
                return model.graph_launches()
        else:
            caches = [model.make_cache() for _ in range(B)]
            state["tokens"] = model.prefill_batch(prompts, caches)[0].clone()

            def plain_step():
                state["tokens"], state["logprobs"], state["logits"] = model.step_batch(state["tokens"], caches)

            fed_step = plain_step

            def arm(on: bool) -> int:
                if on:
                    model.set_batch_count_penalty(B)
                    model.write_batch_count_penalty(list(range(B)), [(FREQ, PRES, int(c[0].offset)) for c in caches])
                else:
                    model.clear_batch_count_penalty()
                for _ in range(4):
                    plain_step()
                return model.batch_graph_launches()

        host_records = hip_ops.count_penalty_records([hip_ops.count_penalty_pack(FREQ, PRES, 0)] * B, "cuda")
        host_counts = torch.zeros((B, V), dtype=torch.int32, device="cuda")
        pos = torch.zeros(1, dtype=torch.int32, device="cuda")

        def host_step():
            fed = state["tokens"].reshape(-1).to(torch.int32)
            fed_step()
            logits = state["logits"].reshape(B, V)
            pos.add_(1)
            nxt = state["tokens"].clone()
            for i in range(B):   # per row, as a host processor runs: the op (which counts the row's input id), then the log-softmax + argmax
                hip_ops.logits_count_penalty_rows(logits[i:i + 1], host_records[i:i + 1], host_counts[i:i + 1], fed[i:i + 1], pos)
                tok, _ = hip_ops.logprobs_argmax(logits[i])
                nxt[i:i + 1] = tok
            state["tokens"] = nxt

        # Every timed step advances the sequences, and a step's attention grows with the context (131 KB of K / V per position and sequence
        # on this model): forms timed one after the other would be compared at different contexts.  So a round is cut into chunks of 16
        # steps, every chunk runs all three forms, and the order flips from chunk to chunk -- over a round every form sees the same mean
        # context.  A switch of form re-captures the graph (4 untimed steps).
        best, launches = {}, {}
        chunk = 16
        n_chunks = max(2, args.steps // chunk // 2 * 2)
        for rnd in range(args.rounds):
            total = {"none": 0.0, "fused": 0.0, "host": 0.0}
            for k in range(n_chunks):
                order = ("none", "fused", "host") if k % 2 == 0 else ("host", "fused", "none")
                for form in order:
                    launches[form] = arm(form == "fused") + (3 * B if form == "host" else 0)
                    step = host_step if form == "host" else plain_step
                    step()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(chunk):
                        step()
                    torch.cuda.synchronize()
                    total[form] += time.perf_counter() - t0
            for form, t in total.items():
                best[form] = min(best.get(form, 1e9), t / (n_chunks * chunk))
        arm(False)
        us = op_alone_us(B, V, torch.bfloat16)
        for form, t in best.items():
            row = {"sequences": B, "form": form, "ms_per_step": round(t * 1e3, 3), "tokens_per_s": round(B / t, 1), "launches_per_step": launches[form],
                   "vs_none": round(t / best["none"], 3), "added_us_per_step": round((t - best["none"]) * 1e6, 1)}
            if form == "fused":
                row["op_us"], row["op_traffic_bytes"] = round(us, 2), 8 * V * B
            results.append(row)
            print(json.dumps(row), flush=True)
        if B > 1:
            for c in caches:
                c[0].page_manager.release()
    if args.out:
        Path(args.out).write_text(json.dumps({"model": "llama3-8b int4 g64 bf16 (synthetic weights)", "prompt": args.prompt, "steps": args.steps,
                                              "rounds": args.rounds, "frequency_penalty": FREQ, "presence_penalty": PRES, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
