"""What a batched speculative pass costs under per-request tails, on the 8B int4 g64 geometry with synthetic weights and a
synthetic cache, by scripts/bench_speculative_batch.py's method: forced acceptance, medians of windows with their spreads.

Every seat draws under top-p (temp 0.8, top_p 0.9) with a repetition penalty (1.1 over 60 ids) and a two-entry logit bias, each seat on
its own seed.  Synthetic weights have no meaningful acceptance rate, so the acceptance is FORCED: a draft is what the pass itself draws
for the row before it -- found by running the pass until every draft is accepted, the seats' records and rings put back before every
call, as they are inside the timed windows (two small device copies, inside the window) -- so the pass accepts all m drafts of every
sequence and yields m + 1 tokens each (tokens_yielded reports what it really yielded).  ACCEPTANCE RATES UNDER REAL SAMPLERS ARE NOT MEASURED HERE.
For B in --batches, uniform m in --drafts, at --context cached positions per sequence:
    tail_pass_ms    one Model.spec_step_batch_tail (index upload, gather, the pass over B (m + 1) rows, the segmented sampled verify, the
                    next drafter launch queued behind it, ONE read-back), every sequence rewound and every seat put back before it
    greedy_pass_ms  Model.spec_step_batch on the same rows with nothing armed (fully accepted drafts of its own)
against, alternating in the same process,
    step_sync_ms    the replayed step_batch of the same B under the same armed tail, its tokens read back after every step, as
                    BatchedEngine consumes them
tail_adds_ms = tail_pass_ms - greedy_pass_ms; break_even = tail_pass_ms / step_sync_ms: the tokens per sequence a pass must yield to
match the engine's plain sampled rate.

    python scripts/bench_speculative_batch_tail.py [--context 512] [--batches 2,8,32] [--drafts 3,7] [--reps 5] [--window 16] [--out profiles/spec_batch_tail_bench.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--batches", default="2,8,32")
    ap.add_argument("--drafts", default="3,7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spec_batch_tail_bench.json"))
    args = ap.parse_args()

    from proxy_inference_engine_amd.engine.batch_engine import SamplingParams
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint
    cfg = dict(LLAMA3_8B)
    if args.layers:
        cfg["num_hidden_layers"] = args.layers
    V, o = cfg["vocab_size"], args.context
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    batches = [int(x) for x in args.batches.split(",") if x]
    drafts = [int(x) for x in args.drafts.split(",") if x]
    blocks = (o + 64 + 63) // 64 + 1
    pool = model.enable_paged_kv(num_pages=max(batches) * blocks + 8, max_blocks=blocks)
    pool.slab.view(torch.bfloat16).normal_(0.0, 0.5)                   # the synthetic cache (the slab is raw bytes)
    g = torch.Generator().manual_seed(1)
    results = []
    for B in batches:
        caches = [model.make_cache() for _ in range(B)]
        seqs = [c[0].page_manager for c in caches]
        for s in seqs:                                                 # o cached positions each, on pages of their own
            s.reserve(o)
            s.advance(o)
        first = torch.randint(0, V, (B,), generator=g).to(device="cuda", dtype=torch.int32)
        fed = torch.randint(0, V, (B, o), generator=g)                  # what the seats' rings hold: o ids each
        params = [SamplingParams(temp=0.8, top_p=0.9, seed=1000 + s, repetition_penalty=1.1, repetition_context_size=60) for s in range(B)]
        biases = [([int(fed[s, 0]), int(fed[s, -1])], [1.0, -1.0]) for s in range(B)]

        def arm():
            bt = model.set_batch_tail(B)
            model.set_batch_edits(B, masks=False, bias_cap=2)
            return bt

        def disarm():
            model.clear_batch_tail(), model.clear_batch_edits()

        bt = arm()
        model.write_batch_tail(list(range(B)), [sp.record(0, sp.seed) for sp in params], [fed[s].tolist() for s in range(B)])
        model.write_batch_edits(list(range(B)), biases=biases)
        table0, recent0 = bt["table"].clone(), bt["recent"].clone()

        def rewind():
            for s in seqs:
                s.truncate(o)
            bt["table"].copy_(table0), bt["recent"].copy_(recent0)

        def full_draft(entry, m):
            """Drafts [B, m] the entry accepts whole: row j's token depends on the drafts before it only, so round j settles draft j."""
            d = torch.zeros((B, m), dtype=torch.int32, device="cuda")
            for _ in range(m + 1):
                rewind()
                n, toks, _ = entry(first, caches, d, [m] * B)
                if all(k == m + 1 for k in n):
                    break
                for s, (k, t) in enumerate(zip(n, toks)):
                    if k < m + 1:
                        d[s, k - 1] = t[-1]
            rewind()
            assert all(k == m + 1 for k in n), f"no fully accepted drafts of {m} ids found"
            return d

        seen: dict = {}
        seq_ids = torch.zeros((B, o + 64), dtype=torch.int32, device="cuda")
        seq_ids[:, :o + 1] = torch.randint(0, V, (B, o + 1), generator=g).to(device="cuda", dtype=torch.int32)
        seq_len = torch.zeros(B, dtype=torch.int32, device="cuda")
        nxt_drafts = torch.zeros((B, max(drafts)), dtype=torch.int32, device="cuda")
        tail_d = {m: full_draft(model.spec_step_batch_tail, m) for m in drafts}
        disarm()
        greedy_d = {m: full_draft(model.spec_step_batch, m) for m in drafts}
        arm()

        def pass_window(name, entry, d, m, armed):
            seen[name] = set()

            def run():
                if not armed:
                    disarm()
                for _ in range(args.window):
                    rewind()
                    seq_len.fill_(o + 1)
                    n = entry(first, caches, d, [m] * B, seq_ids, seq_len, then_draft=(3, 1, max(drafts), nxt_drafts))[0]
                    seen[name].update(n)
                if not armed:
                    arm()
                rewind()
            return run

        def step_window():
            rewind()
            tok = first
            for _ in range(args.window):
                tok = model.step_batch(tok, caches)[0]
                tok.tolist()
            rewind()

        windows = {"step_sync": step_window}
        for m in drafts:
            windows[f"tail_pass m={m}"] = pass_window(f"tail_pass m={m}", model.spec_step_batch_tail, tail_d[m], m, True)
            windows[f"greedy_pass m={m}"] = pass_window(f"greedy_pass m={m}", model.spec_step_batch, greedy_d[m], m, False)
        ms = {k: [] for k in windows}
        for rnd in range(args.reps + 1):                               # round 0 warms every shape; then the forms alternate
            for name, fn in windows.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rnd:
                    ms[name].append((time.perf_counter() - t0) * 1e3 / args.window)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for name in windows:
            row = {"context": o, "B": B, "form": name, "ms_median": round(med[name], 4), "ms_spread": round(max(ms[name]) - min(ms[name]), 4)}
            if name.startswith("tail_pass"):
                m = int(name.split("=")[1])
                be = med[name] / med["step_sync"]
                row.update(num_draft=m, tokens_yielded=sorted(seen[name]), tail_adds_ms=round(med[name] - med[f"greedy_pass m={m}"], 4),
                           break_even_tokens=round(be, 2), vs_step_all_accepted=round((m + 1) / be, 3))
            elif name.startswith("greedy_pass"):
                row.update(num_draft=int(name.split("=")[1]), tokens_yielded=sorted(seen[name]))
            else:
                row["aggregate_tokens_per_s"] = round(B / med[name] * 1e3, 1)
            results.append(row)
            print(json.dumps(row), flush=True)
        disarm()
        for s in seqs:
            s.release()
    if args.out:
        Path(args.out).write_text(json.dumps({"model": "llama3-8b int4 g64 bf16 (synthetic weights, synthetic cache)", "sampler": "top_p 0.9, temp 0.8, repetition_penalty 1.1 / 60, 2 bias entries",
                                              "acceptance": "forced (all drafts accepted); acceptance rates under real samplers are not measured",
                                              "context": o, "reps": args.reps, "window": args.window, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
