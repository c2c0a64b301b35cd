"""What a batched speculative pass costs against the replayed multi-sequence step, on the 8B int4 g64 geometry with synthetic
weights and a synthetic cache (the pages hold small random K / V: nothing here depends on what the context says, only on how long it is).

Synthetic weights have no meaningful acceptance rate, so the acceptance is FORCED, as in scripts/bench_speculative.py: the plain greedy
continuation of every sequence is recorded first (replayed step_batch from the context); a draft is that continuation -- with the pass's
own greedy token wherever its many-row arithmetic breaks a near-tie of the synthetic logits the other way -- corrupted at position a, so
the pass accepts exactly a drafts of every sequence and yields a + 1 tokens each (tokens_yielded reports what it really yielded).
For B in --batches, uniform m in --drafts, a in --accepts (and a = all), at --context cached positions per sequence:
    pass_ms         one Model.spec_step_batch (index upload, gather, the pass over B (m + 1) rows, segmented verify, the next drafter launch
                    queued behind it, ONE read-back), every sequence rewound to the context before it (host work, inside the window)
    mixed_ms        the same rows as B prompts continuing their cached sequences through Model.step_mixed: the same GEMMs, with one
                    attention launch per sequence per layer (the chunk launches) where the pass has one per layer
    attn_us         the pass's attention launch(es) of ONE layer alone, at op level, on the same shapes (hip_ops.paged_attn_verify)
against, alternating in the same process,
    step_ms         the replayed step_batch of the same B, queued back to back with one synchronise per window
    step_sync_ms    the same with the tokens read back after every step, as BatchedEngine consumes them
Every figure: the median of --reps windows of --window calls after one warm-up window, with the spread (max - min) of the windows.
break_even = pass_ms / step_sync_ms: the tokens per sequence a pass must yield to match the engine's plain rate; vs_step = (a + 1) / break_even.

    python scripts/bench_speculative_batch.py --context 512 [--batches 2,8,32] [--drafts 3,7] [--accepts 0,2] [--reps 5] [--window 16] [--out FILE]
    python scripts/bench_speculative_batch.py --all [--contexts 512,8192] [--limit 900] --out FILE    # one fresh process per context, each under its own time limit
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def run_all(args):
    """One fresh child per context under its own time limit; the first one that fails or runs out of time ends the run."""
    merged = {"model": "llama3-8b int4 g64 bf16 (synthetic weights, synthetic cache)", "reps": args.reps, "window": args.window, "contexts": {}}
    for ctx in [int(x) for x in args.contexts.split(",") if x]:
        part = Path(args.out).with_suffix(f".ctx{ctx}.json")
        cmd = [sys.executable, __file__, "--context", str(ctx), "--batches", args.batches, "--drafts", args.drafts, "--accepts", args.accepts, "--reps", str(args.reps),
               "--window", str(args.window), "--out", str(part)]
        rc = subprocess.run(cmd, timeout=args.limit).returncode
        if rc != 0:
            print(json.dumps({"context": ctx, "failed": rc}), flush=True)
            return rc
        merged["contexts"][str(ctx)] = json.loads(part.read_text())["results"]
        part.unlink()
    Path(args.out).write_text(json.dumps(merged, indent=1) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--contexts", default="512,8192")
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--batches", default="2,8,32")
    ap.add_argument("--drafts", default="3,7")
    ap.add_argument("--accepts", default="0,2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.all:
        sys.exit(run_all(args))

    from proxy_inference_engine_amd import hip_ops
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

        def rewind():
            for s in seqs:
                s.truncate(o)

        # the plain greedy continuations, recorded first
        tok, cont = first, [first.tolist()]
        for _ in range(max(drafts) + 1):
            tok = model.step_batch(tok, caches)[0].clone()
            cont.append(tok.tolist())
        cont = [[c[s] for c in cont] for s in range(B)]               # cont[s][0] is fed at position o
        rewind()
        full: dict = {}

        def full_draft(m):
            """Drafts [B, m] the pass accepts whole: the plain continuations, with the pass's own token wherever it differs."""
            if m not in full:
                d = torch.tensor([c[1:m + 1] for c in cont], dtype=torch.int32, device="cuda")
                for _ in range(m + 1):
                    n, toks, _ = model.spec_step_batch(first, caches, d, [m] * B)
                    rewind()
                    if all(k == m + 1 for k in n):
                        break
                    for s, (k, t) in enumerate(zip(n, toks)):
                        if k < m + 1:
                            d[s, k - 1] = t[-1]
                assert all(k == m + 1 for k in n), f"no fully accepted drafts of {m} ids found"
                full[m] = d
            return full[m]

        seen: dict = {}
        seq_ids = torch.zeros((B, o + 64), dtype=torch.int32, device="cuda")
        seq_ids[:, :o + 1] = torch.randint(0, V, (B, o + 1), generator=g).to(device="cuda", dtype=torch.int32)
        seq_len = torch.zeros(B, dtype=torch.int32, device="cuda")
        nxt_drafts = torch.zeros((B, max(drafts)), dtype=torch.int32, device="cuda")

        def pass_window(m, a):
            name = f"pass m={m} a={a}"
            seen[name] = set()
            d = full_draft(m).clone()
            if a < m:
                d[:, a] = (d[:, a] + 1) % V

            def run():
                for _ in range(args.window):
                    rewind()
                    seq_len.fill_(o + 1)
                    n = model.spec_step_batch(first, caches, d, [m] * B, seq_ids, seq_len, then_draft=(3, 1, max(drafts), nxt_drafts))[0]
                    seen[name].update(n)
                rewind()
            return run

        def mixed_window(m):
            rows = [cont[s][:m + 1] for s in range(B)]

            def run():
                for _ in range(args.window):
                    rewind()
                    model.step_mixed(None, [], rows, caches)[0].tolist()
                rewind()
            return run

        def step_window(sync):
            def run():
                rewind()
                tok = first
                for _ in range(args.window):
                    tok = model.step_batch(tok, caches)[0]
                    if sync:
                        tok.tolist()
                rewind()
            return run

        def attn_window(m):
            Hq, Hkv, D = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["hidden_size"] // cfg["num_attention_heads"]
            for s in seqs:
                s.reserve(m + 1)
            table = torch.zeros((B, blocks), dtype=torch.int32)
            for i, s in enumerate(seqs):
                table[i, :len(s.pages)] = torch.tensor(s.pages, dtype=torch.int32)
            rewind()
            N = B * (m + 1)
            dev = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")   # noqa: E731
            q = torch.randn((N, Hq, D), device="cuda").to(torch.bfloat16)
            idx = (table.cuda(), dev([r // (m + 1) for r in range(N)]), dev([o + 1 + r % (m + 1) for r in range(N)]), dev([s * (m + 1) for s in range(B + 1)]))

            def run():
                for _ in range(args.window):
                    hip_ops.paged_attn_verify(q, pool.slab[0], pool.size(), *idx, Hkv, D ** -0.5)
            return run

        windows = {"step": step_window(False), "step_sync": step_window(True)}
        for m in drafts:
            windows[f"mixed m={m}"] = mixed_window(m)
            windows[f"attn m={m}"] = attn_window(m)
            for a in sorted({int(x) for x in args.accepts.split(",") if x and int(x) < m} | {m}):
                windows[f"pass m={m} a={a}"] = pass_window(m, a)
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
            if name.startswith("pass"):
                m, a = (int(p.split("=")[1]) for p in name.split()[1:])
                be = med[name] / med["step_sync"]
                row.update(num_draft=m, accepted=a, tokens_yielded=sorted(seen[name]), break_even_tokens=round(be, 2), vs_step=round((a + 1) / be, 3),
                           aggregate_tokens_per_s=round(B * (a + 1) / med[name] * 1e3, 1))
            elif name.startswith("step"):
                row["aggregate_tokens_per_s"] = round(B / med[name] * 1e3, 1)
            results.append(row)
            print(json.dumps(row), flush=True)
        for s in seqs:
            s.release()
    if args.out:
        Path(args.out).write_text(json.dumps({"context": o, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
