"""What a speculative verify pass costs against the plain replayed step, on the 8B int4 g64 geometry with synthetic weights.

Synthetic weights have no meaningful acceptance rate, so the acceptance is FORCED: the plain greedy continuation of a seeded prompt is
recorded first; a draft is that continuation -- with the pass's own greedy token wherever the many-row pass's arithmetic breaks a near-tie
of the synthetic logits the other way (full_draft) -- corrupted at position a: the pass then accepts exactly a drafts and yields a + 1 tokens
(tokens_yielded reports what it really yielded).
For num_draft in --drafts and a in --accepts (and a = all):
    pass_ms        one Model.spec_step (gather, many-row pass over num_draft + 1 rows, verify, the next draft queued behind it, ONE read-back),
                   from a rewound state (the cache trimmed back, the device-side offset and token restored: one 1-thread launch, inside the window)
    tokens_per_s   (a + 1) / pass_ms
against, alternating in the same process,
    step_ms        the plain replayed step, queued back to back with one synchronise per window (bench.py's figure)
    step_sync_ms   the same with the token read back after every step, as InferenceEngine.generate consumes it
Every figure: the median of --reps windows of --window calls after one warm-up window, with the spread (max - min) of the windows.
break_even = pass_ms / step_ms: the tokens a pass must yield to match the plain step's rate.
Then the engine end to end on one repetitive synthetic prompt: plain and speculative generation of --tokens tokens, spec_stats.

    python scripts/bench_speculative.py [--drafts 5,7,15] [--accepts 0,1,2,4] [--reps 5] [--window 20] [--context 512] [--tokens 128] [--out FILE]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams, _ffi  # noqa: E402
from proxy_inference_engine_amd.cache import ReusableKVCache  # noqa: E402
from proxy_inference_engine_amd.models.llama import Model, ModelArgs  # noqa: E402
from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drafts", default="5,7,15")
    ap.add_argument("--accepts", default="0,1,2,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cfg = dict(LLAMA3_8B)
    if args.layers:
        cfg["num_hidden_layers"] = args.layers
    V = cfg["vocab_size"]
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    lib = _ffi.load()
    drafts = [int(x) for x in args.drafts.split(",") if x]
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, V, (args.context,), generator=g).to(device="cuda", dtype=torch.int32)
    o = args.context

    # the plain greedy continuation, recorded first
    cache = [ReusableKVCache() for _ in model.layers]
    model.step(prompt, cache)
    for _ in range(max(drafts) + args.window + 1):
        model.step(None, cache)
    cont = model.history[o:o + max(drafts) + 2].tolist()      # cont[0] is fed at position o

    def rewind():
        """Back to the state behind the prompt: offset o, cont[0] about to be fed."""
        for c in cache:
            c.trim(c.offset - o)
        _ffi.check(lib.pie_decoder_set_state(model._dec, o, cont[0], _ffi.stream()))
        model._kv.offset = o

    seen: dict = {}                                           # the tokens each pass form really yielded (a + 1 unless a near-tie of the synthetic weights interferes)

    accepted_draft: dict = {}

    def full_draft(m):
        """A draft of m ids that a pass over m + 1 rows accepts whole.  It starts from the plain continuation; wherever the pass's own
        greedy token differs from it (synthetic weights: near-ties between the step's and the many-row pass's arithmetic), the pass's
        token takes its place, one position per pass, until every draft is accepted."""
        if m not in accepted_draft:
            d = torch.tensor(cont[1:m + 1], dtype=torch.int32, device="cuda")
            for _ in range(m + 1):
                rewind()
                tokens, n, _ = model.spec_step(d, cache)
                if n == m + 1:
                    break
                d[n - 1] = tokens[n - 1]
            assert n == m + 1, f"no fully accepted draft of {m} ids found"
            accepted_draft[m] = d.tolist()
        return accepted_draft[m]

    def pass_window(m, a):
        seen[f"pass m={m} a={a}"] = set()
        d = list(full_draft(m))
        if a < m:
            d[a] = (d[a] + 1) % V
        d = torch.tensor(d, dtype=torch.int32, device="cuda")

        def run():
            for _ in range(args.window):
                rewind()
                seen[f"pass m={m} a={a}"].add(model.spec_step(d, cache, then_draft=(3, 1, m))[1])
        return run

    def step_window(sync):
        def run():
            rewind()
            for _ in range(args.window):
                tok = model.step(None, cache)[0]
                if sync:
                    tok.item()
        return run

    windows = {"step": step_window(False), "step_sync": step_window(True)}
    for m in drafts:
        for a in sorted({int(x) for x in args.accepts.split(",") if x and int(x) < m} | {m}):
            windows[f"pass m={m} a={a}"] = pass_window(m, a)
    ms = {k: [] for k in windows}
    for rnd in range(args.reps + 1):                          # round 0 warms every shape; then the forms alternate
        for name, fn in windows.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                ms[name].append((time.perf_counter() - t0) * 1e3 / args.window)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    results = []
    for name in windows:
        row = {"form": name, "ms_median": round(med[name], 4), "ms_spread": round(spread[name], 4)}
        if name.startswith("pass"):
            m, a = (int(p.split("=")[1]) for p in name.split()[1:])
            row.update(num_draft=m, accepted=a, tokens_yielded=sorted(seen[name]), tokens_per_s=round((a + 1) / med[name] * 1e3, 1), break_even_tokens=round(med[name] / med["step"], 2),
                       vs_step=round((a + 1) / med[name] * med["step"], 3))
        else:
            row["tokens_per_s"] = round(1e3 / med[name], 1)
        results.append(row)
        print(json.dumps(row), flush=True)

    # the engine end to end on one repetitive prompt
    base = torch.randint(0, V, (32,), generator=g)
    rep_prompt = base.repeat(8)

    def generate(**kw):
        eng = InferenceEngine(model=model)
        eng.prepare_engine(rep_prompt, temp=0)
        list(eng.generate(rep_prompt, max_completion_tokens=8, **kw))             # warm-up (and the prompt cache's prefix for the timed run)
        eng.prompt_cache.cache, eng.prompt_cache.computed_ids = [], []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = [t for t, _ in eng.generate(rep_prompt, max_completion_tokens=args.tokens, **kw)]
        torch.cuda.synchronize()
        return toks, time.perf_counter() - t0, getattr(eng, "spec_stats", None)

    plain, t_plain, _ = generate()
    spec, t_spec, stats = generate(speculative=SpeculativeParams())
    e2e = {"form": "engine", "prompt": "32 random ids x 8", "tokens": len(plain), "same_tokens": plain == spec, "plain_s": round(t_plain, 4), "speculative_s": round(t_spec, 4),
           "plain_tokens_per_s": round(len(plain) / t_plain, 1), "speculative_tokens_per_s": round(len(spec) / t_spec, 1), "spec_stats": stats}
    print(json.dumps(e2e), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps({"model": "llama3-8b int4 g64 bf16 (synthetic weights)", "context": o, "reps": args.reps, "window": args.window,
                                              "results": results, "engine": e2e}, indent=1) + "\n")


if __name__ == "__main__":
    main()
