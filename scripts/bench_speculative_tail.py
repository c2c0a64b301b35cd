"""What a speculative pass under a configured tail costs, with scripts/bench_speculative.py's method on the same 8B int4 g64
geometry with synthetic weights: every figure is the median of --reps windows of --window calls after one warm-up window, with the spread
(max - min) of the windows, all forms alternating in one process.

Acceptance is FORCED to "all": before a pass the samplers' stream position is put back to one fixed value, so row r draws the same token
every time, and the draft is built from the pass's own tokens, one position per pass, until every draft is accepted.  Forms:
    step <tail>          the replayed step under the tail, queued back to back with one synchronise per window
    pass <tail> m=M      one Model.spec_step_tail over M + 1 rows (Model.spec_step for the greedy tail), the next draft queued behind it, ONE
                         read-back, from a rewound state (cache trimmed, device-side offset and token restored, stream position restored:
                         two small launches, inside the window)
Tails: greedy (the raw tail: spec_step) | top_p | top_k (the sampler's 5-launch modes) | top_p+penalty (the edit launch too).
break_even_tokens = pass_ms / step_ms of the SAME tail: the tokens a pass must yield to match that tail's plain step; vs_greedy_pass =
pass_ms / the greedy pass's at the same M: what the tail's launches add to a pass.

    python scripts/bench_speculative_tail.py [--drafts 5,7,15] [--reps 5] [--window 20] [--context 512] [--out FILE]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from proxy_inference_engine_amd import _ffi  # noqa: E402
from proxy_inference_engine_amd.cache import ReusableKVCache  # noqa: E402
from proxy_inference_engine_amd.models.llama import Model, ModelArgs  # noqa: E402
from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint  # noqa: E402
from proxy_inference_engine_amd.samplers import _rng  # noqa: E402

TAILS = {"greedy": {}, "top_p": dict(sampler=("top_p", 0.8, 0.9, 0)), "top_k": dict(sampler=("top_k", 0.8, 0.0, 40)),
         "top_p+penalty": dict(sampler=("top_p", 0.8, 0.9, 0), repetition_penalty=1.1, context_size=60)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drafts", default="5,7,15")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--context", type=int, default=512)
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
    _rng.seed(7)
    counter = _rng.hip_state(model.device)[1]
    fixed = torch.tensor([1000, 0], dtype=torch.int64, device="cuda")          # the stream position every pass starts from

    cache = [ReusableKVCache() for _ in model.layers]
    model.step(prompt, cache)
    fed = int(model.history[o].item())                                         # the token fed at position o, whatever the tail

    def rewind():
        """Back to the state behind the prompt: offset o, `fed` about to be fed, the stream at its fixed position."""
        for c in cache:
            c.trim(c.offset - o)
        _ffi.check(lib.pie_decoder_set_state(model._dec, o, fed, _ffi.stream()))
        model._kv.offset = o
        counter.copy_(fixed)

    def one_pass(tail, d, then_draft=None):
        return (model.spec_step if tail == "greedy" else model.spec_step_tail)(d, cache, then_draft=then_draft)

    accepted_draft: dict = {}

    def full_draft(tail, m):
        """A draft of m ids that a pass over m + 1 rows under `tail` accepts whole from the fixed stream position: the pass's own token
        takes the place of the first rejected draft, one position per pass (row r's token depends on the drafts before it only)."""
        if (tail, m) not in accepted_draft:
            model.set_step_tail(**TAILS[tail])
            d = torch.zeros(m, dtype=torch.int32, device="cuda")
            for _ in range(m + 1):
                rewind()
                tokens, n, _ = one_pass(tail, d)
                if n == m + 1:
                    break
                d[n - 1] = tokens[n - 1]
            assert n == m + 1, f"no fully accepted draft of {m} ids found under {tail}"
            accepted_draft[(tail, m)] = d.clone()
        return accepted_draft[(tail, m)]

    seen: dict = {}

    def pass_window(tail, m):
        name = f"pass {tail} m={m}"
        seen[name] = set()
        d = full_draft(tail, m)

        def prepare():
            model.set_step_tail(**TAILS[tail])

        def run():
            for _ in range(args.window):
                rewind()
                seen[name].add(one_pass(tail, d, then_draft=(3, 1, m))[1])
        return prepare, run

    def step_window(tail):
        def prepare():                                                         # a changed tail drops the captured step: captured again here, outside the window
            model.set_step_tail(**TAILS[tail])
            rewind()
            model.step(None, cache)

        def run():
            rewind()
            for _ in range(args.window):
                model.step(None, cache)
        return prepare, run

    windows = {}
    for tail in TAILS:
        windows[f"step {tail}"] = step_window(tail)
        for m in drafts:
            windows[f"pass {tail} m={m}"] = pass_window(tail, m)
    ms = {k: [] for k in windows}
    for rnd in range(args.reps + 1):                                           # round 0 warms every shape; then the forms alternate
        for name, (prepare, run) in windows.items():
            prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if rnd:
                ms[name].append((time.perf_counter() - t0) * 1e3 / args.window)
    model.set_step_tail()
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    results = []
    for name in windows:
        kind, tail = name.split()[:2]
        row = {"form": name, "tail": tail, "ms_median": round(med[name], 4), "ms_spread": round(spread[name], 4)}
        if kind == "pass":
            m = int(name.split("=")[1])
            step = med[f"step {tail}"]
            row.update(num_draft=m, tokens_yielded=sorted(seen[name]), tokens_per_s=round((m + 1) / med[name] * 1e3, 1),
                       break_even_tokens=round(med[name] / step, 2), vs_step_fully_accepted=round((m + 1) / med[name] * step, 3),
                       vs_greedy_pass=round(med[name] / med[f"pass greedy m={m}"], 4), added_ms_vs_greedy_pass=round(med[name] - med[f"pass greedy m={m}"], 4))
        else:
            row["tokens_per_s"] = round(1e3 / med[name], 1)
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps({"model": "llama3-8b int4 g64 bf16 (synthetic weights)", "context": o, "reps": args.reps, "window": args.window,
                                              "acceptance": "forced: every draft accepted", "tails": {k: {a: list(b) if isinstance(b, tuple) else b for a, b in v.items()} for k, v in TAILS.items()},
                                              "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
