"""What a round of draft-model speculative decoding costs, with scripts/bench_speculative.py's method: the 8B int4 g64
target with synthetic weights, a drafter of the 1B geometry (hidden 2048, 16 layers, 32 / 8 heads of 64, intermediate 8192, V 128256; int4
g64, synthetic weights), a 512-token context.  Every figure is the median of --reps windows of --window calls after one warm-up window,
with the spread (max - min) of the windows, all forms alternating in one process.  Forms, all under one sampler setting (top-p 0.9 at
temperature 0.8) and each from a rewound state (caches trimmed, device-side offsets and tokens restored, stream positions restored):
    step target          the target's replayed step, queued back to back, one synchronise per window
    step drafter         the drafter's replayed step, the same way
    draft k=M            what a round spends drafting: the drafter fed one token, M replayed steps back to back, its bound
                         log-probabilities copied into the [31, V] block behind each, one synchronise
    pass sampled m=M     Model.spec_step_tail over M + 1 rows (DESIGN.md 20's pass), ONE read-back
    pass draft m=M       Model.spec_step_draft over the same rows with the drafter's ids and log-probabilities, ONE read-back
added_ms_vs_sampled_pass = what pie_spec_verify_draft's launches add over pie_spec_verify_sampled's; round_ms = draft + pass draft;
break_even_tokens = round_ms / the target's step: the tokens a round must yield to match the plain loop under the same tail.  Synthetic
weights say nothing about acceptance rates: those stay "not measured" (tokens_yielded reports what these random models happened to do).

    python scripts/bench_speculative_draft.py [--drafts 5,7,15] [--reps 5] [--window 20] [--context 512] [--out FILE]
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

SAMPLER = ("top_p", 0.8, 0.9, 0)
DRAFTER_1B = dict(LLAMA3_8B, hidden_size=2048, num_hidden_layers=16, intermediate_size=8192, num_attention_heads=32, num_key_value_heads=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drafts", default="5,7,15")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--layers", type=int, default=0, help="cut both models to this many layers (a quick check of the script)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cfg_t, cfg_d = dict(LLAMA3_8B), dict(DRAFTER_1B)
    if args.layers:
        cfg_t["num_hidden_layers"] = cfg_d["num_hidden_layers"] = args.layers
    V = cfg_t["vocab_size"]
    target = Model(ModelArgs(**cfg_t), synthetic_checkpoint(cfg_t, seed=0, dtype=torch.bfloat16))
    drafter = Model(ModelArgs(**cfg_d), synthetic_checkpoint(cfg_d, seed=1, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    lib = _ffi.load()
    drafts = [int(x) for x in args.drafts.split(",") if x]
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, V, (args.context,), generator=g).to(device="cuda", dtype=torch.int32)
    o = args.context
    _rng.seed(7)
    counter = _rng.hip_state(target.device)[1]
    dseed, dcounter = _rng.draft_state(drafter.device)
    fixed = torch.tensor([1000, 0], dtype=torch.int64, device="cuda")          # the stream position every form starts from
    target.set_step_tail(sampler=SAMPLER)
    drafter.set_step_tail(sampler=SAMPLER, rng=(dseed, dcounter))
    caches = {id(target): [ReusableKVCache() for _ in target.layers], id(drafter): [ReusableKVCache() for _ in drafter.layers]}
    counter.copy_(fixed), dcounter.copy_(fixed)
    target.step(prompt, caches[id(target)])
    drafter.step(prompt, caches[id(drafter)])
    fed = int(target.history[o].item())                                        # the token both models are fed at position o
    fed_dev = torch.tensor([fed], dtype=torch.int32, device="cuda")
    q_rows = torch.zeros((31, V), dtype=torch.float32, device="cuda")

    def rewind(model):
        """Back to the state behind the prompt: offset o, `fed` about to be fed, the model's stream at its fixed position."""
        cache = caches[id(model)]
        for c in cache:
            c.trim(c.offset - o)
        _ffi.check(lib.pie_decoder_set_state(model._dec, o, fed, _ffi.stream()))
        model._kv.offset = o
        (counter if model is target else dcounter).copy_(fixed)

    def draft(k):
        """A round's drafting, as InferenceEngine._speculative_draft_steps queues it; returns the drafter's ids (a view of its history)."""
        rewind(drafter)
        cache = caches[id(drafter)]
        drafter.step(fed_dev, cache)
        for i in range(k):
            if i:
                drafter.step(None, cache)
            q_rows[i].copy_(drafter.logprobs)
        return drafter.history[o + 1:o + 1 + k]

    seen: dict = {}

    def step_window(model):
        def run():
            rewind(model)
            for _ in range(args.window):
                model.step(None, caches[id(model)])
        return run

    def draft_window(k):
        def run():
            for _ in range(args.window):
                draft(k)
        return run

    def pass_window(kind, m):
        name = f"pass {kind} m={m}"
        seen[name] = set()
        ids = draft(m).clone()                                                 # one draft, verified again and again from the rewound state

        def run():
            for _ in range(args.window):
                rewind(target)
                if kind == "draft":
                    seen[name].add(target.spec_step_draft(ids, q_rows, caches[id(target)], draft_seed=dseed)[1])
                else:
                    seen[name].add(target.spec_step_tail(ids, caches[id(target)])[1])
        return run

    windows = {"step target": step_window(target), "step drafter": step_window(drafter)}
    for m in drafts:
        windows[f"draft k={m}"] = draft_window(m)
        windows[f"pass sampled m={m}"] = pass_window("sampled", m)
        windows[f"pass draft m={m}"] = pass_window("draft", m)
    ms = {k: [] for k in windows}
    for rnd in range(args.reps + 1):                                           # round 0 warms every shape; then the forms alternate
        for name, run in windows.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if rnd:
                ms[name].append((time.perf_counter() - t0) * 1e3 / args.window)
    target.set_step_tail(), drafter.set_step_tail()
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    results = []
    for name in windows:
        row = {"form": name, "ms_median": round(med[name], 4), "ms_spread": round(spread[name], 4)}
        if name.startswith("pass draft"):
            m = int(name.split("=")[1])
            round_ms = med[f"draft k={m}"] + med[name]
            row.update(num_draft=m, tokens_yielded=sorted(seen[name]), added_ms_vs_sampled_pass=round(med[name] - med[f"pass sampled m={m}"], 4),
                       round_ms=round(round_ms, 4), break_even_tokens=round(round_ms / med["step target"], 2),
                       pass_in_target_steps=round(med[name] / med["step target"], 2), tokens_if_all_accepted=m + 1)
        elif name.startswith("pass sampled"):
            row.update(num_draft=int(name.split("=")[1]), tokens_yielded=sorted(seen[name]))
        elif name.startswith("draft"):
            k = int(name.split("=")[1])
            row.update(num_draft=k, ms_per_drafter_step=round(med[name] / k, 4))
        else:
            row["tokens_per_s"] = round(1e3 / med[name], 1)
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps({"target": "llama3-8b int4 g64 bf16 (synthetic weights)", "drafter": "1B geometry int4 g64 bf16 (synthetic weights): hidden 2048, "
                                              "16 layers, 32 / 8 heads of 64, intermediate 8192, V 128256", "context": o, "reps": args.reps, "window": args.window,
                                              "sampler": list(SAMPLER), "acceptance": "not measured (synthetic weights)", "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
