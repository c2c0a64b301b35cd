"""What a speculative pass under a token automaton costs, with scripts/bench_speculative.py's method on the same 8B int4
g64 geometry with synthetic weights: every figure is the median of --reps windows of --window calls after one warm-up window, with the
spread (max - min) of the windows, all forms alternating in one process.

The automaton is a chain: one branching state that allows the even ids, then --run states that allow one (odd) id each, then a state that
allows one id for ever.  Behind the branch every state is forced, so a draft made of the run is accepted in full with synthetic weights
and under any sampler: nothing is rewound to force acceptance but the state the pass starts from.  Forms:
    (a) step automaton        the replayed step with the automaton set, queued back to back, one synchronise per window:
                              the baseline, measured here
    (b) pass grammar m=M      one Model.spec_step_grammar over the forced run's first M ids, the next draft (n-gram + grammar launch)
                              queued behind it, ONE read-back, from a rewound state
        pass grammar+bias     the same with a one-entry logit bias: the edit launch too
    (c) pass tail+bias m=M    Model.spec_step_tail WITHOUT an automaton under the same bias, at the same rows, on a draft it accepts in
                              full: (b) grammar+bias minus this is what walk + mask + masked partials add
        pass raw m=M          Model.spec_step, the greedy and raw pass
    (d) engine                InferenceEngine.generate end to end under the chain, with and without SpeculativeParams(grammar=True):
                              tokens / s and spec_stats
break_even_tokens = pass_ms / step_ms: the tokens a pass must yield to match the automaton's plain step.

    python scripts/bench_speculative_automaton.py [--drafts 5,7,15] [--reps 5] [--window 20] [--context 512] [--out FILE]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams, _ffi  # noqa: E402
from proxy_inference_engine_amd.cache import ReusableKVCache  # noqa: E402
from proxy_inference_engine_amd.logits_processors import TokenAutomaton  # noqa: E402
from proxy_inference_engine_amd.models.llama import Model, ModelArgs  # noqa: E402
from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint  # noqa: E402

BIAS = ([11], [0.5])


def chain_automaton(V: int, run_len: int, seed: int = 0):
    """(automaton, run): state 0 allows the even ids and leads to state 1; state 1 + i allows run[i] alone; the last state run[-1] for ever."""
    rng = np.random.default_rng(seed)
    run = (2 * rng.choice(V // 2, size=run_len, replace=False) + 1).astype(np.int64)   # distinct odd ids
    cls = np.zeros(V, dtype=np.int32)
    cls[0::2] = 1
    cls[run] = 2 + np.arange(run_len)
    trans = np.full((run_len + 2, run_len + 2), -1, dtype=np.int32)
    trans[0, 1] = 1
    trans[1 + np.arange(run_len), 2 + np.arange(run_len)] = 2 + np.arange(run_len)
    trans[run_len + 1, run_len + 1] = run_len + 1
    return TokenAutomaton(cls, trans, 0), [int(t) for t in run]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drafts", default="5,7,15")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--context", type=int, default=512)
    ap.add_argument("--run", type=int, default=96)
    ap.add_argument("--engine-tokens", type=int, default=88)
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
    A, run = chain_automaton(V, args.run)
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, V, (args.context,), generator=g).to(device="cuda", dtype=torch.int32)
    o = args.context

    cache = [ReusableKVCache() for _ in model.layers]
    model.set_step_tail(token_automaton=A)
    model.step(prompt, cache)
    fed = int(model.history[o].item())                                         # the branch's token: the run follows it
    assert fed % 2 == 0
    tails = {"grammar": dict(token_automaton=A), "grammar+bias": dict(token_automaton=A, logit_bias=BIAS), "tail+bias": dict(logit_bias=BIAS), "raw": {}}

    def rewind(tail):
        """Back to the state behind the prompt: offset o, `fed` about to be fed, the automaton behind the branch."""
        for c in cache:
            c.trim(c.offset - o)
        _ffi.check(lib.pie_decoder_set_state(model._dec, o, fed, _ffi.stream()))
        model._kv.offset = o
        if "token_automaton" in tails[tail]:
            model.reset_step_automaton(1)

    def one_pass(tail, d, then_draft=None):
        if tail.startswith("grammar"):
            return model.spec_step_grammar(d, cache, then_draft=None if then_draft is None else then_draft + (True,))
        return (model.spec_step if tail == "raw" else model.spec_step_tail)(d, cache, then_draft=then_draft)

    accepted_draft: dict = {}

    def full_draft(tail, m):
        """The draft a pass over m + 1 rows under `tail` accepts whole: the forced run under the automaton; without one the pass's own token
        takes the place of the first rejected draft, one position per pass."""
        if tail.startswith("grammar"):
            return torch.tensor(run[:m], dtype=torch.int32, device="cuda")
        if (tail, m) not in accepted_draft:
            model.set_step_tail(**tails[tail])
            d = torch.zeros(m, dtype=torch.int32, device="cuda")
            for _ in range(m + 1):
                rewind(tail)
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
            model.set_step_tail(**tails[tail])

        def run_window():
            for _ in range(args.window):
                rewind(tail)
                seen[name].add(one_pass(tail, d, then_draft=(3, 1, m))[1])
        return prepare, run_window

    def step_window():
        def prepare():                                                         # a changed tail drops the captured step: captured again here, outside the window
            model.set_step_tail(**tails["grammar"])
            rewind("grammar")
            model.step(None, cache)

        def run_window():
            rewind("grammar")
            for _ in range(args.window):
                model.step(None, cache)
        return prepare, run_window

    windows = {"step automaton": step_window()}
    for tail in tails:
        for m in drafts:
            windows[f"pass {tail} m={m}"] = pass_window(tail, m)
    ms = {k: [] for k in windows}
    for rnd in range(args.reps + 1):                                           # round 0 warms every shape; then the forms alternate
        for name, (prepare, run_window) in windows.items():
            prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_window()
            torch.cuda.synchronize()
            if rnd:
                ms[name].append((time.perf_counter() - t0) * 1e3 / args.window)
    model.set_step_tail()
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    step = med["step automaton"]
    results = []
    for name in windows:
        row = {"form": name, "ms_median": round(med[name], 4), "ms_spread": round(spread[name], 4)}
        if name.startswith("pass"):
            tail, m = name.split()[1], int(name.split("=")[1])
            assert seen[name] == {m + 1}, (name, seen[name])                   # every pass was accepted in full
            row.update(tail=tail, num_draft=m, tokens_yielded=m + 1, tokens_per_s=round((m + 1) / med[name] * 1e3, 1),
                       break_even_tokens=round(med[name] / step, 2), vs_step_fully_accepted=round((m + 1) / med[name] * step, 3))
            if tail == "grammar+bias":
                row["added_ms_vs_tail_pass"] = round(med[name] - med[f"pass tail+bias m={m}"], 4)
            if tail == "grammar":
                row["added_ms_vs_raw_pass"] = round(med[name] - med[f"pass raw m={m}"], 4)
        else:
            row["tokens_per_s"] = round(1e3 / med[name], 1)
        results.append(row)
        print(json.dumps(row), flush=True)

    # (d) the engine end to end, plain and speculated alternating; every request is fresh (prompt pass included in neither figure's tokens)
    engine = {"plain": [], "grammar": []}
    stats, outputs = None, {}
    sp = SpeculativeParams(grammar=True, num_draft=7, min_draft=5)
    host_prompt = prompt.cpu()
    for rnd in range(args.reps + 1):
        for form in engine:
            eng = InferenceEngine(model=model)
            eng.prepare_engine(host_prompt, temp=0, token_automaton=A)
            gen = eng.generate(host_prompt, max_completion_tokens=args.engine_tokens, **({"speculative": sp} if form == "grammar" else {}))
            first = next(gen)[0]                                               # the prompt pass and the branch's token: outside the window
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks = [t for t, _ in gen]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            outputs[form] = [first] + toks
            if rnd:
                engine[form].append(len(toks) / dt)
            if form == "grammar":
                stats = dict(eng.spec_stats)
    model.set_step_tail()
    assert outputs["plain"] == outputs["grammar"] and A.walk(outputs["grammar"]) >= 0
    engine_rows = {form: {"tokens_per_s_median": round(statistics.median(v), 1), "tokens_per_s_spread": round(max(v) - min(v), 1)} for form, v in engine.items()}
    engine_rows["speed_up"] = round(statistics.median(engine["grammar"]) / statistics.median(engine["plain"]), 3)
    engine_rows["spec_stats"] = stats
    engine_rows["tokens"] = args.engine_tokens
    print(json.dumps({"engine": engine_rows}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"model": "llama3-8b int4 g64 bf16 (synthetic weights)", "context": o, "reps": args.reps, "window": args.window,
                                              "automaton": {"states": A.n_states, "classes": A.n_classes, "forced_run": args.run},
                                              "acceptance": "by construction: the drafts are the chain's forced run", "results": results, "engine": engine_rows},
                                             indent=1) + "\n")


if __name__ == "__main__":
    main()
