"""ms per token and launches per step of the Llama-3-8B int4 model (synthetic weights, batch 1) through InferenceEngine.generate_step
with a grammar as a device-side token automaton, next to the forms it replaces.

    python scripts/bench_step_automaton.py [--steps 64] [--warmup 8] [--reps 3] [--prompt 128] [--out profiles/step_automaton_bench.json]

Rows: unconfigured (greedy) | a static mask | the same grammar as token_mask=callable -- one read-back of the fed-back token, the host's
walk (a table lookup into per-state masks packed ahead of time: the cheapest callable a grammar engine could bind), a 16 KB upload, a
replay | the grammar as token_automaton=: the state, the table and the walk on the device, nothing read back and nothing uploaded.  The
grammar is a synthetic automaton of 200 states and 32 token classes over V = 128256, about half of the ids allowed in every state; the
last two rows generate the same tokens.  The rows alternate, rep by rep, on one model; every rep is a fresh request (prompt pass and graph
capture outside the timed steps).  Also timed, once and on the CPU: TokenAutomaton.from_byte_dfa over a synthetic vocabulary of V byte
strings (a 40-state byte DFA).  Prints one JSON line and, with --out, writes it to that file.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def synthetic_automaton(V: int, S: int = 200, n_cols: int = 32, seed: int = 0):
    from proxy_inference_engine_amd.logits_processors import TokenAutomaton
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, S, size=(S, n_cols)).astype(np.int32)
    cols[rng.random((S, n_cols)) < 0.5] = -1
    cols[:, 0] = (np.arange(S) + 1) % S   # every state is reachable and allows a token
    return TokenAutomaton.from_token_table(cols[:, rng.integers(0, n_cols, size=V)])


def host_compile_seconds(V: int, seed: int = 0) -> float:
    """from_byte_dfa at the model's vocabulary size: V - 256 random strings of 1..8 bytes over a small alphabet, 256 special tokens, a
    random 40-state byte DFA over that alphabet whose states are all accepting."""
    from proxy_inference_engine_amd.logits_processors import TokenAutomaton
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b'{}[]":,0123456789 abcdefghijklmnopqrstuvwxyz', dtype=np.uint8)
    lens = rng.integers(1, 9, size=V - 256)
    flat = rng.choice(alphabet, size=int(lens.sum())).tobytes()
    ends = np.cumsum(lens)
    toks = [flat[e - n:e] for e, n in zip(ends.tolist(), lens.tolist())] + [None] * 256
    bt = np.full((40, 256), -1, dtype=np.int32)
    bt[:, alphabet] = rng.integers(0, 40, size=(40, alphabet.size))
    t0 = time.perf_counter()
    TokenAutomaton.from_byte_dfa(bt, range(40), toks, [V - 1])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from proxy_inference_engine_amd import InferenceEngine, hip_ops
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint

    cfg = dict(LLAMA3_8B)
    V = cfg["vocab_size"]
    compile_s = host_compile_seconds(V)
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    prompt = torch.randint(0, V, (args.prompt,), generator=torch.Generator().manual_seed(0)).tolist()
    A = synthetic_automaton(V)
    packed = [hip_ops.pack_token_mask(torch.from_numpy(A.allowed(s)), V) for s in range(A.n_states)]   # ahead of time, outside every timed step
    walk = {"state": A.start, "seen": 0}

    def host_grammar(tokens):
        """The host's walk, one table lookup per token: the first call sees the prompt, every later one the token fed back."""
        if walk["seen"]:
            walk["state"] = A.step(walk["state"], tokens[-1])
        walk["seen"] += 1
        return packed[walk["state"]]

    rows = {
        "unconfigured": dict(temp=0),
        "static_mask": dict(temp=0, token_mask=packed[A.start]),
        "mask_per_step": dict(temp=0, token_mask=host_grammar),
        "device_automaton": dict(temp=0, token_automaton=A),
    }

    def one_rep(kwargs):
        walk.update(state=A.start, seen=0)
        eng = InferenceEngine(model=model)
        eng.prepare_engine(prompt, **kwargs)
        gen = eng.generate_step(torch.tensor(prompt))
        toks = [next(gen)[0] for _ in range(1 + args.warmup)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks += [next(gen)[0] for _ in range(args.steps)]
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        return ms, model.graph_launches(True), [int(t) for t in torch.cat([t.reshape(1) for t in toks]).tolist()]

    ms = {name: [] for name in rows}
    launches, tokens = {}, {}
    for _ in range(args.reps):
        for name, kwargs in rows.items():
            t, n, toks = one_rep(kwargs)
            ms[name].append(t)
            launches[name], tokens[name] = n, toks
    assert tokens["device_automaton"] == tokens["mask_per_step"] and A.walk(tokens["device_automaton"]) >= 0   # the same grammar, the same tokens
    base = min(ms["unconfigured"])
    results = [{"row": name, "ms_per_step": round(min(v), 4), "over_unconfigured": round(min(v) / base, 4), "runs_ms": [round(x, 4) for x in v],
                "graph_launches_per_step": launches[name]} for name, v in ms.items()]
    model.set_step_tail()
    line = json.dumps({"bench": "step_automaton", "model": "llama3-8b int4 g64 (synthetic)", "batch": 1, "prompt": args.prompt, "steps": args.steps,
                       "reps": args.reps, "automaton": {"states": A.n_states, "classes": A.n_classes, "words": int(A.words().size)},
                       "from_byte_dfa_host_seconds": round(compile_s, 3), "results": results})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
