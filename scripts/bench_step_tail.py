"""ms per token of the Llama-3-8B int4 model (synthetic weights, batch 1) through InferenceEngine.generate_step for the engine's two
generation knobs, each through the fused step tail and through the host-orchestrated branch it replaces.

    python scripts/bench_step_tail.py [--steps 64] [--warmup 8] [--reps 3] [--prompt 128]

Configurations: greedy | temp=1, top_k=40 | repetition_penalty=1.1 | both | both and a three-entry logit_bias.  "host" runs the same request with the sampler closure and
the processor wrapped in plain callables (no `hip_spec`, no `.penalty`), which is exactly what an engine without the fused tail runs:
model.step + the sampler closure for a sampler alone, Model.__call__ + the torch processor + logprobs_argmax with a penalty.  (Greedy has
no other branch: its "host" column is the same path, the run-to-run spread.)  The two paths alternate, rep by rep, on one model; every rep
is a fresh request (prompt pass and graph capture outside the timed steps).  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

CONFIGS = {"greedy": dict(temp=0), "top_k": dict(temp=1.0, top_k=40), "penalty": dict(temp=0, repetition_penalty=1.1),
           "top_k+penalty": dict(temp=1.0, top_k=40, repetition_penalty=1.1),
           "top_k+penalty+bias": dict(temp=1.0, top_k=40, repetition_penalty=1.1, logit_bias={11: -2.0, 257: 1.5, 4000: 0.75})}


def plain(fn):
    return lambda *a: fn(*a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=128)
    args = ap.parse_args()
    from proxy_inference_engine_amd import InferenceEngine, samplers
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint

    cfg = dict(LLAMA3_8B)
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    prompt = torch.randint(0, cfg["vocab_size"], (args.prompt,), generator=torch.Generator().manual_seed(0)).tolist()

    def one_rep(kwargs, fused: bool):
        samplers.seed(1)
        eng = InferenceEngine(model=model)
        eng.prepare_engine(prompt, **kwargs)
        if not fused:
            if not getattr(eng.samplers["root"], "is_greedy", False):
                eng.samplers["root"] = plain(eng.samplers["root"])
            eng.logits_processors["root"] = [plain(p) for p in eng.logits_processors["root"]]
        gen = eng.generate_step(torch.tensor(prompt))
        for _ in range(1 + args.warmup):
            next(gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            next(gen)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        return ms, model.graph_launches(True), model.step_tail != (None, None)

    results = []
    for name, kwargs in CONFIGS.items():
        ms = {"fused": [], "host": []}
        launches = {}
        for _ in range(args.reps):
            for path in ("fused", "host"):
                t, n, configured = one_rep(kwargs, path == "fused")
                assert name == "greedy" or configured == (path == "fused"), (name, path)   # the request took the path it is timed as
                ms[path].append(t)
                launches[path] = n
        row = {"config": name, "kwargs": kwargs, "fused_ms_per_token": round(min(ms["fused"]), 4), "host_ms_per_token": round(min(ms["host"]), 4),
               "fused_over_host": round(min(ms["fused"]) / min(ms["host"]), 4), "fused_runs_ms": [round(v, 4) for v in ms["fused"]],
               "host_runs_ms": [round(v, 4) for v in ms["host"]], "fused_launches_per_step": launches["fused"], "host_launches_per_step": launches["host"]}
        results.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    model.set_step_tail()
    print(json.dumps({"bench": "step_tail", "model": "llama3-8b int4 g64 (synthetic)", "batch": 1, "prompt": args.prompt, "steps": args.steps,
                      "reps": args.reps, "results": results}))


if __name__ == "__main__":
    main()
