"""ms per token and launches per step of the Llama-3-8B int4 model (synthetic weights, batch 1) through InferenceEngine.generate_step with
the step tail's token mask and logit bias, next to the unconfigured step and to the host-orchestrated branch a
structuring engine takes.

    python scripts/bench_step_mask.py [--steps 64] [--warmup 8] [--reps 3] [--prompt 128] [--out profiles/step_mask_bench.json]

Rows: unconfigured (greedy) | a static mask | a mask re-uploaded every step after reading the token (token_mask=callable: one read-back
of the fed-back token, the callable, a 16 KB upload, a replay) | a 300-entry logit bias | the structuring-engine branch
(structuring_engine=an object whose process_logits leaves an allowed set finite: Model.__call__, the torch processor, logprobs_argmax --
the path every constrained request took before the fused mask, and the one such an object still takes).  The mask allows every other
token id.  The rows alternate, rep by rep, on one model; every rep is a fresh request (prompt pass and graph capture outside the timed
steps).  Prints one JSON line and, with --out, writes it to that file.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


class MaskingEngine:
    """The part of a structuring engine _inference talks to: process_logits leaves only `allowed` finite."""
    has_reached_accept_state = False

    def __init__(self, allowed):
        self.allowed = torch.as_tensor(allowed, dtype=torch.long)

    def get_current_state(self):
        return None

    def process_logits(self, tokens, logits):
        idx = self.allowed.to(logits.device)
        out = torch.full_like(logits, float("-inf"))
        out[..., idx] = logits[..., idx]
        return out

    def sample(self, logprobs, sampler):
        return sampler(logprobs)


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
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    prompt = torch.randint(0, V, (args.prompt,), generator=torch.Generator().manual_seed(0)).tolist()
    allowed = list(range(0, V, 2))
    even, odd = hip_ops.pack_token_mask(allowed, V), hip_ops.pack_token_mask(range(1, V, 2), V)
    gen_bias = torch.Generator().manual_seed(1)
    bias = {int(i): float(b) for i, b in zip(torch.randperm(V, generator=gen_bias)[:300].tolist(), (torch.rand(300, generator=gen_bias) * 4 - 2).tolist())}
    rows = {
        "unconfigured": (dict(temp=0), None),
        "static_mask": (dict(temp=0, token_mask=even), None),
        "mask_per_step": (dict(temp=0, token_mask=lambda tokens: even if tokens[-1] % 2 else odd), None),   # reads the token, then uploads new words
        "bias_300": (dict(temp=0, logit_bias=bias), None),
        "structuring_engine_host": (dict(temp=0), MaskingEngine(allowed)),
    }

    def one_rep(kwargs, engine):
        eng = InferenceEngine(model=model, structuring_engine=engine)
        eng.prepare_engine(prompt, **kwargs)
        gen = eng.generate_step(torch.tensor(prompt))
        for _ in range(1 + args.warmup):
            next(gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            next(gen)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        fused = any(e is not None for e in model.step_tail_edits)
        return ms, model.graph_launches(True), fused

    ms = {name: [] for name in rows}
    launches, fused = {}, {}
    for _ in range(args.reps):
        for name, (kwargs, engine) in rows.items():
            t, n, f = one_rep(kwargs, engine)
            ms[name].append(t)
            launches[name], fused[name] = n, f
    assert fused["static_mask"] and fused["mask_per_step"] and fused["bias_300"] and not fused["structuring_engine_host"]
    base = min(ms["unconfigured"])
    results = [{"row": name, "ms_per_step": round(min(v), 4), "over_unconfigured": round(min(v) / base, 4), "runs_ms": [round(x, 4) for x in v],
                # the host branch replays no graph: Model.__call__'s eager launches, lm_head on every row, the torch processor's kernels, then the tail's two
                "graph_launches_per_step": launches[name] if rows[name][1] is None else None}
               for name, v in ms.items()]
    model.set_step_tail()
    line = json.dumps({"bench": "step_mask", "model": "llama3-8b int4 g64 (synthetic)", "batch": 1, "prompt": args.prompt, "steps": args.steps,
                       "reps": args.reps, "results": results})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
