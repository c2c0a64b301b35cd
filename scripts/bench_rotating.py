"""Decode step of the Llama-3-8B int4 model (synthetic weights, batch 1) on a rotating KV cache (max_kv_size = W, keep = 4) against the
contiguous cache, at several offsets.

    python scripts/bench_rotating.py [--window 4096] [--ctx 4096 32768 131072] [--steps 64] [--warmup 8]

Each configuration starts from a cache that already holds `ctx` positions (a full, rotating ring for the rotating cache; the decode
step's time does not depend on the rows' values), then times `steps` replayed step graphs.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--ctx", type=int, nargs="+", default=[4096, 32768, 131072])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from proxy_inference_engine_amd.cache import RotatingKVCache
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint

    cfg = dict(LLAMA3_8B)
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    W = args.window
    results = []
    for ctx in args.ctx:
        for kind in ("rotating", "contiguous"):
            need = 1 + args.warmup + args.reps * args.steps
            if kind == "rotating":
                cache = [RotatingKVCache(W, keep=4) for _ in model.layers]
                for c in cache:  # a full ring whose next write index wraps to the first ring row
                    c.prepare(W, model.n_kv_heads, model.head_dim, model.dtype, model.device)
                    c._len, c.offset, c._idx = W, ctx, W
            else:
                cache = model.make_cache()
                for c in cache:
                    c.reserve(ctx + need, model.n_kv_heads, model.head_dim, model.dtype, model.device)
                    c.advance(ctx)
            model.step(torch.tensor([1], dtype=torch.int32, device="cuda"), cache)
            for _ in range(args.warmup):
                model.step(None, cache)
            ms = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    model.step(None, cache)
                torch.cuda.synchronize()
                ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
            kv_bytes = sum(t.numel() * t.element_size() for c in cache for t in (c.keys, c.values))
            results.append({"ctx": ctx, "cache": kind, "window": W if kind == "rotating" else None, "ms_per_step": round(min(ms), 4),
                            "ms_median": round(sorted(ms)[len(ms) // 2], 4), "tok_s": round(1e3 / min(ms), 1), "kv_gb": round(kv_bytes / 1e9, 3)})
            del cache
            torch.cuda.empty_cache()
            print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"bench": "rotating", "model": "llama3-8b int4 g64 (synthetic)", "batch": 1, "window": W, "keep": 4, "results": results}))


if __name__ == "__main__":
    main()
