"""Decode tok/s of the Llama-3-8B int4 model (synthetic weights, batch 1) at several cache lengths for 16-bit, 8-bit and 4-bit KV (g = 64).

    python scripts/bench_kv_quant.py [--ctx 1024 8192 32768] [--steps 64] [--warmup 8]

Each configuration starts from a cache that already holds `ctx` positions (the decode step's time does not depend on their values),
then times `steps` replayed step graphs.  Prints one JSON line.
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
    ap.add_argument("--ctx", type=int, nargs="+", default=[1024, 8192, 32768])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from proxy_inference_engine_amd.cache import QuantizedKVCache
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint

    cfg = dict(LLAMA3_8B)
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    results = []
    for ctx in args.ctx:
        for bits in (16, 8, 4):
            cache = model.make_cache() if bits == 16 else [QuantizedKVCache(group_size=64, bits=bits) for _ in model.layers]
            need = 1 + args.warmup + args.reps * args.steps
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
            kv_bytes = sum(t.numel() * t.element_size() for c in cache for t in ((c.keys, c.values) if bits == 16 else (*c.keys, *c.values)))
            results.append({"ctx": ctx, "kv_bits": bits, "ms_per_step": round(min(ms), 4), "ms_median": round(sorted(ms)[len(ms) // 2], 4),
                            "tok_s": round(1e3 / min(ms), 1), "kv_gb": round(kv_bytes / 1e9, 3)})
            del cache
            torch.cuda.empty_cache()
            print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"bench": "kv_quant", "model": "llama3-8b int4 g64 (synthetic)", "batch": 1, "group_size": 64, "results": results}))


if __name__ == "__main__":
    main()
