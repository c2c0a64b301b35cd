"""What the chunk attention on int8 pages costs, on the 8B geometry (32 / 8 heads, head_dim 128, bf16), synthetic cache.

Op-level cells, ONE layer's attention, the two forms alternating in one process:
    i8      hip_ops' pie_prefill_attn_i8: one launch for all chunks of the cell, over int8 pages (random codes, every scale 1/32)
    T       k_prefill_attn through pie_sdpa_prefill: one launch per chunk on 16-bit K / V of the same shapes.  The op level has no paged
            entry for it, so K / V are contiguous: the same kernel less one scalar table lookup per 32-key block
  cells: a 256-row chunk behind 512 and 8192 cached positions; 32 suffixes of 32 rows behind 1024 shared positions.
  kv_bytes = the K / V bytes one pass over the shapes needs (kv-heads x positions x head_dim x 2 x element size, once per chunk), over the
  measured time as kv_gb_per_s and its share of HBM_GB_PER_S.
Pass cell (--layers L of the 8B model, synthetic weights): Model.step_mixed of 8 decode rows at 512 positions + a 256-row chunk behind 512,
on a T pool and on an int8 pool (int8_pages=True).  The model holds one pool at a time, so the two forms run in turns of whole windows
(T, int8, T, int8), not call by call.
Every figure: the median of --reps windows of --window calls after one warm-up window, with the spread (max - min) of the windows.

    python scripts/bench_prefill_chunk_i8.py [--reps 5] [--window 16] [--layers 4] [--no-pass] --out profiles/prefill_chunk_i8_bench.json
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
HBM_GB_PER_S = 8000.0   # the MI355X data sheet's peak HBM3E bandwidth, the denominator of hbm_share
sys.path.insert(0, str(ROOT))
HQ, HKV, D = 32, 8, 128


def windows(fns, reps, window):
    """{name: (median ms per call, spread ms)}: the forms alternate window by window; one warm-up window each."""
    times = {k: [] for k in fns}
    for rep in range(reps + 1):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(window):
                fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e3 / window)
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in times.items()}


def op_cell(label, pairs, shared, reps, window):
    """pairs = [(rows, cached)]; shared: every chunk reads the same cached positions (one block-table row's pages in front)."""
    from proxy_inference_engine_amd import _ffi, hip_ops
    lib = _ffi.load()
    pb = int(lib.pie_page_i8_bytes(HKV, D))
    blocks = [(m + p + 63) // 64 for m, p in pairs]
    n_pages, N = sum(blocks) + 1, sum(m for m, _ in pairs)
    slab = torch.randint(-48, 49, (n_pages, pb), dtype=torch.int8, device="cuda")
    slab.view(torch.float16)[:, HKV * 64 * D:HKV * 64 * D + 2 * HKV] = 1 / 32
    tables, chunks, at, first = np.zeros((len(pairs), max(blocks)), np.int32), [], 0, 0
    for s, ((m, p), nb) in enumerate(zip(pairs, blocks)):
        tables[s, :nb] = np.arange(at, at + nb)
        if shared and s:
            tables[s, :p // 64] = tables[0, :p // 64]
        at += nb
        chunks.append([first, m, p, s])
        first += m
    tables_d = torch.from_numpy(tables).cuda()
    q = torch.randn((N, HQ, D), device="cuda").to(torch.bfloat16)
    out = torch.empty_like(q)
    kv = [torch.empty((2, HKV, p + m, D), dtype=torch.bfloat16, device="cuda").normal_(0.0, 0.5) for m, p in (pairs[:1] if shared else pairs)]
    scale = D ** -0.5

    def t_form():
        for (first, m, p, s) in chunks:
            k, v = kv[0 if shared else s]
            _ffi.check(lib.pie_sdpa_prefill(q[first:].data_ptr(), _ffi.p(k), _ffi.p(v), HQ, HKV, m, p, k.shape[1], D, scale, _ffi.PIE_BF16, out[first:].data_ptr(), _ffi.stream()))

    ch = np.ascontiguousarray(np.asarray(chunks, np.int32))

    def i8_form():   # (the entry hip_ops.prefill_attn_i8 calls, into the same preallocated output as the T form)
        _ffi.check(lib.pie_prefill_attn_i8(_ffi.p(q), _ffi.p(slab), n_pages, slab.numel(), _ffi.p(tables_d), len(pairs), tables.shape[1], ch.ctypes.data, len(ch), N, HQ,
                                           HKV, D, _ffi.PIE_BF16, scale, _ffi.p(out), _ffi.stream()))

    assert hip_ops.prefill_attn_i8(q, slab, n_pages, tables_d, chunks, HKV, scale).isfinite().all()
    res = windows({"i8": i8_form, "T": t_form}, reps, window)
    rows = []
    for form, (ms, spread) in res.items():
        kv_bytes = sum(HKV * (p + m) * D * 2 * (1 if form == "i8" else 2) for m, p in pairs)
        rows.append({"cell": label, "form": form, "us": round(ms * 1e3, 2), "spread_us": round(spread * 1e3, 2), "kv_bytes": kv_bytes,
                     "kv_gb_per_s": round(kv_bytes / (ms * 1e-3) / 1e9, 1), "hbm_share": round(kv_bytes / (ms * 1e-3) / 1e9 / HBM_GB_PER_S, 4)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def pass_cells(layers, reps, window):
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint
    cfg = dict(LLAMA3_8B, num_hidden_layers=layers)
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    V, rows = cfg["vocab_size"], []
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, V, (8,), generator=g).to(device="cuda", dtype=torch.int32)
    chunk = torch.randint(0, V, (256,), generator=g).tolist()
    for turn in range(2):
        for form in ("T", "i8"):
            ones = torch.full((layers, HKV), 1 / 32, dtype=torch.float16)
            pool = model.enable_paged_kv(num_pages=9 * 14 + 8, **(dict(kv_dtype=torch.int8, kv_scales=(ones, ones)) if form == "i8" else {}))
            caches = [model.make_cache() for _ in range(9)]
            seqs = [c[0].page_manager for c in caches]
            for s in seqs:                                             # 512 cached positions each; what they hold does not matter here
                s.reserve(512)
                s.advance(512)

            def one():
                model.step_mixed(tok, caches[:8], [chunk], caches[8:], **({"int8_pages": True} if form == "i8" else {}))
                for s in seqs:
                    s.truncate(512)

            ms, spread = windows({form: one}, reps, window)[form]
            rows.append({"cell": f"step_mixed 8 decode rows + 256-row chunk behind 512, {layers} layers", "form": form, "turn": turn, "ms": round(ms, 4), "spread_ms": round(spread, 4)})
            print(json.dumps(rows[-1]), flush=True)
            for s in seqs:
                s.release()
            del pool
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--no-pass", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    results = []
    for label, pairs, shared in (("256 rows behind 512", [(256, 512)], False), ("256 rows behind 8192", [(256, 8192)], False),
                                 ("32 suffixes of 32 rows behind 1024 shared", [(32, 1024)] * 32, True)):
        results += op_cell(label, pairs, shared, args.reps, args.window)
    if not args.no_pass:
        results += pass_cells(args.layers, args.reps, args.window)
    if args.out:
        Path(args.out).write_text(json.dumps({"geometry": "32 / 8 heads, head_dim 128, bf16", "reps": args.reps, "window": args.window, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
