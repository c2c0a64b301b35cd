"""What the one-launch chunk attention on 16-bit pages costs, on the 8B geometry (32 / 8 heads, head_dim 128, bf16), synthetic
cache.  Op-level cells, ONE layer's attention, the forms alternating in one process (DESIGN.md 26's protocol):
    loop      the parent's path: k_prefill_attn through pie_sdpa_prefill, one launch per chunk, on contiguous K / V of the same values (the op
              level has no paged entry for it: the same kernel less one scalar table lookup per 32-key block)
    paged     pie_prefill_attn_paged with splits = 0: one launch for all chunks of the cell, split by its rule, and the merge where it splits
    paged@1split  the same kernel with one split (no partials, no merge)
    paged@T   the same with the split count a target of T workgroups would give (--targets; single-chunk cells), at most 32 and the chunk's pages
  cells: a 256-row chunk behind 512, 8192 and 32768 cached positions; 32 suffixes of 32 rows behind 1024 shared positions.
Before a cell is timed its paged outputs are compared with the loop's on the same values (max |difference|, differing share).
Every figure: the median of --reps windows of --window calls after one warm-up window, with the spread (max - min) of the windows.

    python scripts/bench_prefill_chunk_paged.py [--reps 5] [--window 16] [--targets 256,512,1024] --out profiles/prefill_chunk_paged_bench.json
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
from bench_prefill_chunk_i8 import D, HBM_GB_PER_S, HKV, HQ, windows  # noqa: E402


def op_cell(label, pairs, shared, targets, reps, window):
    """pairs = [(rows, cached)]; shared: every chunk reads the same cached positions (one block-table row's pages in front)."""
    from proxy_inference_engine_amd import _ffi
    lib = _ffi.load()
    blocks = [(m + p + 63) // 64 for m, p in pairs]
    n_pages, N = sum(blocks), sum(m for m, _ in pairs)
    tables, chunks, at, first = np.zeros((len(pairs), max(blocks)), np.int32), [], 0, 0
    for s, ((m, p), nb) in enumerate(zip(pairs, blocks)):
        tables[s, :nb] = np.arange(at, at + nb)
        if shared and s:
            tables[s, :p // 64] = tables[0, :p // 64]
        at += nb
        chunks.append([first, m, p, s])
        first += m
    q = torch.randn((N, HQ, D), device="cuda").to(torch.bfloat16)
    kv = [torch.empty((2, HKV, p + m, D), dtype=torch.bfloat16, device="cuda").normal_(0.0, 0.5) for m, p in (pairs[:1] if shared else pairs)]
    slab = torch.zeros((n_pages, 2, HKV, 64, D), dtype=torch.bfloat16, device="cuda")
    for s, nb in enumerate(blocks):                                    # the same values, page by page
        x = kv[0 if shared else s]
        pad = torch.zeros((2, HKV, nb * 64, D), dtype=x.dtype, device="cuda")
        pad[:, :, :x.shape[2]] = x
        slab[torch.from_numpy(tables[s, :nb]).long().cuda()] = pad.view(2, HKV, nb, 64, D).permute(2, 0, 1, 3, 4)
    tables_d, scale = torch.from_numpy(tables).cuda(), D ** -0.5
    ch = np.ascontiguousarray(np.asarray(chunks, np.int32))
    outs = {"loop": torch.zeros_like(q)}

    def loop_form():
        for (first, m, p, s) in chunks:
            k, v = kv[0 if shared else s]
            _ffi.check(lib.pie_sdpa_prefill(q[first:].data_ptr(), _ffi.p(k), _ffi.p(v), HQ, HKV, m, p, k.shape[1], D, scale, _ffi.PIE_BF16, outs["loop"][first:].data_ptr(),
                                            _ffi.stream()))

    rule = int(lib.pie_prefill_attn_paged_splits(ch.ctypes.data, len(ch), HQ, HKV))
    wgs = sum((m + 31) // 32 for m, _ in pairs) * HKV                 # (one 32-row tile per workgroup: the form these cells take)
    forms = {"paged": rule, "paged@1split": 1}
    for t in (targets if len(pairs) == 1 else ()):
        forms[f"paged@{t}"] = max(1, min(32, max(blocks), -(-t // wgs)))
    ws = torch.empty(max(int(lib.pie_prefill_attn_paged_workspace_bytes(ch.ctypes.data, len(ch), HQ, D, max(forms.values()))), 16), dtype=torch.uint8, device="cuda")

    def paged_form(name):
        def run():
            _ffi.check(lib.pie_prefill_attn_paged(_ffi.p(q), _ffi.p(slab), n_pages, slab.numel() * 2, _ffi.p(tables_d), len(pairs), tables.shape[1], ch.ctypes.data, len(ch), N,
                                                  HQ, HKV, D, _ffi.PIE_BF16, scale, forms[name], _ffi.p(outs[name]), _ffi.p(ws), _ffi.stream()))
        return run

    fns = {"loop": loop_form}
    loop_form()
    for name in forms:
        outs[name] = torch.zeros_like(q)
        fns[name] = paged_form(name)
        fns[name]()
    torch.cuda.synchronize()
    res, rows = windows(fns, reps, window), []
    kv_bytes = sum(HKV * (p + m) * D * 2 * 2 for m, p in pairs)
    for form, (ms, spread) in res.items():
        diff = (outs[form].float() - outs["loop"].float()).abs()
        rows.append({"cell": label, "form": form, "splits": forms.get(form, 1), "workgroups": wgs * forms.get(form, 1) if form != "loop" else wgs, "us": round(ms * 1e3, 2),
                     "spread_us": round(spread * 1e3, 2), "kv_bytes": kv_bytes, "kv_gb_per_s": round(kv_bytes / (ms * 1e-3) / 1e9, 1),
                     "hbm_share": round(kv_bytes / (ms * 1e-3) / 1e9 / HBM_GB_PER_S, 4), "max_abs_diff_to_loop": float(diff.max()),
                     "differing_share_to_loop": round(float((diff > 0).float().mean()), 5)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--targets", default="256,512,1024")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    targets, results = [int(t) for t in args.targets.split(",") if t], []
    for label, pairs, shared in (("256 rows behind 512", [(256, 512)], False), ("256 rows behind 8192", [(256, 8192)], False),
                                 ("256 rows behind 32768", [(256, 32768)], False), ("32 suffixes of 32 rows behind 1024 shared", [(32, 1024)] * 32, True)):
        results += op_cell(label, pairs, shared, targets, args.reps, args.window)
    if args.out:
        Path(args.out).write_text(json.dumps({"geometry": "32 / 8 heads, head_dim 128, bf16", "reps": args.reps, "window": args.window, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
