"""What the log-probabilities of prompt tokens cost inside the prompt pass and what they replace, on the 8B int4 model.

One prompt of L tokens on a fresh contiguous cache, three forms alternating on the one device:
    plain        model.step(ids): the prompt pass as it is without set_prompt_logprobs
    scored       set_prompt_logprobs(L, n, block_rows), targets and counts written, then the same model.step(ids) and one read-back of the records
    composition  what a caller writes without it: model(ids) -> T [L, V] logits, torch.log_softmax(.float(), -1), hip_ops.top_logprobs over
                 all rows, and the same read-back
n = 0 asks for the tokens' own log-probabilities only (count 0 in every row).  Median of --reps repetitions after one warm-up each, host
clock around work that ends in a device synchronise.  peak_mb: torch's allocator peak above what was allocated before the call -- the
logits, log-probabilities and records a form needs, and the fresh KV cache of the call; the library's own prompt scratch is common to the
three and not in it, and neither is the scored form's workspace, which the model allocates once and keeps (workspace_mb, from its size).

    python scripts/bench_prompt_logprobs.py [--lengths 128,1024,4096] [--ns 0,5,20] [--blocks 128,256,512,1024] [--reps 5] [--out FILE]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from proxy_inference_engine_amd import _ffi, hip_ops  # noqa: E402
from proxy_inference_engine_amd.cache import ReusableKVCache  # noqa: E402
from proxy_inference_engine_amd.models.llama import Model, ModelArgs  # noqa: E402
from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="128,1024,4096")
    ap.add_argument("--ns", default="0,5,20")
    ap.add_argument("--blocks", default="128,256,512,1024")
    ap.add_argument("--block-rows", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cfg = dict(LLAMA3_8B)
    if args.layers:
        cfg["num_hidden_layers"] = args.layers
    V = cfg["vocab_size"]
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    g = torch.Generator().manual_seed(1)
    results = []
    lib = _ffi.load()

    def fresh():
        return [ReusableKVCache() for _ in model.layers]

    def forms(ids, n, block_rows):
        L = ids.numel()
        targets = torch.cat([ids[1:], ids[:1]]).contiguous()
        count = torch.full((L,), n, dtype=torch.int32, device="cuda")
        count[-1] = -1

        def plain():
            model.step(ids, fresh())[0].tolist()

        def scored():
            bufs = model.set_prompt_logprobs(L, max(n, 1), block_rows)
            bufs["targets"].copy_(targets), bufs["count"].copy_(count)
            tok = model.step(ids, fresh())[0]
            model.clear_prompt_logprobs()
            torch.cat([tok, bufs["ids"].reshape(-1), bufs["vals"].reshape(-1).view(torch.int32)]).cpu()

        def composition():
            logits = model(ids[None], cache=fresh())[0]
            lp = torch.log_softmax(logits.float(), -1)
            rec_ids, rec_vals = hip_ops.top_logprobs(lp, max(n, 1), tokens=targets, count=count)
            torch.cat([lp[-1].argmax().reshape(1).to(torch.int32), rec_ids.reshape(-1), rec_vals.reshape(-1).view(torch.int32)]).cpu()

        return {"plain": plain, "scored": scored, "composition": composition}

    def measure(fns: dict) -> dict:
        """Every form warmed once, then --reps rounds in which the forms alternate -> {name: (median ms, spread ms, peak MB)}."""
        ms, peak = {k: [] for k in fns}, {}
        for rnd in range(args.reps + 1):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if rnd:
                    ms[name].append(dt)
                    peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
        return {k: (statistics.median(v), max(v) - min(v), peak[k] / 2 ** 20) for k, v in ms.items()}

    def report(mode, L, n, block_rows, got):
        for name, (med, spread, mb) in got.items():
            row = {"mode": mode, "L": L, "n": n, "block_rows": block_rows, "form": name, "ms_median": round(med, 2), "ms_spread": round(spread, 2),
                   "peak_mb": round(mb, 1), "vs_plain": round(med / got["plain"][0], 3) if "plain" in got else None}
            if name.startswith("scored"):
                rows = int(name.split("=")[1]) if "=" in name else block_rows
                row["workspace_mb"] = round(int(lib.pie_decoder_prompt_logprobs_workspace_bytes(model._dec, hip_ops.TOP_LOGPROBS_MAX, rows)) / 2 ** 20, 1)
            results.append(row)
            print(json.dumps(row), flush=True)

    lengths = [int(x) for x in args.lengths.split(",") if x]
    for L in lengths:
        ids = torch.randint(0, V, (L,), generator=g).to(device="cuda", dtype=torch.int32)
        for n in [int(x) for x in args.ns.split(",") if x]:
            report("forms", L, n, args.block_rows, measure(forms(ids, n, args.block_rows)))
    if args.blocks and lengths:
        L = max(lengths)
        ids = torch.randint(0, V, (L,), generator=g).to(device="cuda", dtype=torch.int32)
        sweep = {}
        for b in [int(x) for x in args.blocks.split(",")]:
            sweep[f"scored block_rows={b}"] = forms(ids, 5, b)["scored"]
        sweep = {"plain": forms(ids, 5, args.block_rows)["plain"], **sweep}
        report("block_rows sweep", L, 5, None, measure(sweep))
    if args.out:
        Path(args.out).write_text(json.dumps({"model": "llama3-8b int4 g64 bf16 (synthetic weights)", "reps": args.reps, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
