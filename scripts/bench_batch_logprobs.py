"""What top-n log-probabilities cost inside the passes and what they replace, on the 8B int4 model.

Batched (pie_decoder_step_batch at B sequences), three variants alternating on the one device:
    unarmed   the step as it is without set_batch_top_logprobs
    armed     set_batch_top_logprobs(B, 20) with count = 20 in every row: the records are written inside the replayed graph
    host      what a caller writes today: the unarmed step, then torch.topk(logprobs, 20), a gather of the chosen ids' values, and a
              read-back of the three results
Single sequence: the replayed step under set_step_tail(top_logprobs=20) with one read of the record per token, against the plain step
followed by torch.topk over the [V] row, the chosen id's .item() gather and the read-back (the former InferenceEngine.generate path).
Best of --rounds rounds of --steps steps; launches: the kernel nodes of the captured graph (the host form's library launches are not counted).

    python scripts/bench_batch_logprobs.py [--batches 8,32] [--steps 64] [--rounds 3] [--out profiles/batch_logprobs_bench.json]
    python scripts/bench_batch_logprobs.py --kernels     # only the op, rows = 32, V = 128256, n = 20: for a kernel trace of its own
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from proxy_inference_engine_amd import _ffi, hip_ops  # noqa: E402
from proxy_inference_engine_amd.models.llama import Model, ModelArgs  # noqa: E402
from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint  # noqa: E402

N = 20


def stream_peak_gbps() -> float:
    """bench.py's roofline.stream_peak: a bare streaming read of 1 GiB (pie_stream_read), HIP events, best of 5."""
    buf = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    buf.random_(0, 255)
    lib = _ffi.load()
    _ffi.check(lib.pie_stream_read(buf.data_ptr(), buf.numel(), _ffi.stream()))
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _ffi.check(lib.pie_stream_read(buf.data_ptr(), buf.numel(), _ffi.stream()))
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return buf.numel() / (min(ms) * 1e-3) / 1e9


def kernels_only(rows: int, V: int, reps: int) -> dict:
    """The op alone on log-softmax rows of bf16-rounded logits (ties as a model's rows have them): event-timed, and the shape a kernel
    trace of this process shows."""
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn((rows, V), generator=g) * 2.5).to(torch.bfloat16).float().cuda()
    lp = torch.log_softmax(logits, dim=-1).contiguous()
    tokens = lp.argmax(-1).to(torch.int32)
    ws = hip_ops.top_logprobs_workspace("cuda", rows, V, N)
    out = hip_ops.top_logprobs(lp, N, tokens=tokens, workspace=ws)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip_ops.top_logprobs(lp, N, tokens=tokens, workspace=ws, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    peak = stream_peak_gbps()
    read_us = rows * V * 4 / (peak * 1e9) * 1e6
    return {"mode": "op alone", "rows": rows, "V": V, "n": N, "us_per_call_events_best": round(min(ms) * 1e3, 2), "stream_peak_gbps": round(peak, 1),
            "bytes_read_once": rows * V * 4, "us_to_read_once_at_stream_peak": round(read_us, 2), "ratio": round(min(ms) * 1e3 / read_us, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cfg = dict(LLAMA3_8B)
    V = cfg["vocab_size"]
    if args.kernels:
        print(json.dumps(kernels_only(32, V, 20)), flush=True)
        return
    if args.layers:
        cfg["num_hidden_layers"] = args.layers
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    batches = [int(b) for b in args.batches.split(",")]
    positions = args.prompt + 8 + 3 * (args.rounds * args.steps + 8)
    pages_per_seq = (positions + 63) // 64 + 1
    g = torch.Generator().manual_seed(1)
    results = []

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    # ---- single sequence (contiguous cache): the record inside the replayed step against the step + torch.topk
    cache = model.make_cache()
    model.step(torch.randint(0, V, (args.prompt,), generator=g).cuda(), cache)

    def fused_single():
        model.step(None, cache)
        ids, vals = model.step_top_logprobs
        torch.cat([ids, vals.view(torch.int32)]).cpu()                        # the one read per token

    def host_single():
        tok, lp, _ = model.step(None, cache)
        vals, idx = torch.topk(lp, N)
        t = tok.tolist()[0]
        lp[t].item()
        idx.tolist(), vals.tolist()

    best, launches = {}, {}
    for rnd in range(args.rounds):
        for name, tail, step in (("plain step + torch.topk", {}, host_single), ("top_logprobs=20 in the step", {"top_logprobs": N}, fused_single)):
            model.set_step_tail(**tail)
            for _ in range(4):
                step()
            launches[name] = model.graph_launches()
            best[name] = min(best.get(name, 1e9), timed(step))
    model.set_step_tail()
    for name, t in best.items():
        row = {"mode": "single sequence", "form": name, "ms_per_step": round(t * 1e3, 3), "launches_per_step": launches[name]}
        results.append(row)
        print(json.dumps(row), flush=True)
    del cache

    # ---- batched
    model.enable_paged_kv(num_pages=max(batches) * pages_per_seq + 4, max_blocks=pages_per_seq)
    for B in batches:
        prompts = [torch.randint(0, V, (args.prompt + (i % 7),), generator=g).tolist() for i in range(B)]
        caches = [model.make_cache() for _ in range(B)]
        tokens, _, _ = model.prefill_batch(prompts, caches)
        state = {"tokens": tokens.clone()}

        def plain_step():
            state["tokens"], _, _ = model.step_batch(state["tokens"], caches)
            state["tokens"].tolist()                                          # the per-pass read-back of the tokens every loop has

        def armed_step():
            state["tokens"], _, _ = model.step_batch(state["tokens"], caches)
            torch.cat([state["tokens"][:, None], bufs["ids"][:B], bufs["vals"][:B].view(torch.int32)], dim=1).cpu()   # tokens and records in one read-back

        def host_step():
            nxt, lp, _ = model.step_batch(state["tokens"], caches)
            state["tokens"] = nxt
            vals, idx = torch.topk(lp, N)
            own = lp.gather(1, nxt.long()[:, None])
            nxt.tolist(), idx.tolist(), vals.tolist(), own.tolist()

        best, launches = {}, {}
        for rnd in range(args.rounds):
            for name in ("unarmed", "armed", "host"):                         # the variants alternate inside every round
                if name == "armed":
                    bufs = model.set_batch_top_logprobs(B, N)
                    bufs["count"].fill_(N)
                else:
                    model.clear_batch_top_logprobs()
                step = {"unarmed": plain_step, "armed": armed_step, "host": host_step}[name]
                for _ in range(4):
                    step()
                launches[name] = model.batch_graph_launches()
                best[name] = min(best.get(name, 1e9), timed(step))
        model.clear_batch_top_logprobs()
        for name, t in best.items():
            row = {"mode": "step_batch", "sequences": B, "form": name, "ms_per_step": round(t * 1e3, 3), "tokens_per_s": round(B / t, 1),
                   "launches_per_step": launches[name], "vs_unarmed": round(t / best["unarmed"], 3)}
            results.append(row)
            print(json.dumps(row), flush=True)
        for c in caches:
            c[0].page_manager.release()
    if args.out:
        Path(args.out).write_text(json.dumps({"model": "llama3-8b int4 g64 bf16 (synthetic weights)", "prompt": args.prompt, "steps": args.steps,
                                              "rounds": args.rounds, "n": N, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
