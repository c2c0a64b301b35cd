"""What the per-row tail of the multi-sequence step costs and what it replaces, on the 8B int4 model: ms per step and kernel
launches per step of pie_decoder_step_batch at B sequences with
    none      no tail set (the greedy tail)
    top_k     every row top-k 40 at temperature 0.8
    penalty   every row greedy with a repetition penalty of 1.3 over 60 ids
    mix       a quarter each of greedy, top-k, top-p 0.9 and the penalty
each of the last three in two forms, alternating on the one device: `fused` -- the records of a batch tail, one graph replay per step -- and
`host` -- today's alternative for the same requests: the untailed step, then per row hip_ops.logits_penalty over the host's window and
hip_ops.logprobs_argmax where the row has a penalty, and make_sampler's closure over the row's log-probabilities where it samples.  Best of
--rounds rounds of --steps steps.  Launches: the kernel nodes of the captured graph, plus for `host` the launches of the ops it calls per
step (pie_logits_penalty 1, pie_logprobs_argmax 2, pie_sample 2 or 5).

    python scripts/bench_batch_tail.py [--batches 8,32] [--steps 64] [--rounds 3] [--out profiles/batch_tail_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from proxy_inference_engine_amd import hip_ops, samplers  # noqa: E402
from proxy_inference_engine_amd.engine import SamplingParams  # noqa: E402
from proxy_inference_engine_amd.models.llama import Model, ModelArgs  # noqa: E402
from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint  # noqa: E402

KINDS = {"greedy": SamplingParams(), "top_k": SamplingParams(temp=0.8, top_k=40), "top_p": SamplingParams(temp=0.8, top_p=0.9),
         "penalty": SamplingParams(repetition_penalty=1.3, repetition_context_size=60)}
SAMPLE_LAUNCHES = {"categorical": 2, "top_k": 5, "top_p": 5, "min_p": 2}


def requests(variant: str, B: int) -> list:
    if variant == "mix":
        order = ["greedy", "top_k", "top_p", "penalty"]
        return [KINDS[order[i * 4 // B]] for i in range(B)]
    return [KINDS[variant]] * B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cfg = dict(LLAMA3_8B)
    if args.layers:
        cfg["num_hidden_layers"] = args.layers
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    batches = [int(b) for b in args.batches.split(",")]
    V = cfg["vocab_size"]
    # every timed loop advances the sequences: 7 forms x rounds x steps positions, plus the warm-ups
    positions = args.prompt + 8 + 7 * (args.rounds * args.steps + 8)
    pages_per_seq = (positions + 63) // 64 + 1
    model.enable_paged_kv(num_pages=max(batches) * pages_per_seq + 4, max_blocks=pages_per_seq)
    g = torch.Generator().manual_seed(1)
    results = []
    for B in batches:
        prompts = [torch.randint(0, V, (args.prompt + (i % 7),), generator=g).tolist() for i in range(B)]
        caches = [model.make_cache() for _ in range(B)]
        tokens, _, _ = model.prefill_batch(prompts, caches)
        state = {"tokens": tokens.clone(), "fed": [list(p) for p in prompts]}

        def fused_step():
            state["tokens"], _, _ = model.step_batch(state["tokens"], caches)

        def make_host_step(params):
            closures = [None if sp.temp == 0 else samplers.make_sampler(temp=sp.temp, top_p=sp.top_p, min_p=sp.min_p, top_k=sp.top_k) for sp in params]

            def host_step():
                fed_now = state["tokens"]
                nxt, logprobs, logits = model.step_batch(fed_now, caches)
                if any(sp.repetition_penalty != 1.0 for sp in params):
                    for f, t in zip(state["fed"], fed_now.tolist()):             # (the window lives on the host: one read-back per step)
                        f.append(t)
                nxt = nxt.clone()
                for i, sp in enumerate(params):
                    lp = logprobs[i]
                    if sp.repetition_penalty != 1.0:
                        window = torch.tensor(state["fed"][i][-sp.repetition_context_size:], dtype=torch.int32, device=logits.device)
                        hip_ops.logits_penalty(logits[i], window, sp.repetition_penalty)
                        tok, lp = hip_ops.logprobs_argmax(logits[i])
                        nxt[i:i + 1] = tok
                    if closures[i] is not None:
                        nxt[i:i + 1] = closures[i](lp[None]).reshape(1).to(torch.int32)
                state["tokens"] = nxt
            return host_step

        def host_launches(params):
            n = 0
            for sp in params:
                n += 3 if sp.repetition_penalty != 1.0 else 0
                n += SAMPLE_LAUNCHES[sp.hip_spec()[0]] if sp.hip_spec() else 0
            return n

        def timed(step):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps

        def arm(params):
            """The tail for these requests (None: off), warmed until the step replays its graph; -> its kernel nodes."""
            if params is None:
                model.clear_batch_tail()
            else:
                model.set_batch_tail(B)
                drawn = 0
                model.write_batch_tail(list(range(B)), [sp.record(drawn, seed=100 + i) for i, sp in enumerate(params)], state["fed"])
            for _ in range(4):
                fused_step()
            return model.batch_graph_launches()

        forms = [("none", "fused", None)]
        for variant in ("top_k", "penalty", "mix"):
            forms += [(variant, "fused", requests(variant, B)), (variant, "host", requests(variant, B))]
        best = {}
        launches = {}
        for rnd in range(args.rounds):
            for variant, form, params in forms:                                   # the forms alternate inside every round
                if form == "fused":
                    launches[(variant, form)] = arm(params)
                    t = timed(fused_step)
                else:
                    launches[(variant, form)] = arm(None) + host_launches(params)
                    step = make_host_step(params)
                    for _ in range(2):
                        step()
                    t = timed(step)
                best[(variant, form)] = min(best.get((variant, form), 1e9), t)
        model.clear_batch_tail()
        for (variant, form), t in best.items():
            row = {"sequences": B, "requests": variant, "form": form, "ms_per_step": round(t * 1e3, 3), "tokens_per_s": round(B / t, 1),
                   "launches_per_step": launches[(variant, form)], "vs_no_tail": round(t / best[("none", "fused")], 3)}
            results.append(row)
            print(json.dumps(row), flush=True)
        for c in caches:
            c[0].page_manager.release()
    if args.out:
        Path(args.out).write_text(json.dumps({"model": "llama3-8b int4 g64 bf16 (synthetic weights)", "prompt": args.prompt, "steps": args.steps,
                                              "rounds": args.rounds, "results": results}, indent=1) + "\n")


if __name__ == "__main__":
    main()
