"""What XTC costs, on the 8B int4 model, batch 1 and the 32-row batched step.

1. The replayed decode step, ms per token and kernel nodes of the captured graph, for temp = 1 (categorical) and top_p = 0.9, each with
   and without XTC, each fused (the draw inside the replayed step) and host-orchestrated (the unconfigured step, then hip_ops.sample on
   its log-probabilities: launches = the step's graph + the sampler's own).
2. step_batch at 32 sequences with a batch tail (temp = 1 in every row), with and without a per-row XTC record in every row.
Method: every figure is the median of --windows windows; the forms of one comparison alternate inside every window, in an order that
flips from window to window, in this one process.  The spread (min .. max over the windows) is reported beside each median.
The weights are synthetic: few steps have two ids above the threshold, so the figures are the cost of the extra launch and of the
removed-or-not test in the others, not of a particular removed set (which only adds the special-id scan of at most 1 / threshold ids).

    python scripts/bench_xtc.py [--batch 32] [--windows 7] [--steps 16] [--out profiles/xtc_bench.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from proxy_inference_engine_amd import hip_ops  # noqa: E402
from proxy_inference_engine_amd.models.llama import Model, ModelArgs  # noqa: E402
from proxy_inference_engine_amd.models.utils import LLAMA3_8B, synthetic_checkpoint  # noqa: E402

XTC = (0.5, 0.1, (128001,))
SPECS = {"temp1": ("categorical", 1.0, 0.0, 0), "top_p0.9": ("top_p", 1.0, 0.9, 0)}
SAMPLER_LAUNCHES = {"categorical": 2, "top_p": 5}


def stat(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def alternate(forms: dict, arm, windows: int, steps: int) -> dict:
    """forms: name -> argument of arm(), which returns (step function, launches per step); per window every form is armed (4 untimed
    steps re-capture), then `steps` steps are timed."""
    ms, launches = {k: [] for k in forms}, {}
    names = list(forms)
    for wnd in range(windows):
        for name in (names if wnd % 2 == 0 else names[::-1]):
            step, launches[name] = arm(forms[name])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    return {k: {"ms_per_token": stat(v), "launches_per_step": launches[k]} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    cfg = dict(LLAMA3_8B)
    if args.layers:
        cfg["num_hidden_layers"] = args.layers
    V = cfg["vocab_size"]
    out = {"model": "llama3-8b int4 g64 bf16 (synthetic weights)", "prompt": args.prompt, "steps": args.steps, "windows": args.windows, "xtc": [XTC[0], XTC[1], list(XTC[2])]}
    model = Model(ModelArgs(**cfg), synthetic_checkpoint(cfg, seed=0, dtype=torch.bfloat16))
    torch.cuda.empty_cache()
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, V, (args.prompt,), generator=g).tolist()
    positions = args.prompt + 8 * args.windows * (args.steps + 4) + 16
    cache = model.make_cache()
    state = {"token": model.step(torch.tensor(prompt, dtype=torch.int32), cache)[0].clone()}
    rec = hip_ops.xtc_records([hip_ops.xtc_pack(*XTC)], "cuda")

    def arm1(form):
        spec, xtc, fused = form
        if fused:
            model.set_step_tail(sampler=spec, xtc=xtc)

            def step():
                state["token"] = model.step(None, cache)[0]
        else:
            model.set_step_tail()

            def step():
                lp = model.step(state["token"], cache)[1]
                state["token"] = hip_ops.sample(lp, *spec, xtc=rec if xtc else None).reshape(1).to(torch.int32)
        for _ in range(4):
            step()
        own = 0 if fused else SAMPLER_LAUNCHES[spec[0]] + (1 if xtc else 0)
        return step, model.graph_launches() + own

    forms = {}
    for name, spec in SPECS.items():
        for xtc in (None, XTC):
            for fused in (True, False):
                forms[f"{name}{'+xtc' if xtc else ''} {'fused' if fused else 'host'}"] = (spec, xtc, fused)
    out["step"] = alternate(forms, arm1, args.windows, args.steps)
    model.set_step_tail()
    print(json.dumps({"step": out["step"]}), flush=True)

    B = args.batch
    pages_per_seq = (positions + 63) // 64 + 1
    model.enable_paged_kv(num_pages=B * pages_per_seq + 4, max_blocks=pages_per_seq)
    caches = [model.make_cache() for _ in range(B)]
    state["tokens"] = model.prefill_batch([list(prompt) for _ in range(B)], caches)[0].clone()
    model.set_batch_tail(B)
    model.write_batch_tail(list(range(B)), [hip_ops.row_tail_pack("categorical", 1.0, seed=s) for s in range(B)])

    def stepb():
        state["tokens"] = model.step_batch(state["tokens"], caches)[0].clone()

    def armb(on):
        if on:
            model.set_batch_xtc(B)
            model.write_batch_xtc(list(range(B)), [XTC] * B)
        else:
            model.clear_batch_xtc()
        for _ in range(4):
            stepb()
        return stepb, model.batch_graph_launches()

    out["step_batch"] = {str(B): alternate({"temp1": False, "temp1+xtc": True}, armb, args.windows, args.steps)}
    model.clear_batch_xtc(), model.clear_batch_tail()
    print(json.dumps({"step_batch": out["step_batch"]}), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
