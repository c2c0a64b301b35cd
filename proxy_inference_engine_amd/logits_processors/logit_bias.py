"""logit_bias: the other processor the reference's factory builds (logits_params.hpp: logit_bias; logit_processor_factory.cpp, where its
body is a TODO).  Defined here: logits[id] = T(f32(logits[id]) + bias) for every listed id inside the vocabulary -- one fp32
addition, one rounding to the logits' type.  The processor carries `.ids` and `.values`: where the engine can, it runs the same edit inside
the decode step's tail (hip_ops.logits_bias's kernel, Model.set_step_tail) and never calls it."""
from __future__ import annotations

import math
from collections.abc import Callable, Mapping

import torch

MAX_ENTRIES = 1024  # one thread per entry of the kernel's single workgroup


def make_logit_bias(logit_bias: Mapping[int, float]) -> Callable:
    items = [(int(k), float(v)) for k, v in dict(logit_bias).items()]
    if not 1 <= len(items) <= MAX_ENTRIES:
        raise ValueError(f"logit_bias takes 1..{MAX_ENTRIES} entries, got {len(items)}")
    if len({k for k, _ in items}) != len(items):
        raise ValueError("logit_bias: a token id is listed twice")
    for k, v in items:
        if not 0 <= k < 2 ** 31 or not math.isfinite(v):
            raise ValueError(f"logit_bias: token ids must be non-negative int32 values and biases finite, got {k}: {v}")
    ids, values = tuple(k for k, _ in items), tuple(v for _, v in items)

    def logit_bias_processor(tokens, logits: torch.Tensor) -> torch.Tensor:
        V = logits.shape[-1]
        keep = [i for i, k in enumerate(ids) if k < V]  # ids beyond the vocabulary are skipped
        if keep:
            idx = torch.tensor([ids[i] for i in keep], dtype=torch.long, device=logits.device)
            add = torch.tensor([values[i] for i in keep], dtype=torch.float32, device=logits.device)
            logits[..., idx] = (logits[..., idx].float() + add).to(logits.dtype)
        return logits

    logit_bias_processor.ids, logit_bias_processor.values = ids, values
    return logit_bias_processor
