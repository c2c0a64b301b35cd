"""The DRY ("don't repeat yourself") sequence-repetition penalty: the token that would extend a verbatim repeat of the
sequence's tail of at least allowed_length ids loses multiplier * base ** (repeat length - allowed_length); a repeat does not cross a
sequence breaker (token ids here: no tokenizer is in scope).

Installed when dry_multiplier != 0.  The processor carries `.dry_multiplier`, `.dry_base`, `.dry_allowed_length`, `.dry_range` and
`.dry_sequence_breakers`: where the request can take the decode step's configured tail the engine runs the same edit inside the step
(hip_ops.logits_dry_penalty's kernel, Model.set_step_tail) and never calls it.  Called (a structuring engine, a tensor-parallel model, a
processor list the tail cannot take), it runs the stand-alone op on the last `range` ids.  No torch arithmetic touches a logit."""
from __future__ import annotations

from collections.abc import Callable

import torch

from .. import hip_ops


def dry_logits_processor(multiplier: float, base: float = 1.75, allowed_length: int = 2, range: int = 1024, sequence_breakers=()) -> Callable:
    m, b, a, r, brk = hip_ops.check_dry(multiplier, base, allowed_length, range, sequence_breakers, "dry_logits_processor")
    state: dict = {"breakers": None}

    def dry_processor(tokens, logits: torch.Tensor) -> torch.Tensor:
        window = list(tokens[-r:])
        if m == 0.0 or len(window) < 2:
            return logits
        V = logits.shape[-1]
        if state["breakers"] is None or state["breakers"].device != logits.device:
            state["breakers"] = torch.tensor(brk, dtype=torch.int32, device=logits.device)
        ids = torch.tensor(window, dtype=torch.int32, device=logits.device)
        row = logits.reshape(V)
        if not row.is_contiguous() or row.data_ptr() != logits.data_ptr():
            row = row.contiguous()
            hip_ops.logits_dry_penalty(row, ids, m, b, a, state["breakers"])
            logits.copy_(row.reshape(logits.shape))
            return logits
        hip_ops.logits_dry_penalty(row, ids, m, b, a, state["breakers"])
        return logits

    dry_processor.dry_multiplier, dry_processor.dry_base, dry_processor.dry_allowed_length = m, b, a
    dry_processor.dry_range, dry_processor.dry_sequence_breakers = r, brk
    return dry_processor
