"""Frequency and presence penalties: logits[v] -= frequency_penalty * c[v] + presence_penalty wherever c[v] > 0, c[v] = how
often id v occurs among the tokens GENERATED so far for the request -- the prompt's tokens do not count.

Installed when either penalty is non-zero.  The processor carries `.frequency_penalty`, `.presence_penalty` and `.prompt_len`: where the
request can take the decode step's configured tail the engine runs the same edit inside the step (hip_ops.logits_count_penalty_rows'
kernel, Model.set_step_tail) and never calls it.  Called (a structuring engine, a tensor-parallel model, a processor list the tail cannot
take), it is host-orchestrated on the same kind of device state -- an int32 [1, V] count buffer and one record -- and the same kernel:
the new generated ids are added to the counts, then the stand-alone op edits the logits in place.  No torch arithmetic touches a logit."""
from __future__ import annotations

from collections.abc import Callable

import torch

from .. import hip_ops


def count_penalty_logits_processor(frequency_penalty: float = 0.0, presence_penalty: float = 0.0, prompt_len: int = 0) -> Callable:
    f, p = hip_ops.check_count_penalties(frequency_penalty, presence_penalty, "count_penalty_logits_processor")
    if int(prompt_len) < 0:
        raise ValueError(f"prompt_len must be non-negative, got {prompt_len}")
    state: dict = {"counts": None, "records": None, "counted": 0}

    def count_penalty_processor(tokens, logits: torch.Tensor) -> torch.Tensor:
        start = count_penalty_processor.prompt_len
        generated = list(tokens[start:])
        V = logits.shape[-1]
        counts = state["counts"]
        if counts is None or counts.shape[1] != V or counts.device != logits.device or len(generated) < state["counted"]:
            counts = state["counts"] = torch.zeros((1, V), dtype=torch.int32, device=logits.device)
            state["records"] = hip_ops.count_penalty_records([hip_ops.count_penalty_pack(f, p, start)], logits.device)
            state["counted"] = 0
        new = [int(t) for t in generated[state["counted"]:] if 0 <= int(t) < V]
        state["counted"] = len(generated)
        if new:
            at = torch.tensor(new, dtype=torch.long, device=logits.device)
            counts[0].index_add_(0, at, torch.ones(at.numel(), dtype=torch.int32, device=logits.device))
        rows = logits.reshape(1, V)
        if not rows.is_contiguous() or rows.data_ptr() != logits.data_ptr():
            rows = rows.contiguous()
            hip_ops.logits_count_penalty_rows(rows, state["records"], counts)
            logits.copy_(rows.reshape(logits.shape))
            return logits
        hip_ops.logits_count_penalty_rows(rows, state["records"], counts)
        return logits

    def reset(prompt_len: int) -> None:
        """A new request: `prompt_len` prompt tokens in front, nothing generated, zero counts."""
        count_penalty_processor.prompt_len = int(prompt_len)
        state["counts"], state["records"], state["counted"] = None, None, 0

    count_penalty_processor.frequency_penalty, count_penalty_processor.presence_penalty = f, p
    count_penalty_processor.prompt_len = int(prompt_len)
    count_penalty_processor.reset = reset
    return count_penalty_processor
