"""Sampler random state: the role mx.random.state plays for the reference's compiled samplers
(samplers/*.py: `@partial(mx.compile, inputs=mx.random.state, outputs=mx.random.state)`): a 64-bit seed plus a device-side call counter
per device for the HIP sampler's Philox stream (csrc/sampler.hip)."""
from __future__ import annotations

import torch

_hip_counters: dict[str, torch.Tensor] = {}
_hip_seed: int | None = None


def hip_state(device: torch.device) -> tuple[int, torch.Tensor]:
    """(seed, counter) for pie_sample on `device`: counter is a device int64[2] the kernel advances per call."""
    global _hip_seed
    if _hip_seed is None:
        import os
        _hip_seed = int.from_bytes(os.urandom(8), "little") & (2 ** 64 - 1)
    key = str(device)
    if key not in _hip_counters:
        _hip_counters[key] = torch.zeros(2, dtype=torch.int64, device=device)
    return _hip_seed, _hip_counters[key]


DRAFT_SEED_OFFSET = 0x9E3779B97F4A7C15
_draft_counters: dict[str, torch.Tensor] = {}


def draft_state(device: torch.device) -> tuple[int, torch.Tensor]:
    """(seed, counter) of a draft model's draws on `device`: the samplers' seed plus the 64-bit golden ratio, and a call
    counter of its own.  A drafter that drew under the target's seed would use, at the same call index, the Gumbels of the target's
    residual draw, and the accepted tokens would no longer be distributed as the target's."""
    seed_, _ = hip_state(device)
    key = str(device)
    if key not in _draft_counters:
        _draft_counters[key] = torch.zeros(2, dtype=torch.int64, device=device)
    return (seed_ + DRAFT_SEED_OFFSET) & (2 ** 64 - 1), _draft_counters[key]


def seed(n: int) -> None:
    """mx.random.seed(n): restarts every device's stream."""
    global _hip_seed
    _hip_seed = int(n) & (2 ** 64 - 1)
    for c in list(_hip_counters.values()) + list(_draft_counters.values()):
        c.zero_()
