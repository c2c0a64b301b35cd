"""XTC, "exclude top choices" (the reference's samplers/xtc.py is an empty placeholder; the rule is mlx-lm's apply_xtc, restated in
include/pie_hip.h and DESIGN.md 19): with probability `xtc_probability`, every token more probable than the least probable one above
`xtc_threshold` is hidden from the draw, except the special tokens.  The draw itself is the sampler kernel's (csrc/sampler.hip,
pie_sample_xtc): one launch more than the same sampler without XTC, the coin drawn on the device from the samplers' own stream."""
from __future__ import annotations

import math
from collections.abc import Callable

import torch

from .. import hip_ops


def check_xtc(probability, threshold, special_tokens=(), who: str = "xtc") -> tuple[float, float, tuple] | None:
    """(probability, threshold, special token ids) under the ABI's rules, or None when XTC is off (probability == 0, whatever the
    threshold): probability in [0, 1], threshold in (0, 0.5], at most 16 special tokens, each an int32 id.  ValueError otherwise (NaN
    included)."""
    p = float(probability)
    if not (math.isfinite(p) and 0.0 <= p <= 1.0):
        raise ValueError(f"{who}: `xtc_probability` has to be in [0, 1], got {probability!r}")
    if p == 0.0:
        return None
    t = float(threshold)
    if not (math.isfinite(t) and 0.0 < t <= 0.5):
        raise ValueError(f"{who}: `xtc_threshold` has to be in (0, 0.5], got {threshold!r}")
    ids = tuple(int(i) for i in special_tokens)
    if len(ids) > hip_ops.XTC_SPECIAL_MAX or any(not -2 ** 31 <= i < 2 ** 31 for i in ids):
        raise ValueError(f"{who}: at most {hip_ops.XTC_SPECIAL_MAX} `xtc_special_tokens`, each an int32 token id")
    return p, t, ids


def xtc_sampling(spec: tuple, xtc: tuple) -> Callable[[torch.Tensor], torch.Tensor]:
    """The host-orchestrated closure: hip_ops.sample's (mode, temp, p, k) under the XTC parameters `xtc` (check_xtc's result).  The
    record is uploaded once per device and then only read."""
    rec = hip_ops.xtc_pack(*xtc)
    on_device: dict = {}

    def sampler(logprobs: torch.Tensor) -> torch.Tensor:
        key = str(logprobs.device)
        if key not in on_device and logprobs.is_cuda:
            on_device[key] = hip_ops.xtc_records([rec], logprobs.device)
        return hip_ops.sample(logprobs, *spec, xtc=on_device.get(key, rec))

    return sampler
