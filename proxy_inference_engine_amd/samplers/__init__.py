"""Samplers (mirror of samplers/__init__.py:11-46 of the reference).

`make_sampler(temp=0)` -- the greedy branch (samplers/__init__.py:37-38) -- is the parity target of the decode
path and runs in the fused HIP tail (argmax of the fp32 log-probabilities, first maximal index).
The stochastic branches (top-p, min-p, top-k, categorical: samplers/{top_p,min_p,top_k,categorical}.py, SURVEY.md
8f-4) are sort-free HIP kernels (csrc/sampler.hip) on the device that holds the log-probabilities (no host sync: the
drawn token stays a device tensor and feeds the next step; host tensors are refused -- the reference's definitions restated
with torch ops live in tests/sampler_reference.py as the comparator); their random stream is Philox, not MLX's, so parity
is the kept-token set (exact) and the distribution, not the individual draw.  `seed(n)` = mx.random.seed(n).
"""
from __future__ import annotations

from collections.abc import Callable

import torch

from .. import hip_ops
from ._rng import seed
from .categorical import categorical_sampling
from .min_p import min_p_sampling
from .top_k import top_k_sampling
from .top_p import top_p_sampling
from .xtc import check_xtc, xtc_sampling


def greedy(logprobs: torch.Tensor) -> torch.Tensor:
    """logprobs [B=1, V] (fp32 or 16-bit) -> token ids [1] int32: argmax over the last axis."""
    x = logprobs.reshape(-1)
    if x.dtype == torch.float32:
        # argmax of fp32 log-probabilities: monotone in the logits, done by the same tail kernel on a 16-bit
        # view is not possible, so use the fp32 path of the tail kernel's host mirror
        return _argmax_f32(x)
    tok, _ = hip_ops.logprobs_argmax(x)
    return tok


def _argmax_f32(x: torch.Tensor) -> torch.Tensor:
    # first maximal index (mx.argmax semantics); tiny host-glue reduction over V values
    m = x.max()
    idx = torch.nonzero(x == m)[0, 0]
    return idx.to(torch.int32).reshape(1)


def sampler_spec(temp: float = 0.0, top_p: float = 0.0, min_p: float = 0.0, min_tokens_to_keep: int = 1, top_k: int = -1) -> tuple | None:
    """Which branch a request's sampler settings select (samplers/__init__.py:37-46 of the reference): None for greedy (temp == 0), else
    (mode, temp, p, k) as hip_ops.sample takes them -- top-p for 0 < top_p < 1, else min-p, else top-k, else categorical."""
    if temp == 0:
        return None
    if top_p > 0 and top_p < 1.0:
        return ("top_p", temp, top_p, 0)
    if min_p != 0.0:
        return ("min_p", temp, min_p, min_tokens_to_keep)
    if top_k > 0:
        return ("top_k", temp, 0.0, top_k)
    return ("categorical", temp, 0.0, 0)


def make_sampler(temp: float = 0.0, top_p: float = 0.0, min_p: float = 0.0, min_tokens_to_keep: int = 1,
                 top_k: int = -1, xtc_probability: float = 0.0, xtc_threshold: float = 0.0,
                 xtc_special_tokens=()) -> Callable[[torch.Tensor], torch.Tensor]:
    """The stochastic closures carry `hip_spec = (mode, temp, p, k)` -- hip_ops.sample's arguments -- so the engine can run the same
    draw inside the decode step's tail (Model.set_step_tail) instead of calling the closure.
    xtc_probability > 0 (with xtc_threshold in (0, 0.5] and up to 16 xtc_special_tokens; samplers/xtc.py): the chosen
    branch draws under XTC, and the closure also carries `hip_xtc = (probability, threshold, special ids)` -- set_step_tail's `xtc`.
    The greedy branch ignores XTC, as upstream's make_sampler does; with xtc_probability == 0 nothing changes."""
    spec = sampler_spec(temp, top_p, min_p, min_tokens_to_keep, top_k)
    if spec is None:
        return greedy
    xtc = check_xtc(xtc_probability, xtc_threshold, xtc_special_tokens, "make_sampler")
    sampler = {"top_p": lambda x: top_p_sampling(x, top_p, temp),
               "min_p": lambda x: min_p_sampling(x, min_p, min_tokens_to_keep, temp),
               "top_k": lambda x: top_k_sampling(x, top_k, temp),
               "categorical": lambda x: categorical_sampling(x, temp)}[spec[0]]
    if xtc is not None:
        sampler = xtc_sampling(spec, xtc)
        sampler.hip_xtc = xtc
    sampler.hip_spec = spec
    return sampler


greedy.is_greedy = True  # lets the engine pick the fused tail
