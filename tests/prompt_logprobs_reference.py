"""The contract of pie_prompt_logprobs (include/pie_hip.h) restated in numpy -- TEST INFRASTRUCTURE, shared by
tests/test_prompt_logprobs_host.py (CPU) and tests/test_gpu_prompt_logprobs.py (-m gpu).

One row's record from its 16-bit logits, given as float32: lp = x - lse in float32, ranked as tests/top_logprobs_reference.py ranks
log-probabilities (value descending, id ascending).  The log-sum-exp is float64 here: the exact comparisons take theirs from the library's
own composition, the tolerance comparisons this one."""
from __future__ import annotations

import numpy as np

from tests import top_logprobs_reference as tref


def lse64(x: np.ndarray) -> float:
    """log(sum(exp(x))) of one row in float64; -inf for a row of -inf."""
    x = np.asarray(x, np.float64).reshape(-1)
    m = x.max()
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.exp(x - m).sum()))


def logprobs(x: np.ndarray, lse=None) -> np.ndarray:
    """float32 [V]: f32(x) - f32(lse), one float32 subtraction per id (lse None: lse64(x))."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    return x - np.float32(lse64(x) if lse is None else lse)


def reference(x: np.ndarray, n: int, target=None, count=None, lse=None):
    """One row's record: (ids int32 [n + 1], value bits uint32 [n + 1]), or None for a negative count (the row is left alone)."""
    return tref.reference(logprobs(x, lse), n, token=target, count=count)
