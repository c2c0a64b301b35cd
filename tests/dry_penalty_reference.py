"""The reference of the DRY penalty (include/pie_hip.h, "DRY penalty"), numpy: a plain restatement of the rule, position by
position.  The power is `M - allowed_length` separate np.float32 multiplications and the penalty one np.float32 subtraction (numpy
scalars do not fuse), then one conversion to T (round to nearest even; an f16 result beyond 65504 is inf)."""
import numpy as np
import torch

from tests._util import TORCH_DT

MAX_MATCH = 64


def penalties(window, V: int, multiplier: float, base: float, allowed_length: int, breakers=()) -> dict:
    """{id: (L, p)} for every id the rule penalises under the window c[0..n) (c[n-1] = the input id): L = M[id], p the np.float32 penalty."""
    c = [int(v) for v in np.asarray(window).reshape(-1)]
    n, brk = len(c), {int(b) for b in breakers}
    if float(np.float32(multiplier)) == 0.0 or n < 2 or c[n - 1] in brk:
        return {}
    M = {}
    for i in range(n - 1):
        if c[i] != c[n - 1]:
            continue
        t = c[i + 1]
        if t in brk or not 0 <= t < V:
            continue
        L = 1
        while L < min(i + 1, MAX_MATCH) and c[i - L] == c[n - 1 - L] and c[n - 1 - L] not in brk:
            L += 1
        M[t] = max(M.get(t, 0), L)
    out = {}
    with np.errstate(over="ignore"):
        for t, L in M.items():
            if L >= allowed_length:
                p = np.float32(multiplier)
                for _ in range(L - allowed_length):
                    p = np.float32(p * np.float32(base))
                out[t] = (L, p)
    return out


def apply(bits: np.ndarray, dt: str, window, multiplier: float, base: float, allowed_length: int, breakers=()) -> np.ndarray:
    """Storage bits (uint16 [V]) of the processed logits: x'[t] = T(f32(x[t]) - p) at the penalised ids, the stored bits elsewhere."""
    out = np.ascontiguousarray(bits).copy()
    pen = penalties(window, out.shape[-1], multiplier, base, allowed_length, breakers)
    if not pen:
        return out
    ids = sorted(pen)
    x = torch.from_numpy(out[ids].view(np.int16)).view(TORCH_DT[dt]).to(torch.float32).numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.array([np.float32(x[k]) - pen[t][1] for k, t in enumerate(ids)], np.float32)
    out[ids] = torch.from_numpy(y).to(TORCH_DT[dt]).view(torch.int16).numpy().view(np.uint16)
    return out


def ring_window(fed, pos: int, range_: int) -> list:
    """The window of a row whose fed ids by position are `fed` (fed[pos] = the input id)."""
    return list(fed[max(0, pos + 1 - range_): pos + 1])
