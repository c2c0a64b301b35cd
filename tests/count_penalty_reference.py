"""The reference of the frequency / presence penalties, CPU torch: x'[v] = T(f32(x[v]) - (f32(f) * (float)c[v] + f32(p))) where
c[v] > 0, the stored T value where c[v] == 0 -- three separate fp32 tensor ops (mul, add, sub: no fused multiply-add can form) and one
conversion to T (round to nearest even; an f16 result beyond 65504 is inf).  `generated_counts` is the expected count state."""
import numpy as np
import torch

from tests._util import TORCH_DT


def count_penalty_reference(bits: np.ndarray, counts: np.ndarray, freq: float, pres: float, dt: str) -> np.ndarray:
    """Storage bits (uint16 [..., V]) of the processed logits for int counts [..., V]."""
    x = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(TORCH_DT[dt])
    c = torch.from_numpy(np.ascontiguousarray(counts).astype(np.int32))
    f, p = torch.tensor(freq, dtype=torch.float32), torch.tensor(pres, dtype=torch.float32)
    pen = torch.add(torch.mul(f, c.to(torch.float32)), p)
    y = torch.sub(x.to(torch.float32), pen).to(TORCH_DT[dt])
    out = torch.where(c > 0, y, x)
    return out.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def generated_counts(ids, V: int) -> np.ndarray:
    """int32 [V]: how often each in-range id occurs among the generated ids."""
    ids = np.asarray(list(ids), dtype=np.int64).reshape(-1)
    ids = ids[(ids >= 0) & (ids < V)]
    return np.bincount(ids, minlength=V).astype(np.int32)
