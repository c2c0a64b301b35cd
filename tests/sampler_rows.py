"""Designed rows of fp32 log-probabilities for the sampler and logits-tail tests -- TEST INFRASTRUCTURE, shared by
tests/test_host_logic.py (CPU) and tests/test_gpu_sampler.py / tests/test_gpu_logits_tail.py (-m gpu).

Random standard-normal rows never reach the code that decides ties, masks or a boundary between workgroups; these rows do.  The
sampler kernel (csrc/sampler.hip) gives every workgroup a slice of SLICE = 512 ids, so the rows place their ties and masked ids
across slices on purpose.  Every row is seeded: the same (family, V, seed) always gives the same bits."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

SLICE = 512                     # ids per workgroup of csrc/sampler.hip (SMP_SLICE)
V_MAX = 1024 * SLICE            # the ABI limit of pie_sample (SMP_MAX_WGS x SMP_SLICE)
VOCABS = [2, 511, 512, 513, 32000, 50257, 128256, 151936, 152064, V_MAX]
TEMPS = [0.05, 0.7, 1.0, 3.0]


@dataclass
class Row:
    name: str
    lp: np.ndarray              # fp32 [V]
    temp: float = 1.0
    top_k: int = 5              # a k that lands where the row's designer wanted it
    top_p: float = 0.9
    min_p: float = 0.1
    keep: int = 1               # min_tokens_to_keep of the min-p cases that take the union
    notes: dict = field(default_factory=dict)

    @property
    def V(self) -> int:
        return int(self.lp.shape[0])


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> the nearest bf16 value (round to nearest even), kept as fp32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16
    return b.astype(np.uint32).view(np.float32)


def log_softmax32(logits: np.ndarray) -> np.ndarray:
    """fp32 logits - fp32(log-sum-exp computed in float64): equal logits give bit-equal log-probs."""
    z = logits.astype(np.float64)
    m = z[np.isfinite(z)].max() if np.isfinite(z).any() else 0.0
    lse = np.float32(m + np.log(np.exp(z - m).sum()))
    return (logits.astype(np.float32) - lse).astype(np.float32)


def _spread_ids(rng, V, n, min_slices):
    """n distinct ids that touch at least min(min_slices, number of slices) different slices, in random order."""
    n_sl = (V + SLICE - 1) // SLICE
    sl = rng.choice(n_sl, size=min(n_sl, max(min_slices, 1)), replace=False)
    first = np.array([min(s * SLICE + int(rng.integers(SLICE)), V - 1) for s in sl])
    first = np.unique(first)
    rest = np.setdiff1d(np.arange(V), first)
    more = rng.choice(rest, size=max(n - len(first), 0), replace=False)
    return np.concatenate([first, more])[:n]


def quantized(V, seed=0, temp=1.0):
    """log-softmax of bf16-rounded logits: a few hundred distinct values, so exact ties everywhere (top-k's boundary included)."""
    rng = np.random.default_rng(seed)
    logits = bf16_round((rng.standard_normal(V) * 2.5).astype(np.float32))
    lp = log_softmax32(logits)
    srt = np.sort(lp)[::-1]
    k = min(max(1, V // 50), V - 1)
    while k < V - 1 and srt[k - 1] != srt[k]:     # move k into a tie class when the row has one there
        k += 1
    if k >= V - 1:
        k = max(1, min(V // 50, V - 1))
    return Row("quantized", lp, temp=temp, top_k=max(1, min(k, V - 1)), top_p=0.8, min_p=0.05, keep=min(3, V))


def wide_tie(V, seed=0, last_slice=False, temp=1.0):
    """~40 ids share one value at the top-k boundary: 20 ids lie above it and k takes 17 of the 40 (lowest index first).  The class
    touches >= 8 slices and holds adjacent (even, odd) pairs -- ids one thread of the kernel owns together -- or, with last_slice,
    lies wholly in the last slice."""
    rng = np.random.default_rng(seed + 7)
    lp = (rng.standard_normal(V) * 0.5 - 12.0).astype(np.float32)          # everything else far below the class
    n_tie, n_above = 40, 20
    if last_slice:
        lo = ((V - 1) // SLICE) * SLICE
        tie = np.arange(lo, V)[:n_tie] if V - lo >= n_tie else np.arange(V - n_tie, V)
    else:
        base = _spread_ids(rng, V, n_tie - 8, 8)
        pairs = []
        for b in base[:4]:                                                   # four (even, odd) pairs
            e = int(b) & ~1
            pairs += [e, e + 1] if e + 1 < V else [e - 2, e - 1]
        tie = np.unique(np.concatenate([base, np.array(pairs)]))[:n_tie]
    rest = np.setdiff1d(np.arange(V), tie)
    above = rng.choice(rest, size=n_above, replace=False)
    lp[tie] = np.float32(-3.0)
    lp[above] = (-2.0 + rng.random(n_above) * 1.5).astype(np.float32)
    lp = log_softmax32(lp)
    name = "wide_tie_last_slice" if last_slice else "wide_tie"
    return Row(name, lp, temp=temp, top_k=n_above + 17, top_p=0.5, min_p=0.2, keep=n_above + 5,
               notes=dict(tie=np.sort(tie), above=np.sort(above)))


def sparse(V, n, seed=0, temp=1.0):
    """only n ids are finite, the rest -inf; slice 1 (or the last slice) is entirely -inf.  top_k = n + 5 > n."""
    rng = np.random.default_rng(seed + 13)
    lp = np.full(V, -np.inf, np.float32)
    banned = np.arange(SLICE, min(2 * SLICE, V)) if V > 2 * SLICE else np.arange(V - 1, V)
    allowed = rng.choice(np.setdiff1d(np.arange(V), banned), size=min(n, V - len(banned)), replace=False)
    lp[allowed] = (rng.standard_normal(len(allowed)) * 1.5).astype(np.float32)
    lp = log_softmax32(lp)
    return Row(f"sparse{n}", lp, temp=temp, top_k=min(len(allowed) + 5, V - 1), top_p=0.9, min_p=0.01, keep=min(len(allowed) + 2, V),
               notes=dict(allowed=np.sort(allowed)))


def all_inf(V, temp=1.0):
    return Row("all_inf", np.full(V, -np.inf, np.float32), temp=temp, top_k=min(3, V - 1), top_p=0.9, min_p=0.1, keep=min(2, V))


def one_hot(V, seed=0, temp=1.0):
    """one id with probability ~1, the rest 40+ nats below it."""
    rng = np.random.default_rng(seed + 17)
    lp = (-45.0 - rng.random(V) * 10.0).astype(np.float32)
    lp[int(rng.integers(V))] = 0.0
    return Row("one_hot", log_softmax32(lp), temp=temp, top_k=min(4, V - 1), top_p=0.5, min_p=0.5, keep=min(3, V))


def uniform(V, temp=1.0):
    return Row("uniform", np.full(V, -np.float32(math.log(V)), np.float32), temp=temp, top_k=max(1, min(V // 3, V - 1)), top_p=0.7,
               min_p=0.9, keep=min(4, V))


def topp_tie(V, seed=0, temp=1.0):
    """a tie class of 6 ids straddles the top-p threshold: the rest of the row holds 5 % of the mass, the 6 tied ids 5 % each, 10 large
    ids 6-7 % each (65 %).  top_p = 0.775: the ascending cumulative mass crosses 1 - top_p = 0.225 inside the tie class (it covers
    0.05 .. 0.35), 12.5 % of the mass from either end of the class and 2.5 % from the nearest step of the reference's cumulative sum.  The
    kernel keeps the whole class; the reference's sorted cumulative sum keeps its last 3 members."""
    rng = np.random.default_rng(seed + 19)
    ids = rng.choice(V, size=16, replace=False)
    big, tie = ids[:10], ids[10:]
    rest = np.setdiff1d(np.arange(V), ids)
    p = np.zeros(V)
    p[big] = 0.06 + 0.01 * np.arange(10) / 9.0
    p[tie] = 0.05
    p[rest] = 0.5 + rng.random(len(rest))
    p[rest] *= 0.05 / p[rest].sum()
    lp = log_softmax32(np.log(p).astype(np.float32))
    # at temp = 1 the masses are as designed; other temperatures move them (the kernel's rule still holds, the margins are not designed)
    return Row("topp_tie", lp, temp=temp, top_k=12, top_p=0.775, min_p=0.5, keep=12, notes=dict(tie=np.sort(tie), big=np.sort(big)))


def merged_by_temp(V, seed=0):
    """two distinct log-probs that fp32(x * fp32(1 / 3.0)) maps to ONE value: at temp 3.0 they become a tie at the top-k boundary.  The
    larger of the two sits at the HIGHER index, so a float64 restatement keeps the other id than the fp32 one does."""
    rng = np.random.default_rng(seed + 23)
    inv = np.float32(1.0 / 3.0)
    while True:
        a = np.float32(-rng.random() * 2.0 - 1.0)
        b = np.nextafter(a, np.float32(0.0))                              # b > a, adjacent
        if np.float32(a * inv) == np.float32(b * inv):
            break
    lp = (rng.standard_normal(V) * 0.3 - 20.0).astype(np.float32)
    lo, hi = sorted(rng.choice(V, size=2, replace=False))
    above = rng.choice(np.setdiff1d(np.arange(V), [lo, hi]), size=min(4, V - 2), replace=False)
    lp[above] = np.float32(0.0) + (rng.random(len(above)) * 0.25).astype(np.float32)
    lp[lo], lp[hi] = a, b
    k = len(above) + 1
    return Row("merged_by_temp", lp, temp=3.0, top_k=k, top_p=0.5, min_p=0.1, keep=k, notes=dict(lo=int(lo), hi=int(hi)))


def families(V, seed=0):
    """Every designed family at vocabulary size V (the ones that fit)."""
    out = [quantized(V, seed, temp=TEMPS[seed % len(TEMPS)]), all_inf(V), one_hot(V, seed), uniform(V)]
    if V >= 64:
        out += [wide_tie(V, seed), wide_tie(V, seed, last_slice=True), topp_tie(V, seed), merged_by_temp(V, seed)]
    for n in (1, 3, 600):
        if n + 6 < V:
            out.append(sparse(V, n, seed))
    return out


def make(name, V, seed=0):
    """One designed row by its family name (the names families() gives)."""
    for row in families(V, seed):
        if row.name == name:
            return row
    raise KeyError(f"no family {name!r} at V = {V}")


def names(V):
    """families(V)'s names without building the rows."""
    out = ["quantized", "all_inf", "one_hot", "uniform"]
    if V >= 64:
        out += ["wide_tie", "wide_tie_last_slice", "topp_tie", "merged_by_temp"]
    return out + [f"sparse{n}" for n in (1, 3, 600) if n + 6 < V]
