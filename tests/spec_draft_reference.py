"""Speculative sampling's definition in float64 numpy (include/pie_hip.h: pie_spec_verify_draft): dist over a kept set, the
accept rule given u, the residual, u_i from the Python Philox of tests/xtc_reference.py, and a host simulation of one round for the
chi-square tests.  The comparator of the HIP op; nothing here touches a device."""
import numpy as np

from tests.xtc_reference import COIN_IDX4, M32, philox4x32_10

U_IDX4 = 0xFFFFFFFE
DRAFT_SEED_OFFSET = 0x9E3779B97F4A7C15
CHI2_INPUTS = dict(V=1000, k=12, temp=0.8, trials=2000)   # the inputs the chi-square bound was worked out for: keep them
CHI2_BOUND_11 = 48.87                                     # the 1 - 1e-6 quantile of chi-square with 11 degrees of freedom


def inv_temp(temp: float) -> np.float64:
    """fp32(1 / temp) as the sampler derives it, widened."""
    return np.float64(np.float32(1.0 / float(temp)))


def dist(lp: np.ndarray, kept: np.ndarray, temp: float) -> np.ndarray:
    """dist(x) = exp((lp[x] - max_K lp) * inv_temp) / sum_K exp(...) on the kept set, 0 elsewhere; all zeros for an empty kept set."""
    lp, kept = np.asarray(lp, dtype=np.float64), np.asarray(kept, dtype=bool)
    out = np.zeros(lp.shape, dtype=np.float64)
    if not kept.any():
        return out
    e = np.exp((lp[kept] - lp[kept].max()) * inv_temp(temp))
    out[kept] = e / e.sum()
    return out


def accepts(p_d: float, q_d: float, u: float) -> bool:
    """The accept test on fp32 values: one fp32 multiply, one fp32 compare."""
    p_d, q_d, u = np.float32(p_d), np.float32(q_d), np.float32(u)
    return bool(q_d > np.float32(0)) and bool(np.float32(u * q_d) < p_d)


def accepted_prefix(P: np.ndarray, Q: np.ndarray, draft, us) -> int:
    """n_acc for P [rows, V], Q [rows - 1, V]: an id outside [0, V) is refused and never indexed."""
    V, n = P.shape[1], 0
    for i, d in enumerate(draft):
        if not 0 <= int(d) < V or not accepts(P[i, int(d)], Q[i, int(d)], us[i]):
            break
        n += 1
    return n


def residual(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """log(max(0, p - q)) in float64, -inf where the difference is <= 0."""
    diff = np.asarray(p, dtype=np.float64) - np.asarray(q, dtype=np.float64)
    out = np.full(diff.shape, -np.inf)
    out[diff > 0] = np.log(diff[diff > 0])
    return out


def accept_u(seed: int, call: int) -> np.float32:
    """u of the accept test: word 0 of the block with key `seed` and counter {0xFFFFFFFE, 0, call lo, call hi}."""
    r = philox4x32_10((U_IDX4, 0, call & M32, (call >> 32) & M32), (seed & M32, (seed >> 32) & M32))[0]
    return np.float32((np.float32(r >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24))


def index_words_are_disjoint(V: int) -> bool:
    """The accept test's index word is neither the coin's nor a vocabulary index's (ids 4 i .. 4 i + 3 share block i <= (V - 1) / 4)."""
    return U_IDX4 != COIN_IDX4 and U_IDX4 > (int(V) - 1) // 4


def draft_seed(seed: int) -> int:
    return (int(seed) + DRAFT_SEED_OFFSET) & (2 ** 64 - 1)


def top_k_kept(lp: np.ndarray, k: int) -> np.ndarray:
    kept = np.zeros(lp.shape, dtype=bool)
    kept[np.argsort(-np.asarray(lp, dtype=np.float64), kind="stable")[:k]] = True
    return kept


def chi2_inputs(seed: int):
    """(P, Q) of the chi-square tests: V = 1000, top-k 12 at temp 0.8, logits N(0, 2) for P and the same plus N(0, 1) for Q, as
    log-softmax rows in fp32."""
    rng = np.random.default_rng(seed)
    c = CHI2_INPUTS
    lp_logits = rng.normal(0.0, 2.0, c["V"])
    lq_logits = lp_logits + rng.normal(0.0, 1.0, c["V"])

    def log_softmax(x):
        return (x - x.max() - np.log(np.exp(x - x.max()).sum())).astype(np.float32)

    lp, lq = log_softmax(lp_logits), log_softmax(lq_logits)
    return lp, lq, dist(lp, top_k_kept(lp, c["k"]), c["temp"]), dist(lq, top_k_kept(lq, c["k"]), c["temp"])


def simulate_first_token(P: np.ndarray, Q: np.ndarray, trials: int, seed: int, rule: str = "exact") -> np.ndarray:
    """The first output token of `trials` rounds of one draft: rule "exact" (accept iff u Q(x) < P(x), else draw from the normalised
    residual), "always" (accept every draft) or "redraw" (on refusal draw from P instead of the residual)."""
    rng = np.random.default_rng(seed)
    res = np.maximum(P - Q, 0.0)
    res = res / res.sum() if res.sum() > 0 else P
    out = np.empty(trials, dtype=np.int64)
    for t in range(trials):
        x, u = rng.choice(P.size, p=Q), rng.random()
        if rule == "always" or u * Q[x] < P[x]:
            out[t] = x
        else:
            out[t] = rng.choice(P.size, p=res if rule == "exact" else P)
    return out


def chi2_statistic(tokens: np.ndarray, P: np.ndarray) -> tuple[float, int, int]:
    """(Pearson's chi-square of `tokens` against P over P's support, the degrees of freedom, how many tokens fell outside the support)."""
    support = np.flatnonzero(P > 0)
    counts = np.bincount(np.asarray(tokens, dtype=np.int64), minlength=P.size)
    expected = P[support] * len(tokens)
    stat = float((((counts[support] - expected) ** 2) / expected).sum())
    return stat, support.size - 1, int(len(tokens) - counts[support].sum())
