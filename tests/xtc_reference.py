"""XTC's definition in numpy (include/pie_hip.h; mlx-lm's apply_xtc): the removed set over fp32 log-probabilities with
fp32 compares, and a Python Philox-4x32-10 for the coin.  The comparator of the HIP op; nothing here touches a device."""
import math

import numpy as np

M32 = 0xFFFFFFFF
COIN_IDX4 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox-4x32-10 (Salmon et al. 2011): counter = four 32-bit words, key = two; returns four 32-bit words."""
    c = [int(x) & M32 for x in counter]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def coin_u(seed: int, call: int, row: int = 0) -> np.float32:
    """u of the coin: word 0 of the block with key `seed` and counter {0xFFFFFFFF, row, call}."""
    r = philox4x32_10((COIN_IDX4, row, call & M32, (call >> 32) & M32), (seed & M32, (seed >> 32) & M32))[0]
    return np.float32((np.float32(r >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24))


def coin(seed: int, call: int, probability: float, row: int = 0) -> bool:
    return bool(coin_u(seed, call, row) < np.float32(probability))


def log_threshold(threshold: float) -> np.float32:
    return np.float32(math.log(float(threshold)))


def removed_set(lp: np.ndarray, threshold: float, special=()) -> np.ndarray:
    """The removed set R as a bool [V] array -- the coin said yes.  lp fp32 [V]."""
    lp = np.asarray(lp, dtype=np.float32)
    cand = lp > log_threshold(threshold)                     # special ids are members like any other
    out = np.zeros(lp.shape, dtype=bool)
    if int(cand.sum()) < 2:
        return out
    m = lp[cand].min()
    out = lp > m                                             # ids tied at m stay
    for s in special:
        if 0 <= int(s) < lp.size:                            # an id outside the vocabulary is ignored
            out[int(s)] = False
    return out


def edited(lp: np.ndarray, removed: np.ndarray) -> np.ndarray:
    """What the sampler sees: lp with the removed set at -inf."""
    x = np.asarray(lp, dtype=np.float32).copy()
    x[removed] = -np.inf
    return x
