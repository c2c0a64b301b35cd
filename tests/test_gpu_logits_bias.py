"""-m gpu: logit_bias on 16-bit logits (pie_logits_bias).  Exact on storage bits: one fp32 addition and one rounding, which
numpy computes to the same bits; the first of duplicate ids owns the id, ids outside [0, V) are skipped, untouched ids keep their bits."""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import to_bits, to_dev
from tests.test_gpu_step_tail import assert_same_bits, specials

pytestmark = pytest.mark.gpu


def biased(bits: np.ndarray, ids, vals, dt: str) -> np.ndarray:
    """The definition on storage bits: entries in order, an id taken by an earlier entry or outside [0, V) skipped."""
    ids, vals = np.asarray(ids, np.int64), np.asarray(vals, np.float32)
    ok = (ids >= 0) & (ids < bits.size)
    _, first = np.unique(ids[ok], return_index=True)
    idx, add = ids[ok][first], vals[ok][first]
    out = bits.copy()
    with np.errstate(all="ignore"):
        out[idx] = po.to_bits((po.from_bits(bits[idx], dt).astype(np.float32) + add).astype(np.float32), dt)
    return out


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V", [7, 4099, 128256])
def test_logits_bias_op_bit_for_bit(dt, V):
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(V + len(dt))
    base = po.to_bits((rng.standard_normal(V) * 6).astype(np.float32), dt)
    sp = specials(dt)
    if V > 27:
        where = np.arange(len(sp)) * 3
        base[where], base[V - 1] = sp, sp[-1]
    else:
        where = np.arange(7)
        base[where] = sp[[0, 1, 2, 3, 6, 7, 8]]
    hot = np.unique(np.concatenate([where, [0, V - 1]]))      # every special value gets a bias
    pool = np.array([0.0, -0.0, 100.0, -100.0, 1e-3, -2.5, 7e4, -7e4, 1e-40, 0.3333], np.float32)   # 7e4 overflows f16; 1e-40 is an fp32 denormal
    ids_dev = torch.empty(1024, dtype=torch.int32, device="cuda")
    vals_dev = torch.empty(1024, dtype=torch.float32, device="cuda")
    checked = 0
    for n in (1, 300, 1024):
        some = rng.integers(0, V, n)
        some[: min(n, len(hot))] = rng.permutation(hot)[: min(n, len(hot))]
        tables = {
            "all equal": np.full(n, hot[n % len(hot)]),                           # n different biases on one id: the first wins
            "pairs of duplicates": np.repeat(rng.permutation(some)[: (n + 1) // 2], 2)[:n],
            "ids 0 and V - 1": np.concatenate([[0, V - 1], some])[:n] if n > 1 else np.array([V - 1]),
            "out of range": np.resize(np.array([-1, V]), n),
            "in and out of range": np.resize(np.array([-1, 0, V, V - 1, 1 << 30, -(1 << 31)]), n),
        }
        for name, ids in tables.items():
            assert ids.size == n
            vals = rng.permutation(np.resize(pool, n)) if n > 1 else pool[2:3]
            if name != "out of range":
                vals = vals + np.arange(n, dtype=np.float32) * np.float32(0.125)   # duplicates carry different biases
            logits = to_dev(base, dt)
            ids_dev[:n].copy_(torch.from_numpy(ids.astype(np.int32)))
            vals_dev[:n].copy_(torch.from_numpy(vals.astype(np.float32)))
            out = hip_ops.logits_bias(logits, ids_dev[:n], vals_dev[:n])
            assert out.data_ptr() == logits.data_ptr()
            got, want = to_bits(logits), biased(base, ids, vals, dt)
            assert_same_bits(got, want, dt, (name, n))
            untouched = np.ones(V, bool)
            untouched[[i for i in ids.tolist() if 0 <= i < V]] = False
            assert np.array_equal(got[untouched], base[untouched]), (name, n)
            if name == "out of range":
                assert np.array_equal(got, base), n
            checked += 1
    assert checked == 15
    # the first of duplicate ids owns the id: +2 then -100 on one small finite logit gives x + 2
    logits = to_dev(base, dt)
    hip_ops.logits_bias(logits, torch.tensor([4, 4], dtype=torch.int32, device="cuda"), torch.tensor([2.0, -100.0], device="cuda"))
    assert to_bits(logits)[4] == biased(base, [4], [2.0], dt)[4] != biased(base, [4], [-100.0], dt)[4]
    if dt == "float16":   # 65504 + 7e4 overflows to +inf, -inf stays -inf under any finite bias
        logits = to_dev(base, dt)
        idx = int(where[-2])                                                      # the largest finite positive value
        ninf = int(np.flatnonzero(base == 0xFC00)[0])
        hip_ops.logits_bias(logits, torch.tensor([idx, ninf], dtype=torch.int32, device="cuda"), torch.tensor([7e4, 7e4], device="cuda"))
        assert base[idx] == 0x7BFF and to_bits(logits)[idx] == 0x7C00 and to_bits(logits)[ninf] == 0xFC00
    for bad_n in (0, 1025):
        with pytest.raises(ValueError):
            hip_ops.logits_bias(to_dev(base, dt), torch.zeros(bad_n, dtype=torch.int32, device="cuda"), torch.zeros(bad_n, device="cuda"))
    with pytest.raises(ValueError):
        hip_ops.logits_bias(to_dev(base, dt), ids_dev[:4], vals_dev[:3])
