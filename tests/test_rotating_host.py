"""CPU: RotatingKVCache's host protocol against a restatement of the reference's rules (cache/kv_cache/rotating.py), written from the
positions each stored row holds rather than from the cache's own index arithmetic."""
import numpy as np
import pytest
import torch

from proxy_inference_engine_amd.cache import BaseCache, PromptCache, ReusableKVCache, RotatingKVCache
from proxy_inference_engine_amd.models import base

H, D = 2, 4


class RefRing:
    """Rows as (position, k, v) in the reference's row order; idx = the reference's write index."""

    def __init__(self, W, keep):
        self.W, self.keep, self.rows, self.idx, self.offset = W, keep, [], 0, 0

    def _window(self):
        """The retained window in temporal order: all rows while nothing was evicted, else the sinks and the newest W - keep."""
        by_pos = {r[0]: r for r in self.rows}
        if self.offset <= self.W:
            return [by_pos[p] for p in range(self.offset)]
        pos = list(range(self.keep)) + list(range(self.offset - (self.W - self.keep), self.offset))
        return [by_pos[p] for p in pos]

    def update(self, k, v):
        L = k.shape[0]
        new = [(self.offset + i, k[i], v[i]) for i in range(L)]
        if L >= 2:
            self.rows = (self._window() if self.rows else []) + new
            self.idx = len(self.rows)
        else:
            if len(self.rows) > self.W:  # a long store: cut to the window, write at the first ring row
                self.rows, self.idx = self._window(), self.W
            if self.idx == self.W:
                self.idx = self.keep
            if self.idx == len(self.rows):
                self.rows.append(new[0])
            else:
                self.rows[self.idx] = new[0]
            self.idx += 1
        self.offset += L
        n = self.offset if L == 1 and self.offset < self.W else len(self.rows)
        return self.arrays(n)

    def arrays(self, n):
        rows = self.rows[:n]
        return np.stack([r[1] for r in rows], 1), np.stack([r[2] for r in rows], 1), [r[0] for r in rows]

    def state(self):
        n = min(self.offset, len(self.rows))
        return self.arrays(n)


def _rows(rng, L):
    return rng.standard_normal((H, L, D)).astype(np.float32), rng.standard_normal((H, L, D)).astype(np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))[None]


def _run(seq, W, keep, seed=0, check=None):
    rng = np.random.default_rng(seed)
    c, ref = RotatingKVCache(W, keep=keep, step=8), RefRing(W, keep)
    for L in seq:
        k, v = _rows(rng, L)
        gk, gv = c.update_and_fetch(_t(k), _t(v))
        rk, rv, _ = ref.update(k.transpose(1, 0, 2), v.transpose(1, 0, 2))
        assert torch.equal(gk[0], torch.from_numpy(rk)) and torch.equal(gv[0], torch.from_numpy(rv)), (W, keep, L, c.offset)
        assert c.offset == ref.offset and c.meta_state == tuple(map(str, (keep, W, 8, ref.offset, ref.idx)))
        sk, sv = c.state
        rk, rv, _ = ref.state()
        assert torch.equal(sk[0], torch.from_numpy(rk)) and torch.equal(sv[0], torch.from_numpy(rv))
        if check:
            check(c, ref)
    return c, ref


SEQS = [
    [1] * 40,                                 # decode only: fills, wraps several times
    [5] + [1] * 30 + [2] + [1] * 10,          # short prompt, a 2-row chunk on the full ring
    [20] + [1] * 12 + [5, 5] + [1] * 20,      # prompt past the window, two chunks back to back
    [3, 20, 1, 2, 1, 5] + [1] * 17,           # chunks from a part-full ring
    [2] * 15 + [1] * 3,
]


@pytest.mark.parametrize("W", [8, 16])
@pytest.mark.parametrize("keep", [0, 4])
@pytest.mark.parametrize("seq", range(len(SEQS)))
def test_update_and_fetch_matches_restatement(W, keep, seq):
    _run(SEQS[seq], W, keep, seed=seq)


def test_decode_attends_sinks_plus_newest_once_full():
    W, keep = 8, 4

    def check(c, ref):
        _, _, pos = ref.arrays(len(ref.rows))
        if ref.offset >= W and len(ref.rows) == W:
            assert sorted(pos) == list(range(keep)) + list(range(ref.offset - (W - keep), ref.offset))
    _run([1] * 30, W, keep, check=check)


def test_trim_and_trimmable():
    c, _ = _run([5], 8, 4)
    assert c.is_trimmable()
    assert c.trim(2) == 2 and c.offset == 3 and c.meta_state[3:] == ("3", "3")
    k = torch.ones((1, H, 1, D))
    gk, _ = c.update_and_fetch(k, k)
    assert gk.shape[2] == 4 and torch.equal(gk[0, :, 3], k[0, :, 0])
    c2, _ = _run([1] * 9, 8, 4)
    assert not c2.is_trimmable()
    assert not RotatingKVCache(8).is_trimmable()  # nothing stored yet, as in the reference


def test_to_quantized_is_identity_and_bad_sizes_refused():
    c = RotatingKVCache(16, keep=4)
    assert c.to_quantized(bits=4) is c
    for W, keep in ((0, 0), (4, 4), (4, 5), (8, -1)):
        with pytest.raises(ValueError):
            RotatingKVCache(W, keep=keep)


def test_make_kv_cache_types():
    class M:
        layers = [0, 1, 2]
        _page_pool = None

        def make_cache(self):
            return [ReusableKVCache() for _ in self.layers]
    caches = BaseCache.make_kv_cache(M(), max_kv_size=32)
    assert len(caches) == 3 and all(isinstance(c, RotatingKVCache) and c.max_size == 32 and c.keep == 4 for c in caches)
    assert all(type(c) is ReusableKVCache for c in BaseCache.make_kv_cache(M()))
    paged = M()
    paged._page_pool = object()
    with pytest.raises(ValueError):
        BaseCache.make_kv_cache(paged, max_kv_size=32)


@pytest.mark.parametrize("off,L", [(0, 6), (5, 3), (16, 4), (40, 9)])
def test_windowed_attention_mask(off, L):
    W = 16
    c = RotatingKVCache(W, keep=4)
    c.offset = off
    m = base.create_attention_mask(torch.zeros((1, L, 8)), [c])
    o = min(W, off)
    i, j = np.arange(L)[:, None], np.arange(o + L)[None]
    visible = (j <= o + i) & (j >= o + i - W)
    assert m.shape == (L, o + L) and np.array_equal((m.float() >= 0).numpy(), visible)
    r = ReusableKVCache()
    r.offset = off
    assert base.create_attention_mask(torch.zeros((1, L, 8)), [r]).shape == (L, off + L)


def test_save_load_round_trip(tmp_path):
    c, ref = _run([20] + [1] * 5, 8, 4, seed=3)
    c2, _ = _run([3], 16, 0, seed=4)
    f = str(tmp_path / "ring.safetensors")
    BaseCache.save_cache(f, [c, c2], {"note": "x"})
    from safetensors import safe_open
    with safe_open(f, framework="pt") as fh:
        meta = fh.metadata()
        assert set(fh.keys()) == {"0.0", "0.1", "1.0", "1.1"}
    assert meta["2.0"] == "RotatingKVCache" and tuple(meta[f"0.0.{k}"] for k in range(5)) == c.meta_state
    loaded, md = BaseCache.load_cache(f, device="cpu")
    assert md == {"note": "x"}
    for a, b in zip(loaded, (c, c2)):
        assert isinstance(a, RotatingKVCache) and a.meta_state == b.meta_state
        assert all(torch.equal(x, y) for x, y in zip(a.state, b.state))
    # and both continue identically
    rng = np.random.default_rng(9)
    for L in (1, 1, 3, 1):
        k, v = _rows(rng, L)
        x = loaded[0].update_and_fetch(_t(k), _t(v))
        y = c.update_and_fetch(_t(k), _t(v))
        assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_prompt_cache_reuses_only_untouched_rings():
    pc = PromptCache(cache=[RotatingKVCache(16, keep=4) for _ in range(2)])
    k = torch.zeros((1, H, 6, D))
    for c in pc.cache:
        c.update_and_fetch(k, k)
    pc.update([1, 2, 3, 4, 5, 6])
    assert pc([1, 2, 3, 9, 9]) == [9, 9] and all(c.offset == 3 for c in pc.cache)
    for c in pc.cache:
        for _ in range(20):
            c.update_and_fetch(k[:, :, :1], k[:, :, :1])
    pc.update([7] * 20)
    old = list(pc.cache)
    todo = pc([1, 2, 3, 5])
    assert todo == [1, 2, 3, 5] and pc.computed_ids == []
    assert all(isinstance(c, RotatingKVCache) and c.offset == 0 and c.max_size == 16 and c.keep == 4 for c in pc.cache)
    assert all(a is not b for a, b in zip(old, pc.cache))


def test_buffers_shrink_back_after_a_long_store():
    """A prompt longer than the window keeps its rows until the next single-row update cuts them; the buffers then shrink to the window's."""
    c, _ = _run([40], 8, 4)
    assert c.capacity == 40
    k = torch.ones((1, H, 1, D))
    c.update_and_fetch(k, k)
    assert c.capacity == 8 and c.state[0].shape[2] == 8
    c.update_and_fetch(torch.ones((1, H, 30, D)), torch.ones((1, H, 30, D)))
    assert c.capacity == 40  # (8 retained + 30) rounded to whole steps
    c.update_and_fetch(k, k)
    assert c.capacity == 8
