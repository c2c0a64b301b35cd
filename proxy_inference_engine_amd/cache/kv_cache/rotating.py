"""RotatingKVCache on HBM-resident torch buffers: a bounded sliding-window KV cache.

Behavioural mirror of cache/kv_cache/rotating.py of the reference.  W = max_size rows hold the `keep` first positions ("attention
sinks", never evicted) and a ring of the W - keep most recent ones.  The buffers [1, n_kv_heads, cap, head_dim] keep the reference's
row order exactly: rows [0, _len) are the reference's `keys` array (its shape[2] is `_len`; `cap` may be larger), `_idx` is its write
index.  The rules, with off = offset before an update of L rows:
  - L == 1: while off < W the row goes to row off.  Then the ring rotates: the write index runs keep, keep + 1, ..., W - 1, keep, ...
    A store longer than W (after a long prompt or a chunk) is first cut to [sinks, newest W - keep] and the row written at `keep`.
  - L >= 2: the rows become the retained window in temporal order (all off rows if off <= W, else the sinks and the newest W - keep),
    followed by the L new rows; query i of the chunk sees row j iff o' + i - W <= j <= o' + i with o' = min(off, W)
    (create_causal_mask(L, o', window_size=W), models/base.py).  On an empty cache all L rows stay until the next single-row update.
  - RoPE always runs at the absolute position off + i.

The decoder writes the new rows itself, so besides `update_and_fetch` the class exposes its halves: `prepare(n)` rearranges the rows
and makes room (the row moves run as HIP kernels, csrc/rotating.hip) and returns where the update goes; `advance(n)` books it.
"""
from __future__ import annotations

import torch

from . import BaseCache


class RotatingKVCache(BaseCache):
    def __init__(self, max_size: int, keep: int = 0, step: int = 256):
        if int(max_size) < 1:
            raise ValueError(f"RotatingKVCache: max_size must be at least 1, got {max_size}")
        if not 0 <= int(keep) < int(max_size):
            raise ValueError(f"RotatingKVCache: keep must be in [0, max_size), got keep={keep}, max_size={max_size}")
        self.keep = int(keep)
        self.max_size = int(max_size)
        self.step = int(step)
        self.keys: torch.Tensor | None = None
        self.values: torch.Tensor | None = None
        self.offset = 0
        self._idx = 0
        self._len = 0          # the reference's keys.shape[2] (rows in use; 0 = no keys yet)
        self._rot0 = self.max_size  # position written at row `keep` when the ring last started rotating (device-side ring rule)

    meta_args = {"max_size": 1, "keep": 0, "step": 2}

    # ------------------------------------------------------------------ buffers
    @property
    def capacity(self) -> int:
        return 0 if self.keys is None else self.keys.shape[2]

    def _round(self, n: int) -> int:
        return ((n + self.step - 1) // self.step) * self.step

    def _ensure(self, rows: int, n_kv_heads: int = 0, head_dim: int = 0, dtype: torch.dtype | None = None, device=None) -> None:
        """Room for `rows` rows (whole steps), the rows held so far kept.  Buffers a long store left larger than both `rows` and the
        window shrink back (the reference's arrays shrink when it cuts them): only the window stays allocated between updates."""
        bound = self._round(max(rows, self.max_size))
        if self.keys is not None and rows <= self.keys.shape[2] <= bound:
            return
        cap = self._round(rows) if self.keys is None or self.keys.shape[2] < rows else bound
        if self.keys is not None:
            n_kv_heads, head_dim, dtype, device = self.keys.shape[1], self.keys.shape[3], self.keys.dtype, self.keys.device
        k = torch.zeros((1, n_kv_heads, cap, head_dim), dtype=dtype, device=device)
        v = torch.zeros_like(k)
        if self.keys is not None:
            n = min(self.keys.shape[2], cap)
            k[..., :n, :] = self.keys[..., :n, :]
            v[..., :n, :] = self.values[..., :n, :]
        self.keys, self.values = k, v

    def _move(self, n: int, shift: int, n_dst: int) -> None:
        """rows keep + j <- rows keep + (j + shift) % n for j < n_dst (one gather per buffer)."""
        if n_dst <= 0 or shift % n == 0:
            return
        if self.keys.is_cuda:
            from ... import hip_ops
            hip_ops.kv_ring_order(self.keys, self.values, self.keep, n, shift, n_dst)
            return
        idx = self.keep + (torch.arange(n_dst, device=self.keys.device) + shift) % n
        for t in (self.keys, self.values):
            t[..., self.keep:self.keep + n_dst, :] = t[..., idx, :].clone()

    def _trim_rows(self, trim: int) -> None:
        """rotating.py's _trim on the stored rows: [:keep] + [trim + keep:]."""
        if trim > 0:
            self._move(self._len - self.keep, trim, self._len - self.keep - trim)
            self._len -= trim

    def _temporal_order(self) -> None:
        if self._idx == self._len:
            return
        if self._idx < self.offset:  # a rotated ring: [sinks, rows from the write index on, rows before it]
            self._move(self._len - self.keep, self._idx - self.keep, self._len - self.keep)
        else:
            self._len = self._idx

    # ------------------------------------------------------------------ the two halves of update_and_fetch
    def prepare(self, n: int, n_kv_heads: int, head_dim: int, dtype: torch.dtype, device) -> int:
        """Everything of update_and_fetch for `n` new rows except writing them: returns the buffer row the first one goes to."""
        if n < 1:
            raise ValueError("RotatingKVCache: an update needs at least one row")
        if n == 1:
            prev = self.offset
            if self._len == 0 or (prev >= self._len and self._len < self.max_size):
                self._len += min(self.step, self.max_size - prev)
                self._ensure(self._len, n_kv_heads, head_dim, dtype, device)
                self._idx = prev
            trim = self._len - self.max_size
            if trim > 0:
                self._trim_rows(trim)
                self._ensure(self._len)  # the long store's rows are gone: back to the window's buffers
                self._idx = self.max_size
            if self._idx == self.max_size:
                self._idx = self.keep
            if self._idx != self.offset:  # rotating: keep the device's rule (row of position p >= rot0) in step with the write index
                span = self.max_size - self.keep
                if self._rot0 > self.offset or (self.offset - self._rot0) % span != self._idx - self.keep:
                    self._rot0 = self.offset - (self._idx - self.keep)
            else:  # not rotating yet: position p is row p
                self._rot0 = self.max_size
            return self._idx
        if self._len:
            old_idx = self._idx
            self._temporal_order()
            self._trim_rows(old_idx - self.max_size)
        self._ensure(self._len + n, n_kv_heads, head_dim, dtype, device)
        row0 = self._len
        self._len += n
        self._idx = row0
        return row0

    def reserve(self, needed: int, n_kv_heads: int, head_dim: int, dtype: torch.dtype, device, batch: int = 1) -> int:
        if batch != 1:
            raise ValueError("RotatingKVCache: batch 1 only")
        return self.prepare(needed, n_kv_heads, head_dim, dtype, device)

    def advance(self, n: int) -> None:
        self.offset += n
        self._idx += n

    def update_and_fetch(self, keys: torch.Tensor, values: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """keys / values [1, n_kv, L, D] -> the keys / values the new rows attend (rotating.py's return values)."""
        L = keys.shape[2]
        row = self.prepare(L, keys.shape[1], keys.shape[3], keys.dtype, keys.device)
        self.keys[..., row:row + L, :] = keys
        self.values[..., row:row + L, :] = values
        self.advance(L)
        n = self.offset if L == 1 and self.offset < self.max_size else self._len
        return self.keys[..., :n, :], self.values[..., :n, :]

    # ------------------------------------------------------------------ reference protocol
    @property
    def state(self):
        if self.keys is None:
            return None, None
        n = self.offset if self.offset < self._len else self._len
        return self.keys[..., :n, :], self.values[..., :n, :]

    @state.setter
    def state(self, v):
        k, vv = v
        if k is None:
            self.keys = self.values = None
            self._len = 0
            return
        self.keys, self.values = k.contiguous(), vv.contiguous()
        self._len = k.shape[2]

    @property
    def meta_state(self):
        return tuple(map(str, (self.keep, self.max_size, self.step, self.offset, self._idx)))

    @meta_state.setter
    def meta_state(self, v):
        self.keep, self.max_size, self.step, self.offset, self._idx = map(int, v)
        # the device-side ring rule: a rotated ring (write index behind the offset) continues from the stored write index
        self._rot0 = self.max_size if self._idx >= self.offset else self.offset - (self._idx - self.keep)

    def is_trimmable(self) -> bool:
        return self.keys is not None and self.offset < self.max_size

    def trim(self, n: int) -> int:
        n = min(self.offset, n)
        self.offset -= n
        self._idx -= n
        return n

    def to_quantized(self, group_size: int = 64, bits: int = 4) -> BaseCache:
        return self  # as in the reference: a rotating cache stays 16-bit

    def reuse(self, new_prompt_length: int, common_prefix_length: int) -> None:
        """PromptCache prefix reuse (prompt_cache.py): only while nothing has been evicted (is_trimmable); the prompt cache starts
        fresh rotating caches otherwise."""
        if not self.is_trimmable():
            raise ValueError("RotatingKVCache: prefix reuse needs a ring that has not evicted anything (is_trimmable())")
        self.trim(self.offset - common_prefix_length)
