"""QuantizedKVCache on HBM-resident torch buffers.

Behavioural mirror of cache/kv_cache/quantized.py:7-196 of the reference: per layer, keys and values are each a triple
(codes uint32 [B, n_kv_heads, capacity, head_dim*bits/32], scales T [B, n_kv_heads, capacity, head_dim/group_size],
biases T [same]) -- mx.quantize's output for every cached row.  Capacity is allocated and grown in whole `step`s (256): a
request for n more positions adds ceil(n/step)*step rows, after first cutting the buffers to `offset` when that is not a
multiple of `step` (quantized.py:53-80) -- not the 1.5x growth of ReusableKVCache.

As with ReusableKVCache the decode kernels write the new rows themselves (the attention launch quantises the row the q|k|v
launch staged), so `update_and_fetch` is also available as its two halves `reserve(n)` / `advance(n)`.  Formats: bits 4 / 8,
group_size 32 / 64 / 128 dividing head_dim (64 / 128), T bf16 / f16; anything else raises ValueError.
"""
from __future__ import annotations

import torch

from . import BaseCache

BITS = (4, 8)
GROUP_SIZES = (32, 64, 128)


def check_format(group_size: int, bits: int, head_dim: int | None = None, dtype: torch.dtype | None = None) -> None:
    """The formats the kernels take (bits 2 / 3 / 6, which mx.quantize accepts, are excluded like in the reference's docstring)."""
    if bits not in BITS:
        raise ValueError(f"QuantizedKVCache: bits must be 4 or 8, got {bits}")
    if group_size not in GROUP_SIZES:
        raise ValueError(f"QuantizedKVCache: group_size must be 32, 64 or 128, got {group_size}")
    if head_dim is not None:
        if head_dim not in (64, 128):
            raise ValueError(f"QuantizedKVCache: head_dim must be 64 or 128, got {head_dim}")
        if head_dim % group_size:
            raise ValueError(f"QuantizedKVCache: group_size {group_size} does not divide head_dim {head_dim}")
    if dtype is not None and dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"QuantizedKVCache: the activation dtype must be bfloat16 or float16, got {dtype}")


class QuantizedKVCache(BaseCache):
    def __init__(self, group_size: int = 64, bits: int = 8):
        check_format(group_size, bits)
        self.keys: tuple[torch.Tensor, torch.Tensor, torch.Tensor] | None = None
        self.values: tuple[torch.Tensor, torch.Tensor, torch.Tensor] | None = None
        self.offset = 0
        self.step = 256
        self.group_size = group_size
        self.bits = bits

    # ------------------------------------------------------------------ capacity
    @property
    def capacity(self) -> int:
        return 0 if self.keys is None else self.keys[0].shape[2]

    def _init_quant(self, shape: tuple[int, int, int], dim: int, dtype: torch.dtype, device) -> tuple[torch.Tensor, ...]:
        el_per_int = 32 // self.bits
        return (torch.zeros((*shape, dim // el_per_int), dtype=torch.uint32, device=device),
                torch.zeros((*shape, dim // self.group_size), dtype=dtype, device=device),
                torch.zeros((*shape, dim // self.group_size), dtype=dtype, device=device))

    def reserve(self, needed: int, n_kv_heads: int, head_dim: int, dtype: torch.dtype, device, batch: int = 1) -> None:
        """Capacity half of update_and_fetch (quantized.py:53-80): room for `needed` more positions."""
        prev = self.offset
        if self.keys is not None and prev + needed <= self.keys[0].shape[-2]:
            return
        check_format(self.group_size, self.bits, head_dim, dtype)
        new_steps = (self.step + needed - 1) // self.step * self.step
        if self.keys is None:
            shape = (batch, n_kv_heads, new_steps)
            self.keys = self._init_quant(shape, head_dim, dtype, device)
            self.values = self._init_quant(shape, head_dim, dtype, device)
            return
        if prev % self.step != 0:
            self.keys = tuple(x[..., :prev, :] for x in self.keys)
            self.values = tuple(x[..., :prev, :] for x in self.values)

        def expand(x: torch.Tensor) -> torch.Tensor:
            B, H = x.shape[0], x.shape[1]
            return torch.cat([x, torch.zeros((B, H, new_steps, x.shape[-1]), dtype=x.dtype, device=x.device)], dim=-2)

        self.keys = tuple(expand(x) for x in self.keys)
        self.values = tuple(expand(x) for x in self.values)

    def advance(self, n: int) -> None:
        self.offset += n

    def reuse(self, new_prompt_length: int, common_prefix_length: int) -> None:
        """PromptCache prefix reuse (prompt_cache.py:52-76): keep the common prefix; the prompt's remaining rows are appended by
        the next model call, which grows the buffers the reference's way."""
        if self.keys is None or self.values is None:
            return
        self.offset = common_prefix_length

    # ------------------------------------------------------------------ reference protocol
    def update_and_fetch(self, keys: torch.Tensor, values: torch.Tensor):
        """keys / values [B, n_kv, L, D] T -> the quantized triples of the first offset+L positions (quantized.py:37-103)."""
        from ... import hip_ops
        B, n_kv, L, D = keys.shape
        prev = self.offset
        self.reserve(L, n_kv, D, keys.dtype, keys.device, B)
        for src, dst in ((keys, self.keys), (values, self.values)):
            codes, scales, biases = hip_ops.kv_quantize(src, self.group_size, self.bits)
            dst[0][..., prev:prev + L, :] = codes
            dst[1][..., prev:prev + L, :] = scales
            dst[2][..., prev:prev + L, :] = biases
        self.offset += L
        return (tuple(x[..., :self.offset, :] for x in self.keys), tuple(x[..., :self.offset, :] for x in self.values))

    @property
    def state(self):
        if self.keys is None:
            return None, None
        if self.offset == self.keys[0].shape[2]:
            return self.keys, self.values
        return tuple(x[..., :self.offset, :] for x in self.keys), tuple(x[..., :self.offset, :] for x in self.values)

    @state.setter
    def state(self, v):
        self.keys, self.values = v
        if self.keys is not None:
            self.keys = tuple(self.keys)
            self.values = tuple(self.values)
            self.offset = self.keys[0].shape[-2]

    @property
    def meta_state(self):
        return tuple(map(str, (self.step, self.offset, self.group_size, self.bits)))

    @meta_state.setter
    def meta_state(self, v):
        step, offset, group_size, bits = map(int, v)
        check_format(group_size, bits)
        self.step, self.offset, self.group_size, self.bits = step, offset, group_size, bits

    def is_trimmable(self) -> bool:
        return True

    def trim(self, n: int) -> int:
        n = min(self.offset, n)
        self.offset -= n
        return n

    def to_quantized(self, group_size: int = 64, bits: int = 4) -> "QuantizedKVCache":
        return self  # quantized.py:185-196

    @classmethod
    def from_cache(cls, cache, group_size: int = 64, bits: int = 4) -> "QuantizedKVCache":
        """KVCache.to_quantized of the reference (cache/kv_cache/cache.py:127-148) for a ReusableKVCache: the same capacity and
        offset, its first `offset` rows quantised on the device (pie_kv_quantize)."""
        from ... import hip_ops
        from .reusable import ReusableKVCache
        if isinstance(cache, cls):
            return cache
        if not isinstance(cache, ReusableKVCache):
            raise TypeError(f"QuantizedKVCache.from_cache: expected a ReusableKVCache, got {type(cache).__name__}")
        q = cls(group_size=group_size, bits=bits)
        q.offset = cache.offset
        if cache.keys is None or cache.values is None:
            return q
        B, H, cap, D = cache.keys.shape
        check_format(group_size, bits, D, cache.keys.dtype)
        q.keys = q._init_quant((B, H, cap), D, cache.keys.dtype, cache.keys.device)
        q.values = q._init_quant((B, H, cap), D, cache.keys.dtype, cache.keys.device)
        for src, dst in ((cache.keys, q.keys), (cache.values, q.values)):
            hip_ops.kv_quantize_rows(src, cache.offset, *dst, group_size=group_size, bits=bits)
        return q
