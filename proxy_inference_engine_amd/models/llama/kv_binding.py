"""What the native decoder (csrc/decoder.hip) is pointed at: one binding for every KV cache kind.  `KVBinding.sync(cache, n_new)` makes
the decoder's device-side view (buffers, capacity, offset) match the Python cache objects before a model call, `advance(cache, n)`
books the rows after it.  One driver does what every kind shares; a kind is one row of `_KINDS`: the function that checks every layer
and names the buffers in a key that starts with the kind (a cache of another kind over the same addresses is bound again), and the
function that issues its `pie_decoder_set_*` call.  Nothing here needs a GPU: library, decoder handle and stream are arguments."""
from __future__ import annotations

import ctypes as C
from operator import attrgetter

import torch

from ... import _ffi
from ...cache.kv_cache import PagedKVCache, QuantizedKVCache, ReusableKVCache, RotatingKVCache


def on_int8_pages(cache) -> bool:
    """A cache on the reference KVPage's own storage (int8 rows): its single-sequence prompt pass is not available."""
    return isinstance(cache[0], PagedKVCache) and cache[0].page_manager.allocator.dtype == torch.int8


_CAPACITY = attrgetter("capacity")


def _room(b: "KVBinding", cache, n_new: int) -> int:
    """The host half of cache.update_and_fetch for every layer (reusable.py:113-131); the capacity all layers have."""
    n_kv_heads, head_dim, dtype, device = b.geometry
    for c in cache:
        c.reserve(n_new, n_kv_heads, head_dim, dtype, device)
    return min(map(_CAPACITY, cache))


# ------------------------------------------------------------------ the kinds: (b, cache, n_new) -> key, checked before anything is allocated
def _plain(b, cache, n_new):
    off = cache[0].offset
    for c in cache:
        if not isinstance(c, ReusableKVCache):
            raise TypeError("the decode path runs on ReusableKVCache (prompt_cache.py:73)")
        if c.offset != off:
            raise ValueError("layer caches disagree on offset")
    cap = _room(b, cache, n_new)
    return ("plain", tuple(c.keys.data_ptr() for c in cache), tuple(c.values.data_ptr() for c in cache), cap)


def _ring(b, cache, n_new):  # making room also rearranges every layer's rows for the update (rotating.py: HIP row moves, outside any captured graph)
    c0 = cache[0]
    for c in cache:
        if not isinstance(c, RotatingKVCache):
            raise TypeError("all layers of a rotating cache must be RotatingKVCache")
        if (c.offset, c.max_size, c.keep, c._idx, c._len) != (c0.offset, c0.max_size, c0.keep, c0._idx, c0._len):
            raise ValueError("layer caches disagree on offset or ring geometry")
    if b.tensor_parallel:
        raise ValueError("a rotating KV cache is not available on a tensor-parallel model")
    if c0.keys is not None and (c0.keys.dtype, c0.keys.device) != b.geometry[2:]:
        raise ValueError("the rotating cache's buffers are not in the model's dtype / device")
    cap = _room(b, cache, n_new)
    return ("ring", tuple(c.keys.data_ptr() for c in cache), tuple(c.values.data_ptr() for c in cache), cap)


def _quant(b, cache, n_new):  # the key carries the format, so a captured step graph is re-captured when it changes
    c0 = cache[0]
    for c in cache:
        if not isinstance(c, QuantizedKVCache):
            raise TypeError("all layers of a quantized cache must be QuantizedKVCache")
        if c.offset != c0.offset or c.group_size != c0.group_size or c.bits != c0.bits:
            raise ValueError("layer caches disagree on offset or format")
    cap = _room(b, cache, n_new)
    return ("quant", tuple(tuple(t.data_ptr() for t in (*c.keys, *c.values)) for c in cache), cap, c0.group_size, c0.bits)


def _paged(b, cache, n_new):  # (int8 pages: the step's new K / V row is quantised into the sequence's page, attention reads the codes back)
    seq = cache[0].page_manager
    for c in cache:
        if not isinstance(c, PagedKVCache) or c.page_manager is not seq:
            raise TypeError("the layers of a paged cache must share one PagedSequence")
    _room(b, cache, n_new)
    a = seq.allocator
    b.match_page_format(a)
    return ("paged", a.slab.data_ptr(), a.size(), seq.table.data_ptr(), seq.max_blocks, a.dtype == torch.int8)


# ------------------------------------------------------------------ their pie_decoder_set_* calls: (b, cache, key)
def _bind_kv(b, cache, key):
    n = len(cache)
    _ffi.check(b.lib.pie_decoder_set_kv(b.dec, (C.c_void_p * n)(*key[1]), (C.c_void_p * n)(*key[2]), key[3], b.stream()))


def _bind_quant(b, cache, key):
    n = len(cache)
    cols = [(C.c_void_p * n)(*[p[j] for p in key[1]]) for j in range(6)]
    _ffi.check(b.lib.pie_decoder_set_kv_quant(b.dec, *cols, *key[2:], b.stream()))


def _bind_paged(b, cache, key):
    seq = cache[0].page_manager
    slabs, n_pages, _ = b.pool_args(seq.allocator)
    _ffi.check(b.lib.pie_decoder_set_paged_kv(b.dec, slabs, n_pages, _ffi.p(seq.table), seq.max_blocks, b.stream()))
    b._hold = (seq.allocator, seq.table)  # keeps the slab and the table alive while the decoder points at them


def _ring_rule(b, c0, n_new):
    """The ring's second-level binding: its window and sink rows, the row rule of the steps (`_rot0`), the buffer row a prompt pass
    appends at, and the bound the steps' positions stay below (the staging table covers them: grown in 64k steps)."""
    rule = (c0.max_size, c0.keep, c0._rot0, c0._idx if n_new > 1 else 0, ((c0.offset + n_new) // 65536 + 1) * 65536)
    if rule != b._ring:
        _ffi.check(b.lib.pie_decoder_set_kv_ring(b.dec, *rule, b.stream()))
        b._ring = rule


# the single dispatch point, in this order: (class of cache[0], key, bind, what follows the bind on every sync)
_KINDS = ((PagedKVCache, _paged, _bind_paged, None), (QuantizedKVCache, _quant, _bind_quant, None),
          (RotatingKVCache, _ring, _bind_kv, _ring_rule), (ReusableKVCache, _plain, _bind_kv, None))


class KVBinding:
    def __init__(self, lib, dec, n_layers: int, n_kv_heads: int, head_dim: int, dtype: torch.dtype, device, tensor_parallel: bool = False,
                 stream=_ffi.stream):
        self.lib, self.dec, self.stream, self.n_layers, self.tensor_parallel = lib, dec, stream, n_layers, tensor_parallel
        self.geometry = (n_kv_heads, head_dim, dtype, torch.device(device))  # what a cache's reserve() takes
        self._key = None     # (kind, buffer addresses, capacity, ...) currently in the decoder's device table
        self._ring = None    # (window, keep, rot0, row0, positions) of the bound rotating cache; None under every other binding
        self._hold = None
        self.offset = None   # device-side cache offset the decoder believes in: after advance(), the position the chosen token will occupy
        self._i8 = None      # the decoder's page format (PIE_OPT_KV_I8); None until a pool was seen

    def sync(self, cache, n_new: int) -> None:
        """Room for `n_new` more rows in every layer, then the decoder bound to them; all layers are checked before the first allocation."""
        if len(cache) != self.n_layers:
            raise ValueError(f"expected {self.n_layers} layer caches, got {len(cache)}")
        c0 = cache[0]
        for cls, key_of, bind, then in _KINDS:  # (what is none of them is left to the last row, which refuses it)
            if isinstance(c0, cls):
                break
        key = key_of(self, cache, n_new)
        if key != self._key:
            bind(self, cache, key)
            self._key, self._ring = key, None
        if then is not None:
            then(self, c0, n_new)
        if self.offset != c0.offset:
            _ffi.check(self.lib.pie_decoder_set_state(self.dec, c0.offset, -1, self.stream()))
            self.offset = c0.offset

    def advance(self, cache, n: int) -> None:
        for c in cache:
            c.advance(n)  # reusable.py:139
        self.offset += n

    def invalidate(self) -> None:
        """Forget the binding and the device-side offset (something else re-pointed the decoder): the next sync binds again."""
        self._key = self._ring = self.offset = None

    # ------------------------------------------------------------------ page pools
    def match_page_format(self, allocator, always: bool = False) -> None:
        """The decoder indexes the slabs with the page stride of ITS page format (PIE_OPT_KV_I8); a pool handed to make_cache(allocator=...)
        may be of the other one.  Every entry point therefore follows the pool it is given (and the C ABI checks the slab size)."""
        if always or self._i8 != (allocator.dtype == torch.int8):
            self._i8 = allocator.dtype == torch.int8
            _ffi.check(self.lib.pie_decoder_configure(self.dec, _ffi.PIE_OPT_KV_I8, int(self._i8)))

    def pool_args(self, allocator):
        """(per-layer slab planes, pages, bytes of one plane) as the paged entry points take them, the decoder set to the pool's format."""
        self.match_page_format(allocator)
        slabs = (C.c_void_p * self.n_layers)(*[allocator.slab[i].data_ptr() for i in range(self.n_layers)])
        return slabs, allocator.size(), allocator.slab[0].numel() * allocator.slab.element_size()

    def sequences(self, who: str, caches) -> list:
        """The PagedSequences behind `caches`: paged caches of distinct sequences of one pool, or `who` refuses them."""
        for c in caches:
            if len(c) != self.n_layers or not isinstance(c[0], PagedKVCache):
                raise TypeError(f"{who} runs on paged caches (enable_paged_kv(), then make_cache())")
        seqs = [c[0].page_manager for c in caches]
        if not seqs:
            raise ValueError(f"{who}: an empty batch")
        if any(s.allocator is not seqs[0].allocator for s in seqs) or len({id(s) for s in seqs}) != len(seqs):
            raise ValueError(f"{who}: distinct sequences of one page pool")
        return seqs
