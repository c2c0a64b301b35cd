"""The rules by which the decoder is pointed at a KV cache (models/llama/kv_binding.py), on the CPU: a stand-in library records
every pie_decoder_* call the binding makes, the caches are the real ones over CPU tensors (paged: the native page pool with a CPU slab)."""
import pytest
import torch

from proxy_inference_engine_amd import _ffi
from proxy_inference_engine_amd.cache.kv_cache import PageAllocator, PagedKVCache, PagedSequence, QuantizedKVCache, ReusableKVCache, RotatingKVCache
from proxy_inference_engine_amd.models.llama.kv_binding import KVBinding, on_int8_pages

N, H, D, DT = 3, 2, 64, torch.bfloat16
PAGES = 12
I8 = _ffi.PIE_OPT_KV_I8


class Lib:
    """pie_decoder_<name>(...) -> 0, logged as (name, *integer arguments): handles, pointer arrays and the stream are left out."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        if not name.startswith("pie_decoder_"):
            raise AttributeError(name)

        def call(*args):
            self.log.append((name[len("pie_decoder_"):], *[a for a in args if type(a) is int]))
            return 0
        return call

    def take(self):
        log, self.log = self.log, []
        return log


def binding(tensor_parallel=False):
    lib = Lib()
    return KVBinding(lib, object(), N, H, D, DT, "cpu", tensor_parallel=tensor_parallel, stream=lambda: None), lib


def paged(pool, max_blocks=2):
    seq = PagedSequence(pool, max_blocks)
    return [PagedKVCache(seq, i) for i in range(N)]


@pytest.fixture
def pool():
    return PageAllocator(PAGES, H, D, dtype=DT, device="cpu", num_layers=N)


def make(kind, pool):
    return {"plain": lambda: [ReusableKVCache() for _ in range(N)],
            "quant": lambda: [QuantizedKVCache(group_size=64, bits=8) for _ in range(N)],
            "ring": lambda: [RotatingKVCache(16, keep=4) for _ in range(N)],
            "paged": lambda: paged(pool)}[kind]()


# the bind calls of a fresh cache of each kind given a 5-row prompt
FIRST = {"plain": [("set_kv", 256)],
         "quant": [("set_kv_quant", 256, 64, 8)],
         "ring": [("set_kv", 256), ("set_kv_ring", 16, 4, 16, 0, 65536)],
         "paged": [("configure", I8, 0), ("set_paged_kv", PAGES, 2)]}
KINDS = list(FIRST)


def unallocated(cache, pool):
    return all(getattr(c, "keys", None) is None for c in cache) and pool.get_num_free_pages() == PAGES


@pytest.mark.parametrize("kind", KINDS)
def test_first_use_binds_then_sets_the_state_and_an_unchanged_cache_costs_no_call(kind, pool):
    b, lib = binding()
    cache = make(kind, pool)
    b.sync(cache, 5)
    assert lib.take() == FIRST[kind] + [("set_state", 0, -1)]
    b.advance(cache, 5)
    assert b.offset == 5 and all(c.offset == 5 for c in cache)
    for i in range(4):
        b.sync(cache, 1)
        b.advance(cache, 1)
    assert lib.take() == [] and b.offset == 9 and cache[-1].offset == 9


@pytest.mark.parametrize("kind", KINDS)
def test_invalidate_makes_the_next_sync_bind_and_set_the_state(kind, pool):
    b, lib = binding()
    cache = make(kind, pool)
    b.sync(cache, 5), b.advance(cache, 5), lib.take()
    b.invalidate()
    assert b.offset is None
    b.sync(cache, 1)
    assert lib.take() == [c for c in FIRST[kind] if c[0] != "configure"] + [("set_state", 5, -1)]  # (the page format is the decoder's, not the binding's)


@pytest.mark.parametrize("kind, rows, rebind", [("plain", 256, ("set_kv", 512)), ("quant", 256, ("set_kv_quant", 512, 64, 8)),
                                                ("paged", 128, ("set_paged_kv", PAGES, 4))])
def test_growth_past_the_capacity_binds_once_with_the_new_capacity(kind, rows, rebind, pool):
    b, lib = binding()
    cache = make(kind, pool)
    b.sync(cache, rows), b.advance(cache, rows), lib.take()
    assert cache[0].capacity == rows
    b.sync(cache, 1)  # plain / quantized: the 257th row; paged: a third block in a table of two
    assert lib.take() == [rebind]
    b.advance(cache, 1), b.sync(cache, 1)
    assert lib.take() == []


@pytest.mark.parametrize("kind", KINDS)
def test_trim_and_reuse_on_the_host_set_the_state_without_a_bind(kind, pool):
    b, lib = binding()
    cache = make(kind, pool)
    b.sync(cache, 10), b.advance(cache, 10), lib.take()
    assert all(c.trim(3) == 3 for c in cache)
    b.sync(cache, 1)
    assert lib.take() == [("set_state", 7, -1)]
    b.advance(cache, 1)
    for c in cache:
        c.reuse(12, 4)  # PromptCache: a 12-token prompt that shares 4 tokens with the cached one
    b.sync(cache, 1)
    assert lib.take() == [("set_state", 4, -1)] and cache[0].offset == 4


def test_a_small_ring_is_bound_once_and_its_rule_follows_rot0_the_prompt_row_and_the_position_bucket():
    b, lib = binding()
    cache = make("ring", None)
    b.sync(cache, 5), b.advance(cache, 5)
    assert lib.take() == FIRST["ring"] + [("set_state", 0, -1)]
    for _ in range(30):  # fills at 16, then rotates: row of position p is 4 + (p - 16) % 12, which is the rule bound first
        b.sync(cache, 1), b.advance(cache, 1)
    assert lib.take() == [] and cache[0].offset == 35 and cache[0].capacity == 256
    b.sync(cache, 3)  # a chunk behind a rotated ring: the rows in temporal order, the chunk appended at row 16
    assert lib.take() == [("set_kv_ring", 16, 4, 16, 16, 65536)]
    b.advance(cache, 3)
    b.sync(cache, 1)  # 19 rows are cut to the window, the ring restarts at row `keep` with position 38
    assert lib.take() == [("set_kv_ring", 16, 4, 38, 0, 65536)]
    b.advance(cache, 1)
    for c in cache:  # 5462 turns of the 12-row ring later: the same write index, the next 64k bucket of positions
        c.offset += 5462 * 12
    b.sync(cache, 1)
    assert lib.take() == [("set_kv_ring", 16, 4, 38, 0, 131072), ("set_state", 39 + 65544, -1)]


def test_a_ring_whose_buffers_grow_while_it_fills_is_bound_again_with_its_rule():
    b, lib = binding()
    cache = [RotatingKVCache(600, keep=4) for _ in range(N)]
    b.sync(cache, 5), b.advance(cache, 5)
    assert lib.take() == [("set_kv", 256), ("set_kv_ring", 600, 4, 600, 0, 65536), ("set_state", 0, -1)]
    b.sync(cache, 1)  # the first single row makes room for a whole step of them: 5 + 256 rows
    assert lib.take() == [("set_kv", 512), ("set_kv_ring", 600, 4, 600, 0, 65536)]
    b.advance(cache, 1), b.sync(cache, 1)
    assert lib.take() == []


def test_a_change_of_kind_over_the_same_buffers_is_bound_both_ways():
    """Rings dropped and plain caches allocated next may get the same addresses back from the allocator: the key carries the kind, so
    the decoder leaves ring mode (only the pie_decoder_set_* entry points do that) and enters it again."""
    b, lib = binding()
    ring = make("ring", None)
    b.sync(ring, 5), b.advance(ring, 5), lib.take()
    plain = [ReusableKVCache() for _ in range(N)]
    for p, r in zip(plain, ring):
        p.keys, p.values, p.offset = r.keys, r.values, r.offset
    b.sync(plain, 1)
    assert lib.take() == [("set_kv", 256)]
    assert [p.keys.data_ptr() for p in plain] == [r.keys.data_ptr() for r in ring]
    b.sync(ring, 1)
    assert lib.take() == [("set_kv", 256), ("set_kv_ring", 16, 4, 16, 0, 65536)]
    b.sync(ring, 1)
    assert lib.take() == []


@pytest.mark.parametrize("first", KINDS)
@pytest.mark.parametrize("other", KINDS)
def test_layers_of_two_kinds_are_refused_before_anything_is_allocated(first, other, pool):
    if first == other:
        return
    b, lib = binding()
    cache = make(first, pool)
    cache[-1] = make(other, pool)[-1]
    with pytest.raises(TypeError):
        b.sync(cache, 5)
    assert lib.take() == [] and unallocated(cache, pool) and b.offset is None


def test_layers_that_disagree_and_wrong_layer_counts_are_refused_before_anything_is_allocated(pool):
    def plain():
        cache = make("plain", pool)
        cache[-1].offset = 1
        return cache

    def fmt():
        cache = make("quant", pool)
        cache[-1] = QuantizedKVCache(group_size=64, bits=4)
        return cache

    def geometry():
        cache = make("ring", pool)
        cache[-1] = RotatingKVCache(16, keep=2)
        return cache

    for bad in (plain, fmt, geometry):
        b, lib = binding()
        cache = bad()
        with pytest.raises(ValueError, match="disagree"):
            b.sync(cache, 5)
        assert lib.take() == [] and unallocated(cache, pool)
    for kind in KINDS:
        b, lib = binding()
        cache = make(kind, pool)[:-1]
        with pytest.raises(ValueError, match="expected 3 layer caches"):
            b.sync(cache, 5)
        assert lib.take() == [] and unallocated(cache, pool)
    b, lib = binding(tensor_parallel=True)
    cache = make("ring", pool)
    with pytest.raises(ValueError, match="tensor-parallel"):
        b.sync(cache, 5)
    assert lib.take() == [] and unallocated(cache, pool)
    b.sync(make("plain", pool), 5)  # every other kind runs on a tensor-parallel binding
    assert lib.take() == FIRST["plain"] + [("set_state", 0, -1)]
    b, lib = binding()
    cache = paged(pool)
    cache[-1] = paged(pool)[-1]  # a layer of another sequence
    with pytest.raises(TypeError):
        b.sync(cache, 5)
    assert lib.take() == [] and unallocated(cache, pool)


def test_the_batch_entry_points_share_one_check_and_one_description_of_the_pool(pool):
    b, lib = binding()
    one, two = paged(pool), paged(pool)
    assert b.sequences("step_batch", [one, two]) == [one[0].page_manager, two[0].page_manager]
    with pytest.raises(ValueError, match="step_mixed: distinct"):
        b.sequences("step_mixed", [one, one])
    with pytest.raises(ValueError, match="distinct"):
        b.sequences("step_batch", [one, paged(PageAllocator(2, H, D, dtype=DT, device="cpu", num_layers=N))])
    with pytest.raises(ValueError, match="empty"):
        b.sequences("prefill_batch", [])
    for bad in (make("plain", pool), one[:-1]):
        with pytest.raises(TypeError, match="prefill_batch runs on paged caches"):
            b.sequences("prefill_batch", [two, bad])
    slabs, n_pages, plane = b.pool_args(pool)
    assert (len(slabs), n_pages, plane) == (N, PAGES, pool.slab[0].numel()) and slabs[1] == pool.slab[1].data_ptr()
    assert lib.take() == [("configure", I8, 0)]
    b.pool_args(pool)
    assert lib.take() == [] and not on_int8_pages(one) and not on_int8_pages(make("plain", pool))
