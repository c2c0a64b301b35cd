"""CPU: QuantizedKVCache's host half (growth, trim, state, persistence) against the reference's arithmetic
(cache/kv_cache/quantized.py:37-196, cache/kv_cache/__init__.py:163-210), and the 16-bit cache's save files unchanged."""
import pytest
import torch

from proxy_inference_engine.cache import BaseCache, PromptCache, QuantizedKVCache, ReusableKVCache

H, D = 2, 64


def ref_growth(cap: int, prev: int, n: int, step: int = 256) -> int:
    """Capacity after update_and_fetch of n rows at offset prev (quantized.py:53-80)."""
    if cap and prev + n <= cap:
        return cap
    new = (step + n - 1) // step * step
    if not cap:
        return new
    return (prev if prev % step else cap) + new


def test_growth_follows_the_reference():
    c = QuantizedKVCache(group_size=64, bits=4)
    cap = 0
    for n in (1, 300, 7, 1, 250, 600, 1, 256):
        c.reserve(n, H, D, torch.bfloat16, "cpu")
        cap = ref_growth(cap, c.offset, n)
        assert c.capacity == cap, (n, c.offset)
        c.advance(n)
    assert c.keys[0].dtype == torch.uint32 and c.keys[0].shape == (1, H, cap, D * 4 // 32)
    assert c.keys[1].shape == c.keys[2].shape == c.values[1].shape == (1, H, cap, D // 64)
    assert c.values[0].shape == (1, H, cap, D * 4 // 32) and c.keys[1].dtype == torch.bfloat16
    # 520 then 300 positions: the buffers are cut to the offset (520) before 512 rows are added -- not the 1.5x of ReusableKVCache
    c = QuantizedKVCache(bits=8)
    c.reserve(520, H, D, torch.float16, "cpu"), c.advance(520)
    assert c.capacity == 768
    c.reserve(300, H, D, torch.float16, "cpu")
    assert c.capacity == 520 + 512 and c.keys[0].shape[-1] == D * 8 // 32


def test_state_meta_trim_and_to_quantized():
    c = QuantizedKVCache(group_size=32, bits=8)
    assert c.state == (None, None) and c.meta_state == ("256", "0", "32", "8") and c.is_trimmable()
    c.reserve(10, H, D, torch.bfloat16, "cpu"), c.advance(10)
    k, v = c.state
    assert all(t.shape[2] == 10 for t in (*k, *v))
    c.reserve(246, H, D, torch.bfloat16, "cpu"), c.advance(246)
    assert c.state[0][0] is c.keys[0]  # offset == capacity: the buffers themselves
    assert c.trim(300) == 256 and c.offset == 0
    assert c.to_quantized(64, 4) is c
    c.meta_state = ("256", "7", "128", "4")
    assert (c.step, c.offset, c.group_size, c.bits) == (256, 7, 128, 4)
    r = ReusableKVCache()
    assert r.to_quantized() is r  # unchanged (reusable.py:250-254)


@pytest.mark.parametrize("bits,gs", [(2, 64), (3, 64), (6, 64), (5, 64), (4, 16), (8, 256)])
def test_unsupported_formats_raise(bits, gs):
    with pytest.raises(ValueError):
        QuantizedKVCache(group_size=gs, bits=bits)


def test_unsupported_head_dim_or_dtype_raise():
    with pytest.raises(ValueError):
        QuantizedKVCache(group_size=64, bits=4).reserve(1, H, 96, torch.bfloat16, "cpu")
    with pytest.raises(ValueError):
        QuantizedKVCache(group_size=128, bits=4).reserve(1, H, 64, torch.bfloat16, "cpu")
    with pytest.raises(ValueError):
        QuantizedKVCache(group_size=64, bits=4).reserve(1, H, 64, torch.float32, "cpu")


def reference_file(path, layers=2, T=5, bits=4, gs=64, dt=torch.bfloat16):
    """A file laid out as the reference's save_cache writes a list of QuantizedKVCache (tree_flatten names)."""
    from safetensors.torch import save_file
    g = torch.Generator().manual_seed(0)
    arrays, meta = {}, {}
    for i in range(layers):
        for j in range(2):
            arrays[f"{i}.{j}.0"] = torch.randint(0, 2 ** 31, (1, H, T, D * bits // 32), generator=g, dtype=torch.int64).to(torch.uint32)
            arrays[f"{i}.{j}.1"] = torch.randn((1, H, T, D // gs), generator=g).to(dt)
            arrays[f"{i}.{j}.2"] = torch.randn((1, H, T, D // gs), generator=g).to(dt)
        for k, v in enumerate(("256", str(T), str(gs), str(bits))):
            meta[f"0.{i}.{k}"] = v
        meta[f"2.{i}"] = "QuantizedKVCache"
    meta["1.computed_ids"] = "[1, 2, 3, 4, 5]"
    save_file(arrays, str(path), metadata=meta)
    return arrays, meta


def test_reference_quantized_file_loads_and_saves_back(tmp_path):
    from safetensors import safe_open
    src = tmp_path / "ref.safetensors"
    arrays, meta = reference_file(src)
    cache, user = BaseCache.load_cache(str(src), device="cpu")
    assert user == {"computed_ids": "[1, 2, 3, 4, 5]"}
    assert len(cache) == 2 and all(isinstance(c, QuantizedKVCache) for c in cache)
    c = cache[1]
    assert (c.offset, c.group_size, c.bits, c.step) == (5, 64, 4, 256)
    assert torch.equal(c.values[2], arrays["1.1.2"]) and c.keys[0].dtype == torch.uint32
    dst = tmp_path / "back.safetensors"
    BaseCache.save_cache(str(dst), cache, user)
    with safe_open(str(dst), framework="pt") as f:
        assert f.metadata() == meta
        assert sorted(f.keys()) == sorted(arrays)
        for k in arrays:
            t = f.get_tensor(k)
            assert t.dtype == arrays[k].dtype and torch.equal(t, arrays[k]), k


def save_flat(file_name, cache, metadata):
    """save_cache as it was before QuantizedKVCache existed (the flat naming of ReusableKVCache files)."""
    from safetensors.torch import save_file
    arrays, meta = {}, {}
    for i, c in enumerate(cache):
        for j, t in enumerate(c.state):
            if t is not None:
                arrays[f"{i}.{j}"] = t.detach().to("cpu").contiguous()
        meta[f"0.{i}"] = str(c.meta_state)
        meta[f"2.{i}"] = type(c).__name__
    for k, v in (metadata or {}).items():
        meta[f"1.{k}"] = str(v)
    save_file(arrays, file_name, metadata=meta)


def test_reusable_save_file_is_unchanged(tmp_path):
    """A list of ReusableKVCache saves the same names, metadata and arrays as before."""
    g = torch.Generator().manual_seed(1)
    cache = []
    for _ in range(2):
        c = ReusableKVCache()
        c.state = (torch.randn((1, H, 7, D), generator=g).to(torch.bfloat16), torch.randn((1, H, 7, D), generator=g).to(torch.bfloat16))
        cache.append(c)
    got, want = tmp_path / "got.safetensors", tmp_path / "want.safetensors"
    BaseCache.save_cache(str(got), cache, {"computed_ids": "[9]"})
    save_flat(str(want), cache, {"computed_ids": "[9]"})
    from safetensors import safe_open
    with safe_open(str(got), framework="pt") as f, safe_open(str(want), framework="pt") as w:  # (the header's key order is not stable)
        assert f.metadata() == w.metadata() and sorted(f.keys()) == sorted(w.keys()) == ["0.0", "0.1", "1.0", "1.1"]
        for k in w.keys():
            a, b = f.get_tensor(k), w.get_tensor(k)
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), k
    back, user = BaseCache.load_cache(str(got), device="cpu")
    assert user == {"computed_ids": "[9]"} and all(isinstance(c, ReusableKVCache) and c.offset == 7 for c in back)


def test_prompt_cache_reuses_a_quantized_prefix():
    pc = PromptCache()
    layers = []
    for _ in range(2):
        c = QuantizedKVCache(bits=4)
        c.reserve(6, H, D, torch.bfloat16, "cpu"), c.advance(6)
        layers.append(c)
    pc.cache = layers
    pc.computed_ids = [1, 2, 3, 4, 5, 6]
    todo = pc([1, 2, 3, 9, 9])
    assert list(todo) == [9, 9] and all(c.offset == 3 for c in layers)
