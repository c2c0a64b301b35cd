"""KV-cache protocol of the decode path (host-side mirror of the reference's
cache/kv_cache/__init__.py:10-161; buffers are torch ROCm tensors instead of mx.array)."""
from __future__ import annotations

from abc import ABC, abstractmethod

import torch


class BaseCache(ABC):
    """Interface every per-layer cache implements (cache/kv_cache/__init__.py:10-161)."""

    offset: int
    step: int

    @staticmethod
    def make_kv_cache(model, max_kv_size: int | None = None, reusable: bool = True) -> list["BaseCache"]:
        # max_kv_size: a RotatingKVCache(max_kv_size, keep=4) per layer.  The reference gets there through a model without make_cache, which
        # its Llama is; this project's Llama has a make_cache, so the ring is chosen here first to keep that behaviour.
        if max_kv_size is not None:
            if getattr(model, "_page_pool", None) is not None:
                raise ValueError("max_kv_size: a rotating KV cache runs on contiguous buffers, not on the model's KV pages")
            return [RotatingKVCache(max_size=max_kv_size, keep=4) for _ in range(len(model.layers))]
        if hasattr(model, "make_cache") and model.make_cache is not None:
            return model.make_cache()
        if max_kv_size is not None or not reusable:
            raise NotImplementedError("only ReusableKVCache is on the engine path (prompt_cache.py:34-41, :73)")
        return [ReusableKVCache() for _ in range(len(model.layers))]

    # -- persistence (cache/kv_cache/__init__.py:163-210): one .safetensors file.  The per-layer `state` list and the metadata list
    # [per-layer meta_state, the caller's metadata, per-layer class names] are flattened by position, as tree_flatten names them:
    # arrays "3.0" = layer 3 keys (a QuantizedKVCache: "3.0.<0 codes | 1 scales | 2 biases>"), metadata "0.<i>" = meta_state of
    # layer i (a tuple: "0.<i>.<k>"), "1.<key>" = the caller's, "2.<i>" = the class layer i is restored as.
    saved_as: str | None = None      # the class name a layer is stored under, if not its own
    meta_args: dict[str, int] = {}   # constructor arguments load_cache takes from the stored meta_state: name -> position (the reference
                                     # calls every class without arguments, which RotatingKVCache(max_size) does not accept)

    @staticmethod
    def save_cache(file_name: str, cache: list["BaseCache"], metadata: dict[str, str] | None = None) -> None:
        from safetensors.torch import save_file
        arrays: dict[str, torch.Tensor] = {}
        meta: dict[str, str] = {}
        for i, c in enumerate(cache):
            _flatten(c.state, str(i), arrays)
            _flatten(c.meta_state, f"0.{i}", meta)
            meta[f"2.{i}"] = c.saved_as or type(c).__name__
        for k, v in (metadata or {}).items():
            meta[f"1.{k}"] = str(v)
        save_file({k: t.detach().to("cpu").contiguous() for k, t in arrays.items()}, file_name, metadata=meta)

    @staticmethod
    def load_cache(file_name: str, device=None) -> tuple[list["BaseCache"], dict[str, str]]:
        from safetensors import safe_open
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        classes = {cls.__name__: cls for cls in (ReusableKVCache, QuantizedKVCache, RotatingKVCache)}
        with safe_open(file_name, framework="pt", device="cpu") as f:
            meta = f.metadata() or {}
            arrays = {k: f.get_tensor(k).to(device) for k in f.keys()}
        cache: list[BaseCache] = []
        for i in range(sum(1 for k in meta if k.startswith("2."))):
            name = meta[f"2.{i}"]
            if name not in classes:
                raise ValueError(f"{file_name}: cache class {name} is not on the MI355X path")
            state, meta_state = _unflatten(arrays, str(i)), _unflatten(meta, f"0.{i}")
            c = classes[name](**{k: int(meta_state[j]) for k, j in classes[name].meta_args.items()})
            if state is not None:
                c.state = state
            c.meta_state = meta_state
            cache.append(c)
        return cache, {k[2:]: v for k, v in meta.items() if k.startswith("1.")}

    @property
    def state(self):
        return []

    @state.setter
    def state(self, v):
        if v is not None and v:
            raise ValueError("This cache has no state but a state was set.")

    @property
    def meta_state(self):
        return ""

    @meta_state.setter
    def meta_state(self, v):
        if v is not None and v:
            raise ValueError("This cache has no meta_state but a meta_state was set.")

    def is_trimmable(self) -> bool:
        return False

    # The decode kernels append the new rows themselves, so every cache on the decode path also offers update_and_fetch as its two
    # halves, which the decoder's binding (models/llama/kv_binding.py) calls on every layer around a model call:
    #   reserve(needed, n_kv_heads, head_dim, dtype, device)   room for `needed` more positions behind `offset`: allocates or grows the
    #                                                          [1, n_kv_heads, capacity, head_dim] buffers where the cache owns them
    #   advance(n)                                             books the `n` rows the decoder has written: offset += n

    @abstractmethod
    def trim(self, n: int) -> int: ...

    @abstractmethod
    def update_and_fetch(self, keys: torch.Tensor, values: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]: ...

    @abstractmethod
    def to_quantized(self, group_size: int = 64, bits: int = 4) -> "BaseCache": ...


def _flatten(tree, name: str, out: dict) -> None:
    """tree_flatten: the leaves of nested tuples / lists under dotted position names; None holds nothing."""
    if isinstance(tree, (tuple, list)):
        for i, t in enumerate(tree):
            _flatten(t, f"{name}.{i}", out)
    elif tree is not None:
        out[name] = tree


def _unflatten(flat: dict, name: str):
    """tree_unflatten of what _flatten stored under `name`: the leaf, a tuple of what lies below it, or None."""
    if name in flat:
        return flat[name]
    if not any(k.startswith(name + ".") for k in flat):
        return None
    below = []
    while (t := _unflatten(flat, f"{name}.{len(below)}")) is not None:
        below.append(t)
    return tuple(below) or None


from .reusable import ReusableKVCache  # noqa: E402
from .paged import PageAllocator, PagedKVCache, PagedSequence  # noqa: E402
from .quantized import QuantizedKVCache  # noqa: E402
from .rotating import RotatingKVCache  # noqa: E402

__all__ = ["BaseCache", "ReusableKVCache", "QuantizedKVCache", "RotatingKVCache", "PagedKVCache", "PagedSequence", "PageAllocator"]
