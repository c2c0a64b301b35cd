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

    # -- persistence (cache/kv_cache/__init__.py:163-210): one .safetensors file, arrays named by their position in the
    # nested [layer][keys|values] list ("3.0" = layer 3 keys), metadata flattened the same way:
    # "0.<i>" = meta_state of layer i, "1.<key>" = the caller's metadata, "2.<i>" = cache class name of layer i.
    # A QuantizedKVCache layer's state and meta_state are nested one level deeper, as tree_flatten names them: arrays
    # "<i>.<0 keys | 1 values>.<0 codes | 1 scales | 2 biases>", meta "0.<i>.<0 step | 1 offset | 2 group_size | 3 bits>".
    # A RotatingKVCache layer: arrays "<i>.0" / "<i>.1" (its state), meta "0.<i>.<k>" = keep, max_size, step, offset, _idx.
    @staticmethod
    def save_cache(file_name: str, cache: list["BaseCache"], metadata: dict[str, str] | None = None) -> None:
        from safetensors.torch import save_file
        arrays: dict[str, torch.Tensor] = {}
        meta: dict[str, str] = {}
        for i, c in enumerate(cache):
            if isinstance(c, RotatingKVCache):
                for j, t in enumerate(c.state):
                    if t is not None:
                        arrays[f"{i}.{j}"] = t.detach().to("cpu").contiguous()
                for k, v in enumerate(c.meta_state):
                    meta[f"0.{i}.{k}"] = v
                meta[f"2.{i}"] = type(c).__name__
                continue
            if isinstance(c, QuantizedKVCache):
                for j, triple in enumerate(c.state):
                    for k, t in enumerate(triple or ()):
                        arrays[f"{i}.{j}.{k}"] = t.detach().to("cpu").contiguous()
                for k, v in enumerate(c.meta_state):
                    meta[f"0.{i}.{k}"] = v
                meta[f"2.{i}"] = type(c).__name__
                continue
            for j, t in enumerate(c.state):
                if t is not None:
                    arrays[f"{i}.{j}"] = t.detach().to("cpu").contiguous()
            meta[f"0.{i}"] = str(c.meta_state)
            # a paged cache is stored as its gathered rows, the layout a ReusableKVCache restores from
            meta[f"2.{i}"] = "ReusableKVCache" if type(c).__name__ == "PagedKVCache" else type(c).__name__
        for k, v in (metadata or {}).items():
            meta[f"1.{k}"] = str(v)
        save_file(arrays, file_name, metadata=meta)

    @staticmethod
    def load_cache(file_name: str, device=None) -> tuple[list["BaseCache"], dict[str, str]]:
        from safetensors import safe_open
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        classes = {"ReusableKVCache": ReusableKVCache, "QuantizedKVCache": QuantizedKVCache, "RotatingKVCache": RotatingKVCache}
        with safe_open(file_name, framework="pt", device="cpu") as f:
            meta = f.metadata() or {}
            n = sum(1 for k in meta if k.startswith("2."))
            cache: list[BaseCache] = []
            for i in range(n):
                name = meta[f"2.{i}"]
                if name not in classes:
                    raise ValueError(f"{file_name}: cache class {name} is not on the MI355X path")
                if name == "RotatingKVCache":
                    # the reference's loader calls the class without arguments, which RotatingKVCache(max_size) does not accept: the size
                    # comes from the meta strings here
                    ms = tuple(meta[f"0.{i}.{k}"] for k in range(5))
                    c = RotatingKVCache(max_size=int(ms[1]), keep=int(ms[0]), step=int(ms[2]))
                    if f"{i}.0" in f.keys():
                        c.state = (f.get_tensor(f"{i}.0").to(device), f.get_tensor(f"{i}.1").to(device))
                    c.meta_state = ms
                    cache.append(c)
                    continue
                c = classes[name]()
                if isinstance(c, QuantizedKVCache):
                    keys = f.keys()
                    if f"{i}.0.0" in keys:
                        c.state = tuple(tuple(f.get_tensor(f"{i}.{j}.{k}").to(device) for k in range(3)) for j in range(2))
                    c.meta_state = tuple(meta[f"0.{i}.{k}"] for k in range(4))
                    cache.append(c)
                    continue
                state = tuple(f.get_tensor(f"{i}.{j}").to(device) if f"{i}.{j}" in f.keys() else None for j in range(2))
                c.state = state
                c.meta_state = meta.get(f"0.{i}", "")
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

    @abstractmethod
    def trim(self, n: int) -> int: ...

    @abstractmethod
    def update_and_fetch(self, keys: torch.Tensor, values: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]: ...

    @abstractmethod
    def to_quantized(self, group_size: int = 64, bits: int = 4) -> "BaseCache": ...


from .reusable import ReusableKVCache  # noqa: E402
from .paged import PageAllocator, PagedKVCache, PagedSequence  # noqa: E402
from .quantized import QuantizedKVCache  # noqa: E402
from .rotating import RotatingKVCache  # noqa: E402

__all__ = ["BaseCache", "ReusableKVCache", "QuantizedKVCache", "RotatingKVCache", "PagedKVCache", "PagedSequence", "PageAllocator"]
