from .kv_cache import BaseCache, QuantizedKVCache, ReusableKVCache, RotatingKVCache
from .prompt_cache import PromptCache

__all__ = ["BaseCache", "ReusableKVCache", "QuantizedKVCache", "RotatingKVCache", "PromptCache"]
