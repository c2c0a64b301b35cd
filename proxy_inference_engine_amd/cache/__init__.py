from .kv_cache import BaseCache, QuantizedKVCache, ReusableKVCache
from .prompt_cache import PromptCache

__all__ = ["BaseCache", "ReusableKVCache", "QuantizedKVCache", "PromptCache"]
