"""The token mask of structured decoding: what the reference's first processor, structuring_engine.process_logits, does to the logits
(engine/inference_engine.py:319-335) -- only the allowed token ids stay finite.  Defined here: a disallowed id becomes
-inf, an allowed id keeps its bits.  The mask travels as packed words (hip_ops.pack_token_mask: token i is bit i & 31 of word i >> 5).
The processor carries `.mask` (packed host int32 words, or None), `.mask_fn` (a callable tokens -> mask, or None) and `.vocab_size` (the length of the bool mask it was made from, or None): where the engine
can, it applies the mask inside the decode step's tail (hip_ops.logprobs_argmax_masked's kernel, Model.set_step_tail) and never calls it."""
from __future__ import annotations

from collections.abc import Callable

import torch

from ..hip_ops import pack_token_mask


def packed_token_mask(mask, vocab_size: int) -> torch.Tensor:
    """Any accepted form of a mask -- packed int32 words, a bool [V] tensor, an iterable of allowed ids -- as HOST int32 words
    [ceil(V / 32)].  ValueError for too few words and for a mask that allows no token below V."""
    V = int(vocab_size)
    n = (V + 31) // 32
    if isinstance(mask, torch.Tensor) and mask.dtype == torch.int32:
        words = mask.detach().reshape(-1).cpu()
        if words.numel() < n:
            raise ValueError(f"token mask: {n} words for a vocabulary of {V}, got {words.numel()}")
        words = words[:n].contiguous()
        tail = words.clone()
        if V % 32:
            tail[-1] &= (1 << (V % 32)) - 1  # bits at or beyond V are ignored
        if not bool(tail.any()):
            raise ValueError("token mask: no token is allowed")
        return words
    return pack_token_mask(mask, V)


def unpack_token_mask(words: torch.Tensor, vocab_size: int, device=None) -> torch.Tensor:
    """bool [V]: True where the packed mask allows the token."""
    w = words.to(device) if device is not None else words
    i = torch.arange(int(vocab_size), device=w.device)
    return ((w[i >> 5] >> (i & 31)) & 1).bool()


def make_token_mask(mask_or_fn) -> Callable:
    """mask_or_fn: packed int32 words, a bool [V] mask, or a callable tokens -> either of them (or an iterable of allowed ids) that
    receives prompt_cache.computed_ids -- every id the model was fed so far, the current row's included."""
    mask_fn = mask_or_fn if callable(mask_or_fn) else None
    mask = vocab_size = None
    if mask_fn is None:
        if not isinstance(mask_or_fn, torch.Tensor) or mask_or_fn.dtype not in (torch.bool, torch.int32):
            raise ValueError("make_token_mask takes packed int32 words, a bool [V] mask or a callable tokens -> mask")
        if mask_or_fn.dtype == torch.bool:
            vocab_size = mask_or_fn.numel()  # a bool mask says which vocabulary it is for
            mask = pack_token_mask(mask_or_fn, vocab_size)
        else:
            mask = mask_or_fn.detach().reshape(-1).cpu().contiguous()

    def token_mask_processor(tokens, logits: torch.Tensor) -> torch.Tensor:
        V = logits.shape[-1]
        check_vocab(token_mask_processor, V)
        words = packed_token_mask(mask if mask_fn is None else mask_fn(tokens), V)
        return logits.masked_fill_(~unpack_token_mask(words, V, logits.device), float("-inf"))

    token_mask_processor.mask, token_mask_processor.mask_fn, token_mask_processor.vocab_size = mask, mask_fn, vocab_size
    return token_mask_processor


def check_vocab(proc, vocab_size: int) -> None:
    """ValueError when the processor was made from a bool mask of another length than the vocabulary it is applied to."""
    if proc.vocab_size is not None and proc.vocab_size != int(vocab_size):
        raise ValueError(f"token mask: a bool mask of {proc.vocab_size} entries for a vocabulary of {int(vocab_size)}")
