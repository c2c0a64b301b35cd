"""Llama-shaped decoder on the MI355X decode runtime.

Host-side mirror of models/llama/language.py of the reference (ModelArgs :13-29, Attention :32-108,
MLP :111-127, TransformerBlock :130-154, LlamaModel :157-187, Model :190-219).  The reference builds a lazy MLX
graph of ~17 primitives per layer; here `Model` owns a native decoder (csrc/decoder.hip) that runs the same
graph as 5 fused HIP launches per layer, and this file only (1) repacks the checkpoint's MLX-quantised triplets
into the streaming layouts at load, and (2) keeps the reference's calling convention:

    logits[1, L, V] = model(inputs[1, L], mask=None, cache=[ReusableKVCache, ...])

The cache may be of any of the four kinds (reusable, quantized, rotating, paged); what the decoder is pointed at is kept by one
`KVBinding` (kv_binding.py), which every entry point syncs before its launch and advances after it.

Checkpoints: config["quantization"] = {"group_size": 64 | 128, "bits": 2 | 3 | 4 | 6 | 8} (2 / 3-bit codes ride the 4-bit units, 6-bit
codes the 8-bit units), no entry = dense 16-bit weights, or a per-module mix of both; 32-wide groups are refused by name.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import base
from ... import _ffi, hip_ops
from ...cache.kv_cache import BaseCache, PageAllocator, PagedKVCache, PagedSequence, ReusableKVCache
from .kv_binding import KVBinding, on_int8_pages
from .rows_state import RowsTailState
from .step_state import StepTailState
from .utils import Llama3RoPE


class ModelArgs(base.BaseModelArgs):
    """config.json keys the Llama path reads (language.py:13-29; unknown keys are ignored)."""
    model_type: str = "llama"
    hidden_size: int = 0
    num_hidden_layers: int = 0
    intermediate_size: int = 0
    num_attention_heads: int = 0
    rms_norm_eps: float = 1e-5
    vocab_size: int = 0
    head_dim: int | None = None
    max_position_embeddings: int | None = None
    num_key_value_heads: int | None = None
    attention_bias: bool = False
    mlp_bias: bool = False
    rope_theta: float = 10000
    rope_traditional: bool = False
    rope_scaling: dict | None = None
    tie_word_embeddings: bool = True
    quantization: dict | None = None


class TransformerBlock:
    """One entry of `model.layers` (PromptCache.create_kv_cache counts them, prompt_cache.py:39-41).
    Holds the layer's device weights; the arithmetic of language.py:144-154 runs inside the decoder."""

    def __init__(self, attn_norm, mlp_norm, wqkv, wo, wgateup, wdown, biases=(None, None, None, None)):
        self.input_layernorm = attn_norm
        self.post_attention_layernorm = mlp_norm
        self.wqkv, self.wo, self.wgateup, self.wdown = wqkv, wo, wgateup, wdown
        self.bqkv, self.bo, self.bgateup, self.bdown = biases  # attention_bias / mlp_bias (language.py:42-53,117-126), packed row order

    def nbytes(self) -> int:
        return sum(w.nbytes for w in (self.wqkv, self.wo, self.wgateup, self.wdown))


def _is_quantized(weights: dict, prefix: str) -> bool:
    """The reference's per-module predicate (models/utils.py:99-109): a Linear / Embedding is quantised iff the checkpoint holds
    "{path}.scales" (and its input width is a multiple of 64, which mlx_lm guarantees when it wrote the scales)."""
    return f"{prefix}.scales" in weights


def _group_format(weights: dict, names: list[str]) -> bool:
    """Quantised (True) or dense (False) for a group of Linears that this build streams as ONE matrix (q|k|v, gate|up).  The reference
    decides per module; a group whose members disagree cannot be one matrix and is refused by name."""
    flags = [_is_quantized(weights, n) for n in names]
    if any(flags) != all(flags):
        qs = [n for n, f in zip(names, flags) if f]
        ds = [n for n, f in zip(names, flags) if not f]
        raise ValueError(
            f"{', '.join(qs)} quantised but {', '.join(ds)} dense (models/utils.py:99-109 decides per module): the MI355X path streams "
            f"{' | '.join(n.rsplit('.', 1)[-1] for n in names)} as one packed matrix, so these Linears must share a format")
    return flags[0]


def _triplet(weights: dict, prefix: str):
    """The MLX-quantised triplet of one module."""
    w, s, b = weights.get(f"{prefix}.weight"), weights.get(f"{prefix}.scales"), weights.get(f"{prefix}.biases")
    if w is None:
        raise ValueError(f"{prefix}.weight is missing from the checkpoint")
    if s is None or b is None:
        raise ValueError(f'{prefix}: the checkpoint has "{prefix}.{"scales" if s is not None else "biases"}" but not both halves of the affine pair')
    return w, s, b


def _recode_mlx_codes(w: torch.Tensor, bits: int, to_bits: int) -> torch.Tensor:
    """MLX-packed codes of width `bits` (2, 3 or 6; int32 words [N, K * bits / 32]) re-packed at width `to_bits` (4 or 8).  The VALUES are
    untouched (q < 2**bits <= 2**to_bits), so w = scale * q + bias is the same number: the streaming formats here hold 4- and 8-bit codes, and
    a narrower code is a code.  MLX packs a row as a little-endian bit stream (code k at bits [k * bits, (k + 1) * bits)): 2-bit codes sixteen
    to a word, 3- and 6-bit codes eight / four to three bytes."""
    N = w.shape[0]
    by = w.contiguous().view(torch.uint8).reshape(N, -1).to(torch.int32)  # little-endian bytes of the row
    if bits == 2:
        q = torch.stack([(by >> (2 * i)) & 3 for i in range(4)], dim=-1).reshape(N, -1)
    else:
        t = by.reshape(N, -1, 3)
        v = t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)                # 24 bits = 8 three-bit or 4 six-bit codes
        n, m = (8, 7) if bits == 3 else (4, 63)
        q = torch.stack([(v >> (bits * i)) & m for i in range(n)], dim=-1).reshape(N, -1)
    q = q.to(torch.uint8)
    if to_bits == 4:
        q = q[:, 0::2] | (q[:, 1::2] << 4)
    return q.contiguous().view(torch.int32)


def _dense(weights: dict, prefix: str, dtype: torch.dtype) -> torch.Tensor:
    w = weights.get(f"{prefix}.weight")
    if w is None or w.dtype != dtype or f"{prefix}.scales" in weights:
        raise ValueError(f"{prefix}: expected a dense {dtype} weight (no '{prefix}.scales' in the checkpoint)")
    return w


class Model(RowsTailState, StepTailState):
    def __init__(self, args: ModelArgs, weights: dict[str, torch.Tensor], kv_splits: int = 0, tp=None):
        """weights: the checkpoint in the layout models/utils.py:51-125 of the reference consumes (HF names,
        `.weight` uint32 codes carried as int32, `.scales`/`.biases` in the activation dtype), on the GPU.
        tp: a connected proxy_inference_engine_amd.tp.HipComm -- this model is then ONE RANK of a tensor-parallel group: `args`
        and `weights` are the rank's shard (tp.shard_checkpoint: local heads / intermediate rows, its own `lm_head` rows, the
        full embedding table), every rank must make the same calls in the same order, and logits / logprobs cover the rank's
        vocabulary rows [rank * V / world, (rank + 1) * V / world) while the sampled token is global."""
        self.args = args
        self.tp = tp
        self.model_type = args.model_type
        device = _ffi.require_gpu()
        q = args.quantization or {}
        self.dense = not q  # no "quantization" entry: nn.Linear / nn.Embedding with 16-bit weights (models/utils.py:96-97)
        if q and (q.get("group_size") not in (32, 64, 128) or q.get("bits") not in (2, 3, 4, 6, 8)):
            # nn.quantize(model, **config["quantization"]) takes any group_size in {32, 64, 128} and bits in {2, 3, 4, 6, 8}
            # (models/utils.py:96-111): all fifteen are served.  64-wide groups are the W4S / W8S streaming units (one group per lane), 128-wide
            # groups write every scale / bias to both of their 64-wide halves (below), 32-wide groups are the W4S32 / W8S32 units (two scale /
            # bias pairs per lane); 2- / 3-bit codes ride the 4-bit units and 6-bit codes the 8-bit units (below: a narrower code is a code).
            raise ValueError(f"config['quantization'] = {dict(q)}: mx.quantize knows group_size 32, 64, 128 and bits 2, 3, 4, 6, 8 "
                             f"(got group_size={q.get('group_size')}, bits={q.get('bits')})")
        self.checkpoint_bits = int(q["bits"]) if q else 16
        # 2- and 6-bit codes in 64- / 128-wide groups stream as W2S / W6S units, 0.3125 / 0.8125 B per weight -- the checkpoint's own bytes (round 5).
        # Only the embedding TABLE (one row per step) is re-packed as 4- / 8-bit codes; a tied lm_head is packed from the original codes.
        self.native_narrow = self.checkpoint_bits if bool(q) and self.checkpoint_bits in (2, 6) and q.get("group_size") in (64, 128) else 0
        self.native_w2 = self.native_narrow == 2
        embed_codes_narrow = None
        if q and self.checkpoint_bits in (2, 3, 6):
            # Same weights, wider container: 3-bit codes (and 2- / 6-bit codes in 32-wide groups) are stored as 4-bit codes / bytes, scales and biases
            # unchanged -- every product is what the narrow code gives (same q, same affine pair, same fp32 sums); HBM holds 0.5625 / 1.0625 B per
            # weight instead of the checkpoint's 0.4375 (3-bit: a native unit would need two planes at ~2.1 VALU instructions per weight and lose).
            to_bits = 8 if self.checkpoint_bits == 6 else 4
            weights = dict(weights)
            for k in [k for k in weights if k.endswith(".scales")]:
                wk = k[:-len(".scales")] + ".weight"
                if weights[wk].shape[-1] * 32 % self.checkpoint_bits or (weights[wk].shape[-1] * 32 // self.checkpoint_bits) % 64:
                    raise ValueError(f"{wk}: {self.checkpoint_bits}-bit rows must hold a multiple of 64 codes")
                if self.native_narrow:
                    if wk == "model.embed_tokens.weight":
                        embed_codes_narrow = weights[wk]
                        weights[wk] = _recode_mlx_codes(weights[wk], self.checkpoint_bits, to_bits)
                    continue
                weights[wk] = _recode_mlx_codes(weights[wk], self.checkpoint_bits, to_bits)
            q = dict(q, bits=to_bits)
        self.group_size = int(q.get("group_size", 64)) if q else 0
        if self.group_size == 128:
            # mx.quantize(w, group_size=128): one (scale, bias) per 128 weights.  The streaming units keep one per 64-wide lane group, so each
            # is written twice: w = s q + b holds for both halves unchanged -- the same dequantised matrix (qmm regime: bit for bit), the same
            # affine sums up to fp32 association (qmv regime) -- for 0.5625 instead of the checkpoint's 0.53125 B per weight in HBM.
            weights = dict(weights)
            for k in [k for k in weights if k.endswith(".scales") or k.endswith(".biases")]:
                wk = k[:k.rindex(".")] + ".weight"
                code_bits = self.checkpoint_bits if self.native_narrow and wk != "model.embed_tokens.weight" else int(q["bits"])  # native narrow Linears keep their codes
                if (weights[wk].shape[-1] * 32 // code_bits) % 128:
                    raise ValueError(f"{k}: group_size 128 needs a multiple of 128 input features")
                weights[k] = weights[k].repeat_interleave(2, dim=-1).contiguous()
        self.bits = int(q["bits"]) if q else 16
        self.n_heads = args.num_attention_heads
        self.n_kv_heads = args.num_key_value_heads or self.n_heads
        self.head_dim = args.head_dim or args.hidden_size // self.n_heads
        self.dtype = weights["model.norm.weight"].dtype
        self.device = device
        H, I, V = args.hidden_size, args.intermediate_size, args.vocab_size
        if tp is not None:
            if (args.tie_word_embeddings and tp.world > 1) or V % (2 * tp.world):
                raise ValueError("a tensor-parallel shard carries its own lm_head rows (tie_word_embeddings=False) and needs vocab_size % (2 * world) == 0")
            V //= tp.world  # the rank's slice of the vocabulary: lm_head rows, logits, logprobs
        self.vocab_out = V
        weights = base.sanitize(weights, args.tie_word_embeddings)  # language.py:212-219

        rs = args.rope_scaling or {}
        max_len = args.max_position_embeddings or 8192  # language.py:56
        self.rope = Llama3RoPE(max_len, max_len, self.head_dim, args.rope_theta, float(rs.get("factor", 1.0)),
                               float(rs.get("low_freq_factor", 1.0)), float(rs.get("high_freq_factor", 1.0)), device=device)

        # rotate-half RoPE wants partners (i, i + D/2) on adjacent packed rows; the traditional form rotates (2i, 2i+1), which
        # already are adjacent in the plain q|k|v concatenation
        qkv_map = None if args.rope_traditional else hip_ops.qkv_row_map(self.n_heads, self.n_kv_heads, self.head_dim).to(device)
        gu_map = hip_ops.gateup_row_map(I).to(device)

        # 64-wide units also serve 128-wide groups (scales written twice, above); every Linear of a native 2- / 6-bit checkpoint streams W2S / W6S
        # units, its embedding table stays 4- / 8-bit codes (the decoder's default format: the table's)
        group = 32 if self.group_size == 32 else 64
        wfmt = _ffi.PIE_W_DENSE if self.dense else hip_ops.weight_format(self.bits, group)
        self.mixed = False  # some module is dense although config["quantization"] is set (per-module predicate, models/utils.py:99-109)

        def quantized(names: list[str]) -> bool:
            if self.dense:
                return False
            qf = _group_format(weights, names)
            self.mixed |= not qf
            return qf

        def pack(names: list[str], row_map=None):
            """One streaming-layout matrix from the (concatenated) Linear weights `names`; returns (matrix, its pie_layer_weights.fmt_* code)."""
            if not quantized(names):
                ws = [_dense(weights, n, self.dtype) for n in names]
                m = hip_ops.repack_dense(torch.cat(ws, dim=0) if len(ws) > 1 else ws[0], row_map=row_map)
            else:
                trip = [torch.cat(t, dim=0) for t in zip(*(_triplet(weights, n) for n in names))]
                if self.native_narrow and names == ["model.embed_tokens"]:  # tied lm_head: the table's own narrow codes, not the gather's 4- / 8-bit copy
                    trip[0] = embed_codes_narrow
                m = hip_ops.repack(*trip, bits=self.native_narrow or self.bits, group_size=group, row_map=row_map)
            return m, m.fmt + 1  # PIE_W_* + 1 (0 = the decoder's default format)

        def bias(names: list[str], row_map=None):
            """The (concatenated) Linear biases of `names` in the packed row order of the matching matrix; a Linear without a
            `.bias` entry contributes zeros (Qwen2-style checkpoints carry q/k/v biases but none for o_proj), None if none has one."""
            if not any(f"{n}.bias" in weights for n in names):
                return None
            rows = [int((weights[f"{n}.weight"]).shape[0]) for n in names]
            parts = [weights[f"{n}.bias"].reshape(-1).to(self.dtype) if f"{n}.bias" in weights
                     else torch.zeros(r, dtype=self.dtype, device=device) for n, r in zip(names, rows)]
            b = torch.cat(parts)
            return (b[row_map.long()] if row_map is not None else b).contiguous()

        self.layers: list[TransformerBlock] = []
        for i in range(args.num_hidden_layers):
            pfx = f"model.layers.{i}"
            (wqkv, f_qkv), (wo, f_o) = pack([f"{pfx}.self_attn.{n}_proj" for n in "qkv"], qkv_map), pack([f"{pfx}.self_attn.o_proj"])
            (wgu, f_gu), (wdown, f_down) = pack([f"{pfx}.mlp.gate_proj", f"{pfx}.mlp.up_proj"], gu_map), pack([f"{pfx}.mlp.down_proj"])
            blk = TransformerBlock(
                weights[f"{pfx}.input_layernorm.weight"].contiguous(),
                weights[f"{pfx}.post_attention_layernorm.weight"].contiguous(),
                wqkv, wo, wgu, wdown,
                biases=(bias([f"{pfx}.self_attn.{n}_proj" for n in "qkv"], qkv_map) if args.attention_bias else None,
                        bias([f"{pfx}.self_attn.o_proj"]) if args.attention_bias else None,
                        bias([f"{pfx}.mlp.gate_proj", f"{pfx}.mlp.up_proj"], gu_map) if args.mlp_bias else None,
                        bias([f"{pfx}.mlp.down_proj"]) if args.mlp_bias else None),
            )
            blk.formats = (f_qkv, f_o, f_gu, f_down)
            self.layers.append(blk)
        self.embed_quantized = quantized(["model.embed_tokens"])
        if not self.embed_quantized:
            self.embed_tokens = (_dense(weights, "model.embed_tokens", self.dtype).contiguous(), None, None)
        else:
            self.embed_tokens = tuple(t.contiguous() for t in _triplet(weights, "model.embed_tokens"))
        self.norm = weights["model.norm.weight"].contiguous()
        head = "model.embed_tokens" if args.tie_word_embeddings else "lm_head"  # language.py:206-209
        self.lm_head, f_head = pack([head])
        f_embed = (wfmt if self.embed_quantized else _ffi.PIE_W_DENSE) + 1

        # decoder-owned outputs live in torch tensors so callers can read them without copies
        self.logits = torch.zeros(V, dtype=self.dtype, device=device)
        self.logprobs = torch.zeros(V, dtype=torch.float32, device=device)
        self.token = torch.zeros(1, dtype=torch.int32, device=device)
        self.hidden = torch.zeros(H, dtype=self.dtype, device=device)

        lib = _ffi.load()
        cfg = _ffi.pie_decoder_config(_ffi.dtype_code(self.dtype), H, args.num_hidden_layers, self.n_heads, self.n_kv_heads,
                                      self.head_dim, I, V, float(args.rms_norm_eps), int(args.tie_word_embeddings), int(kv_splits),
                                      wfmt, int(bool(args.rope_traditional)),
                                      tp.rank if tp is not None else 0, tp.world if tp is not None else 0)
        self._dec = C.c_void_p()
        _ffi.check(lib.pie_decoder_create(C.byref(cfg), C.byref(self._dec)))
        if tp is not None:  # world == 1: the tensor-parallel code path on one rank (push to self / one-rank RCCL communicator)
            _ffi.check(lib.pie_decoder_set_comm(self._dec, tp.handle))
        for i, blk in enumerate(self.layers):
            lw = _ffi.pie_layer_weights(blk.input_layernorm.data_ptr(), blk.post_attention_layernorm.data_ptr(),
                                        blk.wqkv.packed.data_ptr(), blk.wo.packed.data_ptr(), blk.wgateup.packed.data_ptr(),
                                        blk.wdown.packed.data_ptr(),
                                        *(b.data_ptr() if b is not None else None for b in (blk.bqkv, blk.bo, blk.bgateup, blk.bdown)),
                                        *blk.formats)
            _ffi.check(lib.pie_decoder_set_layer(self._dec, i, C.byref(lw)))
        gw = _ffi.pie_global_weights(self.embed_tokens[0].data_ptr(), *(t.data_ptr() if t is not None else None for t in self.embed_tokens[1:]),
                                     self.norm.data_ptr(), self.lm_head.packed.data_ptr(), self.rope.freqs.data_ptr(), f_embed, f_head)
        _ffi.check(lib.pie_decoder_set_globals(self._dec, C.byref(gw)))
        # device-side token history: history[p] = greedy token chosen for position p (written by the tail kernel)
        self.history = torch.zeros(1 << 20, dtype=torch.int32, device=device)
        _ffi.check(lib.pie_decoder_bind_outputs(self._dec, _ffi.p(self.logits), _ffi.p(self.logprobs), _ffi.p(self.token), _ffi.p(self.hidden),
                                                _ffi.p(self.history), self.history.numel()))
        # the ids the model was fed, by position: the window of the step tail's repetition penalty (set_step_tail).  step / step_embeds /
        # __call__ copy explicit ids in, device to device; the decode step records a fed-back token itself
        self.fed_ids = torch.zeros(self.history.numel(), dtype=torch.int32, device=device)
        self._kv = KVBinding(lib, self._dec, len(self.layers), self.n_kv_heads, self.head_dim, self.dtype, device, tensor_parallel=tp is not None)
        self._page_pool, self._page_blocks = None, 16
        self._batch_bufs: dict = {}
        self._spec = None   # speculative decoding's record and workspaces, made when first used
        self._spec_batch_ws = None   # the batched speculative pass's workspace, made when first used
        self._spec_batch_tail_ws = None   # ... and the one of the pass under the seats' tails, zeroed when made
        self.spec_batch_last = None  # ... and its last record on the device
        self._init_rows_state()  # the multi-sequence passes' per-row tail state (rows_state.py)
        self._init_step_state()  # the single-sequence step's tail state (step_state.py)
        torch.cuda.synchronize(device)

    def __del__(self):
        dec = getattr(self, "_dec", None)
        if dec is not None and dec.value:
            try:
                _ffi.load().pie_decoder_destroy(dec)
            except Exception:
                pass
            self._dec = None

    # ------------------------------------------------------------------ cache plumbing: the caches are made here; `self._kv` (kv_binding.py)
    # points the decoder at whichever kind a call is given
    def make_cache(self) -> list[BaseCache]:
        if self._page_pool is not None:
            return self.make_paged_cache(self._page_pool, max_blocks=self._page_blocks)
        return [ReusableKVCache() for _ in self.layers]

    def enable_paged_kv(self, num_pages: int = 512, max_blocks: int = 16, kv_dtype: torch.dtype | None = None,
                        kv_scales: tuple[torch.Tensor, torch.Tensor] | None = None) -> PageAllocator:
        """From now on make_cache() (PromptCache.create_kv_cache, prompt_cache.py:34-41) hands out paged caches drawing
        on one pool of `num_pages` 64-token pages (all layers).  Returns the pool.
        kv_dtype=torch.int8: the pages are the reference KVPage's own storage (page.hpp:25-32) -- int8 K / V rows with float16 per-head
        scales; kv_scales = (k, v), each float16 [n_layers, n_kv_heads], is written into every page (None: ones, the reference
        constructor's value -- far too coarse for real activations; pass amax / 127 of a calibration prompt).  Such a pool serves
        prefill_batch / step_batch (the continuous-batching path) and the single-sequence step() / InferenceEngine: a fresh token prompt goes through
        the several-prompts pass as a batch of one (quantised into its pages on the way); a suffix behind a cached prefix, and a prompt of
        embeddings, run as decode steps (the batched single-sequence pass reads T pages)."""
        kv_dtype = self.dtype if kv_dtype is None else kv_dtype
        if kv_dtype not in (self.dtype, torch.int8):
            raise ValueError(f"kv_dtype must be the model's dtype or torch.int8, got {kv_dtype}")
        self._page_pool = PageAllocator(num_pages, self.n_kv_heads, self.head_dim, dtype=kv_dtype, device=self.device,
                                        num_layers=len(self.layers))
        if kv_dtype == torch.int8 and kv_scales is not None:
            ks, vs = (t.to(device=self.device, dtype=torch.float16).contiguous() for t in kv_scales)
            if ks.shape != (len(self.layers), self.n_kv_heads) or vs.shape != ks.shape:
                raise ValueError("kv_scales: two float16 tensors [n_layers, n_kv_heads]")
            for li in range(len(self.layers)):
                hip_ops.page_i8_set_scales(self._page_pool.slab[li], num_pages, self.n_kv_heads, self.head_dim, ks[li], vs[li])
        self._kv.match_page_format(self._page_pool, always=True)
        self._kv.invalidate()
        self._page_blocks = max_blocks
        return self._page_pool

    def make_paged_cache(self, allocator: PageAllocator | None = None, num_pages: int = 512, max_blocks: int = 16) -> list[BaseCache]:
        """Per-layer PagedKVCache objects over one PagedSequence: KV rows live in 64-token pages of
        the allocator's slab (one plane per layer) instead of per-layer contiguous buffers; growth takes pages, never
        copies.  Pass a shared `allocator` to keep several sequences in one pool."""
        if allocator is None:
            allocator = PageAllocator(num_pages, self.n_kv_heads, self.head_dim, dtype=self.dtype, device=self.device,
                                      num_layers=len(self.layers))
        if (allocator.num_layers, allocator.num_heads, allocator.head_dim) != (len(self.layers), self.n_kv_heads, self.head_dim) or \
                allocator.dtype not in (self.dtype, torch.int8) or allocator.slab is None:
            raise ValueError("the allocator's geometry does not match this model")
        seq = PagedSequence(allocator, max_blocks)
        return [PagedKVCache(seq, i) for i in range(len(self.layers))]

    def _feed(self, ids: torch.Tensor, offset: int) -> None:
        """fed_ids[offset : offset + L] = ids (device int32 [L]); positions beyond the buffer are not recorded (the penalty's window skips them)."""
        n = min(ids.numel(), self.fed_ids.numel() - offset)
        if n > 0:
            self.fed_ids[offset:offset + n].copy_(ids[:n])

    # ------------------------------------------------------------------ reference calling convention
    def __call__(self, inputs: torch.Tensor | None = None, mask=None, cache: list[BaseCache] | None = None,
                 inputs_embeds: torch.Tensor | None = None) -> torch.Tensor:
        """Model.__call__ (language.py:199-210): inputs [1, L] -> logits [1, L, V] in the activation dtype,
        lm_head on every position like the reference (the engine's fast path is `step`).
        inputs_embeds [1, L, hidden] replaces embed_tokens(inputs): the VLM text tower's entry
        (models/intern/language.py:148-158, LanguageModel(None, cache=cache, inputs_embeds=...), intern/ensemble.py:108)."""
        if inputs is None and inputs_embeds is None:
            raise ValueError("Either inputs or inputs_embeds must be provided")  # intern/language.py:188-189
        if cache is None:
            cache = self.make_cache()  # reference: cache=None means no caching; a throw-away cache is equivalent
        if mask is not None:
            self._check_mask(mask, (inputs_embeds.shape[-2] if inputs_embeds is not None else inputs.shape[-1]), cache)
        lib = _ffi.load()
        if inputs_embeds is not None:
            emb = self._check_embeds(inputs_embeds)
            L = emb.shape[0]
            self._kv.sync(cache, L)
            out = torch.empty((L, self.vocab_out), dtype=self.dtype, device=self.device)
            _ffi.check(lib.pie_decoder_prefill_embeds(self._dec, _ffi.p(emb), L, _ffi.p(out), _ffi.stream()))
        else:
            if inputs.dim() != 2 or inputs.shape[0] != 1:
                raise ValueError("batch-1 path: inputs must be [1, L]")
            ids = inputs.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
            L = ids.numel()
            self._kv.sync(cache, L)
            self._feed(ids, self._kv.offset)
            out = torch.empty((L, self.vocab_out), dtype=self.dtype, device=self.device)
            _ffi.check(lib.pie_decoder_prefill(self._dec, _ffi.p(ids), L, _ffi.p(out), _ffi.stream()))
        self._kv.advance(cache, L)
        return out.unsqueeze(0)

    def _check_mask(self, mask, L: int, cache) -> None:
        """Model.__call__(mask=...) (language.py:199-204): the reference builds the causal mask itself when none is given
        (models/base.py:37-53) and otherwise hands the caller's to sdpa.  The kernels here apply the causal mask implicitly, so a
        caller's mask is accepted when it IS that mask -- "causal", or an array blocking exactly the future positions (additive: < 0
        where blocked; boolean: False where blocked) -- and refused otherwise instead of being silently ignored."""
        if isinstance(mask, str):
            if mask != "causal":
                raise NotImplementedError(f"mask={mask!r}: only the causal mask is supported")
            return
        offset, window = int(cache[0].offset), getattr(cache[0], "max_size", None)
        if window is not None:  # a ring: the windowed mask create_attention_mask builds for it (models/base.py)
            offset = min(window, offset)
        m = torch.as_tensor(mask)
        blocked = (~m) if m.dtype == torch.bool else (m < 0)
        blocked = blocked.reshape(-1, blocked.shape[-1]) if blocked.dim() > 2 else blocked
        want = base.create_causal_mask(L, offset, window_size=window, device=blocked.device) < 0
        if blocked.shape != want.shape or not torch.equal(blocked, want):
            raise NotImplementedError(f"an explicit mask of shape {tuple(m.shape)} that is not the causal mask for {L} new positions at offset {offset} "
                                      "is not supported: the attention kernels apply the causal mask of models/base.py:37-53 implicitly")

    def _check_embeds(self, inputs_embeds: torch.Tensor) -> torch.Tensor:
        emb = inputs_embeds
        if emb.dim() == 3:
            if emb.shape[0] != 1:
                raise ValueError("batch-1 path: inputs_embeds must be [1, L, hidden]")
            emb = emb[0]
        if emb.dim() != 2 or emb.shape[1] != self.args.hidden_size or emb.shape[0] == 0:
            raise ValueError(f"inputs_embeds must be [L, {self.args.hidden_size}]")
        return emb.to(device=self.device, dtype=self.dtype).contiguous()

    def embed(self, ids: torch.Tensor) -> torch.Tensor:
        """embed_tokens(ids) -> [L, hidden] (language.py:176; the VLM ensemble starts from it, intern/ensemble.py:46)."""
        from ... import hip_ops
        ids = ids.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        if self.embed_tokens[1] is None:
            return hip_ops.embedding_dense(ids, self.embed_tokens[0])
        return hip_ops.embedding(ids, *self.embed_tokens, bits=self.bits, group_size=32 if self.group_size == 32 else 64)

    def step_embeds(self, inputs_embeds: torch.Tensor, cache: list[BaseCache], ids: torch.Tensor | None = None):
        """`step` for a prompt given as embeddings: forwards the rows, lm_head + tail on the last one only.
        ids: the token ids the rows were embedded from, recorded in `fed_ids` for the tail's repetition penalty.
        On an int8 page pool such a prompt runs as L decode steps (~1.2 ms per row on the 8B model: the batched single-sequence pass reads
        T pages and the several-prompts pass takes token ids only); warned about once."""
        emb = self._check_embeds(inputs_embeds)
        if emb.shape[0] >= 6 and on_int8_pages(cache) and not getattr(self, "_warned_i8_embeds", False):
            import warnings
            warnings.warn("a prompt of embeddings on int8 KV pages is processed one row per decode step; use T pages for VLM prompts, or token prompts", stacklevel=2)
            self._warned_i8_embeds = True
        L = emb.shape[0]
        self._kv.sync(cache, L)
        if ids is not None:
            self._feed(ids.reshape(-1).to(device=self.device, dtype=torch.int32), self._kv.offset)
        _ffi.check(_ffi.load().pie_decoder_prefill_embeds(self._dec, _ffi.p(emb), L, None, _ffi.stream()))
        self._kv.advance(cache, L)
        pos = self._kv.offset
        token = self.history[pos:pos + 1] if pos < self.history.numel() else self.token.clone()
        return token, self.logprobs, self.logits

    def step(self, ids: torch.Tensor | None, cache: list[BaseCache], graph: bool = True):
        """Fast path of _inference (engine/inference_engine.py:252-271) for the greedy sampler without logits
        processors: forwards `ids` [L] (device int32) and returns (token[1], logprobs[V], logits[V]).
        `ids=None` feeds back the previous step's greedy token, which already sits in the decoder's device-side
        state (no copy, no host sync).  L == 1 replays the captured hipGraph.
        After set_step_tail(...) the same call applies the repetition penalty and / or draws the token (and feeds THAT back).
        token is a view of the device-side history at the new position (stable); logprobs / logits are the
        decoder's output buffers, valid until the next call."""
        lib = _ffi.load()
        if ids is None:
            L = 1
            self._kv.sync(cache, L)
        else:
            ids = ids.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
            L = ids.numel()
            if L >= 6 and on_int8_pages(cache) and cache[0].offset == 0 and self._step_tail_plain:  # (the several-prompts pass ends in the greedy tail only)
                # A fresh prompt on int8 pages: the single-sequence prompt pass reads T pages (it would run the prompt as L decode steps,
                # ~1.2 ms per token), the several-prompts pass quantises into int8 pages -- one prompt is a batch of one.
                nxt, logprobs, logits = self.prefill_batch([ids.cpu().numpy()], [cache])  # (a prompt arrives once: the host copy is the pass's own row bookkeeping)
                pos = cache[0].offset  # position the chosen token will occupy
                self._kv.invalidate()   # the pass bound its own table: the next step re-binds the sequence and sets the device-side offset
                _ffi.check(lib.pie_decoder_set_token_from(self._dec, _ffi.p(nxt), _ffi.stream()))  # device to device: step(None) feeds it back
                if pos < self.history.numel():
                    self.history[pos:pos + 1].copy_(nxt[:1])
                    return self.history[pos:pos + 1], logprobs[0], logits[0]
                return nxt[:1].clone(), logprobs[0], logits[0]
            self._kv.sync(cache, L)
            self._feed(ids, self._kv.offset)
            if L == 1:
                _ffi.check(lib.pie_decoder_set_token_from(self._dec, _ffi.p(ids), _ffi.stream()))
        if L == 1:
            flags = _ffi.PIE_STEP_LOGITS | (_ffi.PIE_STEP_GRAPH if graph else 0)
            _ffi.check(lib.pie_decoder_step(self._dec, flags, _ffi.stream()))
        else:
            _ffi.check(lib.pie_decoder_prefill(self._dec, _ffi.p(ids), L, None, _ffi.stream()))
        self._kv.advance(cache, L)
        pos = self._kv.offset  # position the chosen token will occupy
        token = self.history[pos:pos + 1] if pos < self.history.numel() else self.token.clone()
        return token, self.logprobs, self.logits

    # ------------------------------------------------------------------ greedy speculative decoding
    # One int32 record at a stable address carries everything the host reads per pass, in one copy:
    #   [0] n | [1:33] the pass's tokens (n of them, then -1) | [33] the next draft's count | [34:65] the next draft | [65] the drafter's len
    _SPEC_N, _SPEC_TOK, _SPEC_COUNT, _SPEC_DRAFT, _SPEC_LEN, _SPEC_WORDS = 0, 1, 33, 34, 65, 66

    def _spec_state(self) -> dict:
        """The record, the pass's workspace and log-probability rows, the drafter's workspace: made when first used."""
        if self._spec is None:
            self._spec = {"rec": torch.zeros(self._SPEC_WORDS, dtype=torch.int32, device=self.device),
                          "logprobs": torch.empty((hip_ops.SPEC_MAX_ROWS, self.vocab_out), dtype=torch.float32, device=self.device),
                          "draft_ws": hip_ops.ngram_draft_workspace(self.device), "host": None}
            self._spec_ws(self._spec, "ws", "pie_decoder_spec_workspace_bytes", False, hip_ops.SPEC_MAX_ROWS)
        return self._spec

    def _spec_ws(self, store: dict, key: str, size_fn: str, zeroed: bool, *dims) -> torch.Tensor:
        """store[key] = the workspace of one kind of speculative pass, made when first used: `size_fn`(decoder, *dims) bytes, zeroed once
        where the sampler's part is carried from pass to pass."""
        if store.get(key) is None:
            nbytes = int(getattr(_ffi.load(), size_fn)(self._dec, *dims))
            store[key] = (torch.zeros if zeroed else torch.empty)((nbytes + 15) // 16 * 2, dtype=torch.int64, device=self.device)
        return store[key]

    def _refuse(self, who: str, rows) -> None:
        """The speculative passes' refusals by name: rows = ((set or not, the part's name), ...)."""
        for bad, name in rows:
            if bad:
                raise ValueError(f"{who}: not available with {name}")

    def _spec_refused_rows(self) -> tuple:
        """The parts of the step's tail that no speculative pass under a tail takes."""
        return ((self._top_n is not None, "top_logprobs"), (self._cnt is not None, "frequency / presence penalties"), (self._dry is not None, "a DRY penalty"))

    @property
    def spec_min_rows(self) -> int:
        """The fewest rows (drafts + 1) a speculative pass takes: below it the many-row pass would run as iterated steps."""
        v = int(_ffi.load().pie_get_knob(_ffi.KNOBS["prefill_min"]))
        return 6 if v < 0 else max(v, 2)

    @property
    def spec_draft(self) -> torch.Tensor:
        """Device int32 [31]: the ids the last drafter launch left (`draft`, or `spec_step(then_draft=...)`); spec_read() tells how many."""
        return self._spec_state()["rec"][self._SPEC_DRAFT:self._SPEC_LEN]

    @property
    def spec_tokens(self) -> torch.Tensor:
        """Device int32 [32]: the tokens of the last pass (or, after `draft`, the one token it drafted behind), then -1."""
        return self._spec_state()["rec"][self._SPEC_TOK:self._SPEC_COUNT]

    def spec_read(self) -> tuple[list[int], int]:
        """(the tokens of the last pass or step, the count of the draft made behind them): ONE read-back of the record, kept until the
        next launch that writes it."""
        sp = self._spec_state()
        if sp["host"] is None:
            sp["host"] = sp["rec"].cpu().numpy()
        h = sp["host"]
        n = int(h[self._SPEC_N])
        return [int(t) for t in h[self._SPEC_TOK:self._SPEC_TOK + n]], int(h[self._SPEC_COUNT])

    def _check_speculative(self, who: str, cache) -> None:
        self._check_speculative_kv(who, cache)
        if not self._step_tail_plain:
            raise ValueError(f"{who}: speculation is greedy and raw -- set_step_tail() with its defaults first "
                             "(no sampler, repetition penalty, token mask, logit bias, top_logprobs or frequency / presence penalty)")

    def _check_speculative_kv(self, who: str, cache) -> None:
        if self.tp is not None:
            raise ValueError(f"{who}: not available on a tensor-parallel model")
        if on_int8_pages(cache):
            raise ValueError(f"{who}: not available on int8 KV pages")
        if not isinstance(cache[0], (ReusableKVCache, PagedKVCache)):
            raise ValueError(f"{who}: runs on ReusableKVCache or 16-bit PagedKVCache, not on {type(cache[0]).__name__}")

    def _queue_draft(self, ngram_max: int, ngram_min: int, k: int, grammar: bool = False) -> None:
        sp = self._spec_state()
        rec = sp["rec"]
        sp["host"] = None
        out = (rec[self._SPEC_DRAFT:self._SPEC_LEN], rec[self._SPEC_COUNT:self._SPEC_COUNT + 1])
        hip_ops.ngram_draft(self.fed_ids, rec[self._SPEC_LEN:self._SPEC_LEN + 1], ngram_max, ngram_min, k, workspace=sp["draft_ws"], out=out)
        if grammar:
            # one more launch, in place on the record's draft and count words, from the automaton's device-side state
            if self._dfa is None:
                raise ValueError("draft(grammar=True): set_step_tail(token_automaton=...) first")
            hip_ops.token_dfa_draft(self._dfa_rec, self._dfa_state, self._dfa_arena, self._step_automaton_forced, self.vocab_out, out[0], out[1], k, out=out)

    def spec_read_draft(self) -> list[int]:
        """The ids of the draft spec_read() counted, from the same read-back."""
        count = self.spec_read()[1]
        return [int(t) for t in self._spec_state()["host"][self._SPEC_DRAFT:self._SPEC_DRAFT + count]]

    def draft(self, ngram_max: int = 3, ngram_min: int = 1, k: int = 7, grammar: bool = False):
        """The prompt-lookup drafter over the sequence of the cache last stepped (hip_ops.ngram_draft): its ids are `fed_ids` up to the
        position the last chosen token will occupy, which is copied in from `history` on the device -- a fed-back token never visits the
        host.  Queued behind the step, no host sync; returns (spec_draft, count [1]) as device views, and spec_read() then gives
        ([the last chosen token], count) in one read-back.  grammar=True (needs set_step_tail(token_automaton=...)): one
        hip_ops.token_dfa_draft launch follows, in place, from the automaton's device-side state -- the looked-up ids are cut at the
        first one the grammar forbids and every forced id is put in, so a forced run is drafted even when nothing was looked up."""
        pos = self._kv.offset
        if pos is None or not 0 < pos < self.fed_ids.numel():
            raise ValueError("draft: step a prompt first (and stay inside the model's id history)")
        rec = self._spec_state()["rec"]
        self.fed_ids[pos:pos + 1].copy_(self.history[pos:pos + 1])
        rec[self._SPEC_TOK:self._SPEC_TOK + 1].copy_(self.history[pos:pos + 1])
        rec[self._SPEC_N:self._SPEC_N + 1].fill_(1)
        rec[self._SPEC_LEN:self._SPEC_LEN + 1].fill_(pos + 1)
        self._queue_draft(ngram_max, ngram_min, k, grammar)
        return self.spec_draft, rec[self._SPEC_COUNT:self._SPEC_COUNT + 1]

    def spec_step(self, draft_ids: torch.Tensor, cache: list[BaseCache], then_draft: tuple | None = None):
        """One speculative pass (pie_decoder_spec_step): the previous call's token and the m ids of `draft_ids` (device int32) go through
        the many-row pass at once, and the drafts are accepted while each equals the greedy token of the row before it.  Returns
        (tokens int32 [n] device view, n, logprobs fp32 [n, V] device view): the n = accepted + 1 tokens greedy decoding would have
        produced and their rows' log-probabilities, valid until the next call; the model, the cache (offset + n) and `fed_ids` are
        then exactly where n calls of step(None) would have left them, so step(None) right after feeds back the last accepted token.
        then_draft = (ngram_max, ngram_min, k): the next draft is queued behind the pass before the host reads n -- the pass costs ONE
        read-back (spec_read() returns it without another).  m + 1 rows: spec_min_rows .. 32.  Contiguous and 16-bit paged caches; the
        greedy raw tail only.  Pages taken for rejected rows stay with the sequence."""
        self._check_speculative("spec_step", cache)
        return self._spec_pass("spec_step", "pie_decoder_spec_step", "ws", draft_ids, cache, then_draft)

    def _spec_pass(self, who: str, entry: str, ws: str, draft_ids: torch.Tensor, cache: list[BaseCache], then_draft: tuple | None, extra: tuple = ()):
        """What spec_step, spec_step_tail and spec_step_draft share: the record, the library entry on workspace `ws`, the drafter hand-off,
        the one read-back and the cache advance.  extra: the entry's arguments between the draft and the outputs."""
        draft_ids = draft_ids.reshape(-1)
        if not draft_ids.is_cuda or draft_ids.dtype != torch.int32 or not draft_ids.is_contiguous():
            raise ValueError(f"{who}: draft_ids is a contiguous int32 device tensor")
        m = draft_ids.numel()
        if not self.spec_min_rows <= m + 1 <= hip_ops.SPEC_MAX_ROWS:
            raise ValueError(f"{who}: {m} drafts make {m + 1} rows, outside {self.spec_min_rows}..{hip_ops.SPEC_MAX_ROWS} (run a plain step below)")
        sp = self._spec_state()
        rec = sp["rec"]
        self._kv.sync(cache, m + 1)
        if self._kv.offset + m + 1 > self.fed_ids.numel():
            raise ValueError(f"{who}: the pass would run past the model's id history")
        sp["host"] = None
        _ffi.check(getattr(_ffi.load(), entry)(self._dec, _ffi.p(draft_ids), m, *extra, _ffi.p(rec[self._SPEC_TOK:]), _ffi.p(rec[self._SPEC_N:]),
                                               _ffi.p(sp["logprobs"]), _ffi.p(sp[ws]), _ffi.p(self.fed_ids), self.fed_ids.numel(),
                                               _ffi.p(rec[self._SPEC_LEN:]), _ffi.stream()))
        sp["last_ws"] = ws
        if then_draft is not None:
            self._queue_draft(*then_draft)
        n = len(self.spec_read()[0])  # the one read-back
        self._kv.advance(cache, n)    # the rejected rows stay behind the offset and are overwritten
        return rec[self._SPEC_TOK:self._SPEC_TOK + n], n, sp["logprobs"][:n]

    def spec_step_tail(self, draft_ids: torch.Tensor, cache: list[BaseCache], then_draft: tuple | None = None):
        """spec_step under the configured tail (pie_decoder_spec_step_tail): after set_step_tail(sampler=..., xtc=...,
        repetition_penalty=..., logit_bias=...) -- at least one of them -- row r's logits get the repetition penalty over the ids a plain
        step at that position would see (the drafts before it included) and the logit bias, its token is drawn at stream position c + r
        (c = the samplers' position before the pass; the argmax under the greedy sampler), and the drafts are accepted while each equals
        the token of the row before it.  The same returns as spec_step; all m + 1 rows of the log-probabilities are written, and
        spec_logits() then holds the PROCESSED logits.  Afterwards the model, the cache, `fed_ids` and the samplers' stream are exactly
        where n calls of step(None) under the same tail would have left them.  A token mask, a token automaton, top_logprobs, frequency / presence
        penalties and DRY are refused by name, like tensor-parallel models, int8 pages and the other cache kinds."""
        who = "spec_step_tail"
        self._check_speculative_kv(who, cache)
        self._refuse(who, ((self._edits[0], "a token mask"), (self._dfa is not None, "a token automaton"), *self._spec_refused_rows()))
        if self._tail[:2] == (None, None) and self._edits[1] == 0:
            raise ValueError(f"{who}: no sampler, repetition penalty or logit bias is set -- the greedy and raw pass is spec_step")
        self._spec_ws(self._spec_state(), "tail_ws", "pie_decoder_spec_tail_workspace_bytes", True, hip_ops.SPEC_MAX_ROWS)
        return self._spec_pass(who, "pie_decoder_spec_step_tail", "tail_ws", draft_ids, cache, then_draft)

    def spec_step_grammar(self, draft_ids: torch.Tensor, cache: list[BaseCache], then_draft: tuple | None = None):
        """spec_step_tail under a token automaton (pie_decoder_spec_step_dfa): after set_step_tail(token_automaton=..., and
        any of sampler / xtc / repetition_penalty / logit_bias) row r is masked in the state the drafts before it lead to -- the automaton
        is walked along draft_ids on the device --, edited and drawn as spec_step_tail's rows are, and the drafts are accepted while each
        equals the token of the row before it.  The same returns; afterwards the model, the cache, `fed_ids`, the samplers' stream and
        the automaton's state are where n calls of step(None) under the same tail would have left them.  then_draft may carry a fourth
        entry, grammar (Model.draft's).  Without an automaton the pass is spec_step_tail's; a token mask, top_logprobs, frequency /
        presence penalties and DRY are refused by name, like tensor-parallel models, int8 pages and the other cache kinds."""
        who = "spec_step_grammar"
        self._check_speculative_kv(who, cache)
        self._refuse(who, ((self._edits[0], "a token mask"), *self._spec_refused_rows()))
        if self._dfa is None:
            raise ValueError(f"{who}: no token automaton is set -- the pass without one is spec_step_tail")
        self._spec_ws(self._spec_state(), "grammar_ws", "pie_decoder_spec_dfa_workspace_bytes", True, hip_ops.SPEC_MAX_ROWS)  # a workspace of its own
        return self._spec_pass(who, "pie_decoder_spec_step_dfa", "grammar_ws", draft_ids, cache, then_draft)

    def spec_step_draft(self, draft_ids: torch.Tensor, q_logprobs: torch.Tensor, cache: list[BaseCache], *, draft_seed: int):
        """One speculative pass over a block a draft MODEL proposed (pie_decoder_spec_step_draft): spec_step_tail's pass and
        per-row edits, with speculative sampling's acceptance in place of "the draw equals the draft".  q_logprobs fp32 [m, V] (device):
        row i = the drafter's log-probabilities at the step that drew draft_ids[i], under the same (mode, temp, p, k) as this model's
        sampler and ANOTHER seed, draft_seed (samplers._rng.draft_state's): under the target's seed the drafter's Gumbels would be those
        of the target's residual draw at the same call index, and the result would no longer be distributed as the target's -- refused.
        Draft i is accepted with probability min(1, P_i(d) / Q_i(d)); the token behind the accepted prefix is
        drawn from the residual max(0, P - Q) (or, behind a fully accepted block, from the last row), so every returned token is
        distributed as a plain step's.  The same returns as spec_step; all m + 1 rows of the log-probabilities are written and the
        samplers' stream moves by n.  A stochastic sampler is required (set_step_tail(sampler=...)); a repetition penalty and a logit
        bias are applied; XTC, a token mask, top_logprobs, frequency / presence penalties and DRY are refused by name, like
        tensor-parallel models, int8 pages and the other cache kinds."""
        who = "spec_step_draft"
        self._check_speculative_kv(who, cache)
        self._refuse(who, ((self._xtc is not None, "XTC"), (self._edits[0], "a token mask"), *self._spec_refused_rows()))
        if self._tail[0] is None:
            raise ValueError(f"{who}: no stochastic sampler is set -- a greedy draft is a point mass, verified by spec_step or spec_step_tail")
        if int(draft_seed) & (2 ** 64 - 1) == int(self._tail[2]) & (2 ** 64 - 1):
            raise ValueError(f"{who}: not available with a drafter under the target's seed (samplers._rng.draft_state gives the drafter's)")
        m = draft_ids.numel()
        if not q_logprobs.is_cuda or q_logprobs.dtype != torch.float32 or q_logprobs.dim() != 2 or q_logprobs.shape[0] < m or \
                q_logprobs.shape[1] != self.vocab_out or not q_logprobs.is_contiguous():
            raise ValueError(f"{who}: q_logprobs is a contiguous fp32 [>= {m}, {self.vocab_out}] device tensor (a vocabulary mismatch is refused)")
        self._spec_ws(self._spec_state(), "draft_model_ws", "pie_decoder_spec_draft_workspace_bytes", True, hip_ops.SPEC_MAX_ROWS)
        return self._spec_pass(who, "pie_decoder_spec_step_draft", "draft_model_ws", draft_ids, cache, None, extra=(_ffi.p(q_logprobs),))

    def spec_logits(self, rows: int) -> torch.Tensor:
        """The logits block [rows, V] of the last pass (a view of its workspace, valid until the next one): raw after spec_step, processed
        after spec_step_tail."""
        sp = self._spec_state()
        return sp[sp.get("last_ws", "ws")].view(self.dtype)[:rows * self.vocab_out].view(rows, self.vocab_out)

    def draft_rows(self, seq_ids: torch.Tensor, seq_len: torch.Tensor, ngram_max: int, ngram_min: int, k: int, out: tuple):
        """The prompt-lookup drafter over several sequences' ids at once (hip_ops.ngram_draft_rows): seq_ids int32 [B, cap], seq_len int32
        [B], out = (drafts int32 [B, k], counts int32 [B]) on the device; queued, no host sync."""
        return hip_ops.ngram_draft_rows(seq_ids, seq_len, ngram_max, ngram_min, k, out=out)

    def spec_step_batch(self, tokens: torch.Tensor, caches: list[list[BaseCache]], drafts: torch.Tensor, counts, seq_ids: torch.Tensor | None = None,
                        seq_len: torch.Tensor | None = None, then_draft: tuple | None = None):
        """One speculative pass for several decode-state sequences (pie_decoder_spec_step_batch): tokens [B] = every sequence's
        input token, caches as step_batch takes them (16-bit pages), drafts device int32 [>= B, >= the largest count] = row s's drafted ids, counts = the
        host's m_s for every sequence, 0..7 (the first m_s ids of its row are verified; their sum + B is at most 256).  Sequence s presents
        1 + m_s rows; its drafts are accepted while each equals the greedy token of the row before it.  Returns (n, tokens, next_counts):
        n[s] = accepted + 1, tokens[s] = the n[s] tokens greedy decoding would have produced (host lists), next_counts = None; every cache
        advances by n[s] -- the pages taken for rejected rows stay with the sequence, their K / V lie behind the offset and are overwritten
        before anything attends to them -- and `spec_batch_last` holds the record on the device: "tokens" int32 [B, 8], "n" int32 [B].
        seq_ids int32 [>= B, cap] / seq_len int32 [>= B] (together): the sequences' ids, row s = sequence s, the last id being its input
        token -- the pass writes the chosen tokens behind it and moves seq_len on the device.  then_draft = (ngram_max, ngram_min, k,
        drafts_out): hip_ops.ngram_draft_rows over those rows is queued behind the pass, before the host reads anything, into drafts_out
        [B, k], and next_counts are its counts, read back with the pass's one record.  Greedy and raw: int8 pages, tensor-parallel models
        and any armed per-row state of the multi-sequence passes are refused by name."""
        return self._spec_batch_pass("spec_step_batch", False, tokens, caches, drafts, counts, seq_ids, seq_len, then_draft)

    def spec_step_batch_tail(self, tokens: torch.Tensor, caches: list[list[BaseCache]], drafts: torch.Tensor, counts, seq_ids: torch.Tensor | None = None,
                             seq_len: torch.Tensor | None = None, then_draft: tuple | None = None):
        """spec_step_batch under the sequences' own samplers, repetition penalties and logit biases (pie_decoder_spec_step_batch_tail;
        DESIGN.md 25): the same arguments and returns.  Needs set_batch_tail armed; record, ring, bias table (set_batch_edits' bias part)
        and XTC record (set_batch_xtc) s belong to sequence s, as in step_batch.  Row j of sequence s is edited with its seat's penalty over
        its own window and its seat's bias and drawn with the draw a plain step would make at the seat's stream position calls + j; a draft
        is accepted while it equals the draw, so tokens[s] are the n[s] tokens that many step_batch calls would have produced.  Afterwards
        the seat's `calls` and ring stand where those steps would have left them, on the device.  `spec_batch_last` additionally holds
        "logprobs" fp32 [N, V] (every row's processed log-probabilities), "logits" [N, V] (the processed block, a view of the workspace,
        valid until the next pass) and "seg_first" int32 [B + 1].  Refused by name, before anything moves: int8 pages, tensor-parallel
        models, a mask part of the batch edits, batch token automata, a batch count penalty, a batch DRY penalty, batch top log-probabilities
        and prompt scoring."""
        return self._spec_batch_pass("spec_step_batch_tail", True, tokens, caches, drafts, counts, seq_ids, seq_len, then_draft)

    def _spec_batch_pass(self, who: str, tail: bool, tokens, caches, drafts, counts, seq_ids, seq_len, then_draft):
        """spec_step_batch's and spec_step_batch_tail's body: the refusals, the index arrays, the entry's call and the one read-back."""
        import numpy as np
        seqs = self._kv.sequences(who, caches)
        B = len(seqs)
        a = seqs[0].allocator
        if self.tp is not None:
            raise ValueError(f"{who}: not available on a tensor-parallel model")
        if a.dtype == torch.int8:
            raise ValueError(f"{who}: not available on int8 KV pages")
        if tail:
            if self._batch_tail is None:
                raise ValueError(f"{who}: no batch tail is set (set_batch_tail; the greedy and raw pass is spec_step_batch)")
            refused = ((self._batch_dfa, "batch token automata"), (None if self._batch_edits is None else self._batch_edits["masks"], "a mask part of the batch logits edits"),
                       (self._batch_counts, "a batch count penalty"), (self._batch_dry, "a batch DRY penalty"))
        else:
            refused = ((self._batch_tail, "a batch tail"), (self._batch_edits, "batch logits edits"), (self._batch_counts, "a batch count penalty"),
                       (self._batch_dry, "a batch DRY penalty"), (self._batch_xtc, "batch XTC records"), (self._batch_dfa, "batch token automata"))
        self._refuse(who, ((armed is not None, name) for armed, name in refused))
        tokens = torch.as_tensor(tokens).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        m = [int(c) for c in counts]
        if tokens.numel() != B or len(m) != B:
            raise ValueError(f"{who}: one token and one count per sequence")
        if any(not 0 <= c <= hip_ops.SPEC_SEG_ROWS - 1 for c in m) or B + sum(m) > hip_ops.SPEC_BATCH_ROWS:
            raise ValueError(f"{who}: every count is 0..{hip_ops.SPEC_SEG_ROWS - 1} and the pass holds at most {hip_ops.SPEC_BATCH_ROWS} rows")
        if any(s.offset < 1 for s in seqs):
            raise ValueError(f"{who}: a decoding sequence holds its prompt already")
        if not drafts.is_cuda or drafts.dtype != torch.int32 or drafts.dim() != 2 or not drafts.is_contiguous() or drafts.shape[0] < B or \
                drafts.shape[1] < max(max(m), 1):
            raise ValueError(f"{who}: drafts is a contiguous int32 device tensor [>= B, >= the largest count]")
        if (seq_ids is None) != (seq_len is None):
            raise ValueError(f"{who}: seq_ids and seq_len come together")
        if seq_ids is not None and (seq_ids.dtype != torch.int32 or seq_len.dtype != torch.int32 or seq_ids.dim() != 2 or not seq_ids.is_contiguous() or
                                    not seq_len.is_contiguous() or seq_ids.shape[0] < B or seq_len.numel() < B or not seq_ids.is_cuda or not seq_len.is_cuda):
            raise ValueError(f"{who}: seq_ids int32 [>= B, cap] and seq_len int32 [>= B] are contiguous device tensors")
        if then_draft is not None and seq_ids is None:
            raise ValueError(f"{who}: then_draft needs seq_ids and seq_len")
        for s, c in zip(seqs, m):
            s.reserve(1 + c)
        # the index arrays, as step_mixed forms them: row r of sequence s at position offset_s + (r - first_s)
        rows = np.asarray([1 + c for c in m], dtype=np.int32)
        N = int(rows.sum())
        seg_first = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
        row_seq = np.repeat(np.arange(B, dtype=np.int32), rows)
        row_ctx = (np.repeat(np.asarray([s.offset for s in seqs], dtype=np.int32), rows) + np.arange(N, dtype=np.int32) - np.repeat(seg_first[:-1], rows) + 1).astype(np.int32)
        mb = max(len(s.pages) for s in seqs)
        table = np.zeros((B, mb), np.int32)
        for i, s in enumerate(seqs):
            table[i, :len(s.pages)] = s.pages
        index = torch.from_numpy(np.concatenate([seg_first, row_seq, row_ctx, table.reshape(-1)])).to(self.device)   # one upload
        t_first, t_seq, t_ctx, t_table = index[:B + 1], index[B + 1:B + 1 + N], index[B + 1 + N:B + 1 + 2 * N], index[B + 1 + 2 * N:]
        lib = _ffi.load()
        V = self.vocab_out
        if tail:
            ws = self._spec_ws(vars(self), "_spec_batch_tail_ws", "pie_decoder_spec_batch_tail_workspace_bytes", True)
            logprobs = torch.empty((N, V), dtype=torch.float32, device=self.device)
        else:
            ws, logprobs = self._spec_ws(vars(self), "_spec_batch_ws", "pie_decoder_spec_batch_workspace_bytes", False), None
        rec = torch.empty(B * (hip_ops.SPEC_SEG_ROWS + 2), dtype=torch.int32, device=self.device)   # tokens [B, 8] | n [B] | the next draft's counts [B]
        out_tok, out_n, nxt_cnt = rec[:B * hip_ops.SPEC_SEG_ROWS], rec[B * hip_ops.SPEC_SEG_ROWS:B * (hip_ops.SPEC_SEG_ROWS + 1)], rec[B * (hip_ops.SPEC_SEG_ROWS + 1):]
        head = (self._dec, _ffi.p(tokens), _ffi.p(drafts), drafts.shape[1], _ffi.p(t_ctx), _ffi.p(t_seq), _ffi.p(t_first), N, B, *self._kv.pool_args(a), _ffi.p(t_table), mb,
                _ffi.p(out_tok), _ffi.p(out_n))
        back = (_ffi.p(seq_ids), _ffi.p(seq_len), 0 if seq_ids is None else seq_ids.shape[1], _ffi.p(ws), _ffi.stream())
        rc = lib.pie_decoder_spec_step_batch_tail(*head, _ffi.p(logprobs), *back) if tail else lib.pie_decoder_spec_step_batch(*head, *back)
        if rc == -5:   # PIE_E_STATE: some per-row state of the multi-sequence passes is armed (top_logprobs, prompt scoring): the caller's fault, by name
            raise ValueError(f"{who}: " + lib.pie_last_error().decode("utf-8", "replace"))
        _ffi.check(rc)
        if then_draft is not None:
            ngram_max, ngram_min, k, drafts_out = then_draft
            self.draft_rows(seq_ids[:B], seq_len[:B], ngram_max, ngram_min, k, out=(drafts_out[:B], nxt_cnt))
        host = rec.cpu().numpy()   # the one read-back
        n = host[B * hip_ops.SPEC_SEG_ROWS:B * (hip_ops.SPEC_SEG_ROWS + 1)].tolist()
        toks = [host[s * hip_ops.SPEC_SEG_ROWS:s * hip_ops.SPEC_SEG_ROWS + n[s]].tolist() for s in range(B)]
        for s, k_ in zip(seqs, n):
            s.advance(k_)
        self.spec_batch_last = {"tokens": out_tok.view(B, hip_ops.SPEC_SEG_ROWS), "n": out_n}
        if tail:
            self.spec_batch_last.update(logprobs=logprobs, logits=ws.view(self.dtype)[:N * V].view(N, V), seg_first=t_first)
        return n, toks, (host[B * (hip_ops.SPEC_SEG_ROWS + 1):].tolist() if then_draft is not None else None)

    def step_batch(self, tokens: torch.Tensor, caches: list[list[BaseCache]], graph: bool = True):
        """One decode step for several sequences at once (continuous batching over the page pool; pie_decoder_step_batch):
        tokens [B] = each sequence's input token, caches = their per-layer PagedKVCache lists (model.make_cache() after
        enable_paged_kv(), all drawing on one PageAllocator, each already holding its prompt -- e.g. through step()).
        Returns (next_tokens [B] int32 greedy, logprobs [B, V] fp32, logits [B, V]) -- buffers owned by the model per batch size,
        valid until the next step_batch of that size; every cache advances by one position.  graph: replay a captured hipGraph
        of the step while the batch size and table width stay the same (captured on the second such step).
        The weights stream once for the whole batch: int4 models run the few-row MFMA GEMM up to 32 sequences."""
        seqs = self._kv.sequences("step_batch", caches)
        B = len(seqs)
        tokens = tokens.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        if tokens.numel() != B:
            raise ValueError("step_batch: one token per sequence")
        for s in seqs:
            s.reserve(1)
        # Persistent device buffers per batch size (the captured graph of the step keeps pointing at them): inputs are copied in,
        # the block table (batch_details.hpp:52-66) is rewritten in place when a sequence takes a page or the batch changes.
        mb = max(len(s.pages) for s in seqs)
        buf = self._batch_bufs.get(B)
        if buf is not None:
            self._batch_bufs[B] = self._batch_bufs.pop(B)  # most recently used last
        if buf is None or buf["table"].shape[1] < mb:
            V = self.args.vocab_size
            width = max(mb, 2 * buf["table"].shape[1]) if buf is not None else max(mb, 4)
            buf = {"table": torch.zeros((B, width), dtype=torch.int32, device=self.device),
                   "tokens": torch.empty(B, dtype=torch.int32, device=self.device), "ctx": torch.empty(B, dtype=torch.int32, device=self.device),
                   "logits": torch.empty((B, V), dtype=self.dtype, device=self.device),
                   "logprobs": torch.empty((B, V), dtype=torch.float32, device=self.device),
                   "next": torch.empty(B, dtype=torch.int32, device=self.device), "key": None}
            self._batch_bufs.pop(B, None)
            while len(self._batch_bufs) >= 4:  # a serving loop revisits few batch sizes: keep the 4 most recent sets (each [B, V] fp32 + T)
                self._batch_bufs.pop(next(iter(self._batch_bufs)))
            self._batch_bufs[B] = buf
        key = tuple(tuple(s.pages) for s in seqs)  # the page ids themselves: truncate + regrow reorders them at equal length, and id() of a retired sequence can be reused
        if buf["key"] != key:
            table = torch.zeros(buf["table"].shape, dtype=torch.int32)
            for i, s in enumerate(seqs):
                table[i, :len(s.pages)] = torch.tensor(s.pages, dtype=torch.int32)
            buf["table"].copy_(table)
            buf["key"] = key
        buf["tokens"].copy_(tokens)
        buf["ctx"].copy_(torch.tensor([s.offset + 1 for s in seqs], dtype=torch.int32))
        _ffi.check(_ffi.load().pie_decoder_step_batch(self._dec, _ffi.p(buf["tokens"]), _ffi.p(buf["ctx"]), *self._kv.pool_args(seqs[0].allocator), _ffi.p(buf["table"]),
                                                      buf["table"].shape[1], B, _ffi.p(buf["logits"]), _ffi.p(buf["logprobs"]), _ffi.p(buf["next"]),
                                                      _ffi.PIE_STEP_GRAPH if graph else 0, _ffi.stream()))
        nxt, logprobs, logits = buf["next"], buf["logprobs"], buf["logits"]
        for s in seqs:
            s.advance(1)
        return nxt, logprobs, logits

    def batch_graph_launches(self) -> int:
        """Kernel nodes of the step_batch graph captured last (-1 before the first capture)."""
        return int(_ffi.load().pie_decoder_batch_graph_launches(self._dec))

    def batch_graph_replays(self) -> int:
        """step_batch calls so far that replayed the captured graph."""
        return int(_ffi.load().pie_decoder_batch_graph_replays(self._dec))

    def prefill_batch(self, prompts: list, caches: list[list[BaseCache]]):
        """Several fresh prompts in ONE pass (pie_decoder_prefill_batch): their rows are concatenated for the GEMMs, every row keeps
        its own position, every prompt its own pages and a causal attention over its own rows only.  caches: empty paged caches
        (make_cache() after enable_paged_kv(), one per prompt).  Returns (next_tokens [S], logprobs [S, V], logits [S, V]) for the
        prompts' last positions; every cache then holds its prompt."""
        return self._varlen_pass("prefill_batch", None, [], prompts, caches)

    def step_mixed(self, tokens: torch.Tensor | None, decode_caches: list[list[BaseCache]], prompts: list, prompt_caches: list[list[BaseCache]]):
        """Decode-state sequences AND fresh prompts in one pass over the weights (pie_decoder_step_mixed; the reference's BatchDetails holds
        both kinds, batch_details.hpp:10-88): tokens [B] = the input token of each decoding sequence (caches as in step_batch), prompts /
        prompt_caches as in prefill_batch -- or caches that already hold a PREFIX (offset > 0: the next chunk of a long prompt, or a suffix
        behind shared prefix pages of a forked sequence): such rows attend to the sequence's pages from that offset.  Returns (next_tokens [B + S], logprobs [B + S, V], logits [B + S, V]): the decoding sequences
        first, then every prompt's last position; the decode caches advance by one position, the prompt caches hold their prompts.
        Every row rides the many-row regime of the Linears (as the rows of a prompt do), also when B alone would take the few-row one."""
        return self._varlen_pass("step_mixed", tokens, decode_caches, prompts, prompt_caches)

    def _varlen_pass(self, who: str, tokens, decode_caches, prompts, caches):
        import numpy as np
        every = self._kv.sequences(who, list(decode_caches) + list(caches))
        B = len(decode_caches)
        dseqs, seqs = every[:B], every[B:]
        if who == "prefill_batch" and any(s.offset for s in seqs):
            raise ValueError(f"{who} takes fresh caches for the prompts (nothing cached before the prompt)")
        if len(prompts) != len(seqs):
            raise ValueError(f"{who}: one prompt per prompt cache")
        a = every[0].allocator
        if B:
            tokens = torch.as_tensor(tokens).reshape(-1).to(device=self.device, dtype=torch.int32)   # stays on the device: no host sync per pass
            if tokens.numel() != B:
                raise ValueError(f"{who}: one token per decoding sequence")
            if any(s.offset < 1 for s in dseqs):
                raise ValueError(f"{who}: a decoding sequence holds its prompt already")
        lens = [len(p) for p in prompts]
        if (lens and min(lens) < 1) or B + sum(lens) > 65535:
            raise ValueError(f"{who}: prompts must be non-empty and the pass holds at most 65535 rows")
        cached = [int(s.offset) for s in seqs]      # > 0: the prompt continues a cached prefix (a chunk of a long prompt, a suffix behind shared pages)
        if any(cached) and a.dtype == torch.int8:
            raise ValueError(f"{who}: a prompt that continues a cached prefix reads T pages (int8 pools: fresh prompts and decoding rows)")
        for s in dseqs:
            s.reserve(1)
        for s, n in zip(seqs, lens):
            s.reserve(n)
        S, N = len(seqs), sum(lens)
        starts = (B + np.concatenate([[0], np.cumsum(lens)[:-1]])).astype(np.int32) if S else np.zeros(0, np.int32)
        ids = np.concatenate([np.zeros(B, np.int32)] + [np.asarray(p, dtype=np.int32).reshape(-1) for p in prompts])   # the decode rows' ids are copied in on the device
        rows_d = np.arange(B, dtype=np.int32)
        rows_p = np.arange(B, B + N, dtype=np.int32)
        cont = np.repeat(np.asarray(cached, dtype=np.int32) > 0, lens) if S else np.zeros(0, bool)   # rows of continuing prompts: trivial segments
        row_seq = np.concatenate([rows_d, B + np.repeat(np.arange(S, dtype=np.int32), lens)]).astype(np.int32)
        row_ctx = np.concatenate([np.asarray([s.offset + 1 for s in dseqs], dtype=np.int32),
                                  rows_p - np.repeat(starts, lens) + np.repeat(np.asarray(cached, dtype=np.int32), lens) + 1]).astype(np.int32)
        seg_lo = np.concatenate([rows_d, np.where(cont, rows_p, np.repeat(starts, lens))]).astype(np.int32)
        seg_hi = np.arange(1, B + N + 1, dtype=np.int32)
        last = np.concatenate([rows_d, starts + np.asarray(lens, dtype=np.int32) - 1]).astype(np.int32)
        chunks = np.asarray([[starts[i], lens[i], cached[i], B + i] for i in range(S) if cached[i] > 0], dtype=np.int32).reshape(-1, 4)
        mb = max(len(s.pages) for s in every)
        table = np.zeros((B + S, mb), np.int32)
        for i, s in enumerate(every):
            table[i, :len(s.pages)] = s.pages
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        t_ids, t_seq, t_ctx, t_lo, t_hi, t_last, t_table = (dev(x) for x in (ids, row_seq, row_ctx, seg_lo, seg_hi, last, table))
        if B:
            t_ids[:B] = tokens
        V = self.args.vocab_size
        logits = torch.empty((B + S, V), dtype=self.dtype, device=self.device)
        logprobs = torch.empty((B + S, V), dtype=torch.float32, device=self.device)
        nxt = torch.empty(B + S, dtype=torch.int32, device=self.device)
        lib = _ffi.load()
        head = (self._dec, _ffi.p(t_ids), _ffi.p(t_ctx), _ffi.p(t_seq), _ffi.p(t_lo), _ffi.p(t_hi), _ffi.p(t_last), B + N, B + S)
        tail = (*self._kv.pool_args(a), _ffi.p(t_table), mb, _ffi.p(logits), _ffi.p(logprobs), _ffi.p(nxt))
        if B or len(chunks):
            _ffi.check(lib.pie_decoder_step_mixed(*head, B, *tail, len(chunks), chunks.ctypes.data if len(chunks) else None, _ffi.stream()))
        else:
            _ffi.check(lib.pie_decoder_prefill_batch(*head, *tail, _ffi.stream()))
        for s in dseqs:
            s.advance(1)
        for s, k in zip(seqs, lens):
            s.advance(k)
        return nxt, logprobs, logits

    def step_bytes(self, T: int, with_logits: bool = True) -> int:
        """Algorithmic HBM bytes of one decode step at context length T."""
        return int(_ffi.load().pie_decoder_step_bytes(self._dec, int(T), int(with_logits)))

    def launch_kernel(self, name: str, layer: int = 0) -> None:
        """Enqueues ONE launch of the step's sequence (for per-kernel timing); needs a prior step() for valid state."""
        _ffi.check(_ffi.load().pie_decoder_launch_kernel(self._dec, _ffi.KERNELS[name], int(layer), _ffi.stream()))

    def graph_launches(self, with_logits: bool = True) -> int:
        """Kernel nodes of the captured step graph (hipGraphGetNodes); -1 before the first graph-replayed step."""
        return int(_ffi.load().pie_decoder_graph_launches(self._dec, 1 if with_logits else 0))

    def kernel_bytes(self, name: str, T: int) -> int:
        return int(_ffi.load().pie_decoder_kernel_bytes(self._dec, _ffi.KERNELS[name], int(T)))

    def weight_bytes(self) -> int:
        return sum(b.nbytes() for b in self.layers) + self.lm_head.nbytes
