"""Op-level host mirror of the MLX ops the reference's decode path calls, on torch (ROCm) tensors.

Same names and argument meaning as the `mx.*` call sites (paths relative to
/root/reference/src/proxy_inference_engine/):
  quantize / dequantize            <- mx.quantize / mx.dequantize   (cache/kv_cache/cache.py:144-147)
  quantized_matmul                 <- mx.quantized_matmul           (via nn.QuantizedLinear, models/utils.py:111)
  rms_norm, rope, scaled_dot_product_attention  <- mx.fast.*        (language.py:137-141, llama/utils.py:42-50, base.py:111-113)
Every function launches hand-written HIP kernels through the C ABI on torch's current stream;
there is no torch-op or CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import _ffi

U32 = torch.int32  # uint32 code words are carried in int32 tensors (same bits)


def _dev(t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise ValueError("pie_hip ops take device tensors (ROCm); got a CPU tensor")
    if not t.is_contiguous():
        raise ValueError("pie_hip ops take contiguous tensors")


def quantize(w: torch.Tensor, group_size: int = 64, bits: int = 4):
    """mx.quantize(w, group_size=64, bits=2|4|6|8): w [N,K] -> (codes [N,K*bits/32] uint32-in-int32, scales, biases [N,K/64])."""
    if group_size != 64 or bits not in (2, 4, 6, 8):
        raise ValueError("only group_size=64 with bits=2, 4, 6 or 8 is implemented")
    _dev(w)
    N, K = w.shape
    if K % 64:
        raise ValueError(f"last dimension must be a multiple of 64, got {K}")
    codes = torch.empty((N, K * bits // 32), dtype=U32, device=w.device)
    scales = torch.empty((N, K // 64), dtype=w.dtype, device=w.device)
    biases = torch.empty_like(scales)
    _ffi.check(_ffi.load().pie_quantize_g64(_ffi.p(w), N, K, bits, _ffi.dtype_code(w.dtype), _ffi.p(codes), _ffi.p(scales),
                                            _ffi.p(biases), _ffi.stream()))
    return codes, scales, biases


def dequantize(codes: torch.Tensor, scales: torch.Tensor, biases: torch.Tensor, group_size: int = 64, bits: int = 4):
    if group_size != 64 or bits not in (4, 8):
        raise ValueError("only group_size=64 with bits=4 or 8 is implemented")
    for t in (codes, scales, biases):
        _dev(t)
    N, K = codes.shape[0], codes.shape[1] * 32 // bits
    out = torch.empty((N, K), dtype=scales.dtype, device=codes.device)
    _ffi.check(_ffi.load().pie_dequantize_g64(_ffi.p(codes), _ffi.p(scales), _ffi.p(biases), N, K, bits,
                                              _ffi.dtype_code(scales.dtype), _ffi.p(out), _ffi.stream()))
    return out


class _Format(NamedTuple):
    bits: int                # code bits (16: dense 16-bit weights)
    group_size: int | None   # weights per scale / bias pair (None: dense)
    size: str                # the C ABI's packed size, repack and streaming-GEMV entry points
    repack: str
    gemv: str


# The streaming formats (include/pie_hip.h PIE_W_*), keyed by their PIE_W_* code
FORMATS = {
    _ffi.PIE_W_INT4_G64: _Format(4, 64, "pie_w4s_bytes", "pie_repack_w4g64", "pie_qgemv_w4g64"),
    _ffi.PIE_W_DENSE: _Format(16, None, "pie_w16s_bytes", "pie_repack_dense", "pie_gemv_dense"),
    _ffi.PIE_W_INT8_G64: _Format(8, 64, "pie_w8s_bytes", "pie_repack_w8g64", "pie_qgemv_w8g64"),
    _ffi.PIE_W_INT4_G32: _Format(4, 32, "pie_w4s32_bytes", "pie_repack_w4g32", "pie_qgemv_w4g32"),
    _ffi.PIE_W_INT8_G32: _Format(8, 32, "pie_w8s32_bytes", "pie_repack_w8g32", "pie_qgemv_w8g32"),
    _ffi.PIE_W_INT2_G64: _Format(2, 64, "pie_w2s_bytes", "pie_repack_w2g64", "pie_qgemv_w2g64"),
    _ffi.PIE_W_INT6_G64: _Format(6, 64, "pie_w6s_bytes", "pie_repack_w6g64", "pie_qgemv_w6g64"),
}


def weight_format(bits: int, group_size: int) -> int:
    """The PIE_W_* code of MLX triplets with these bits and group size (ValueError if no streaming format holds them)."""
    for fmt, f in FORMATS.items():
        if (f.bits, f.group_size) == (bits, group_size):
            return fmt
    raise ValueError(f"no streaming format for bits={bits}, group_size={group_size}")


@dataclass
class PackedWeight:
    """One Linear in its streaming layout (include/pie_hip.h): fmt is the PIE_W_* format of `packed`."""
    packed: torch.Tensor          # uint8 [pie_w*s_bytes(N, K)]
    N: int
    K: int
    dtype: torch.dtype
    fmt: int
    lin_bias: torch.Tensor | None = None

    @property
    def bits(self) -> int:
        return FORMATS[self.fmt].bits

    @property
    def group_size(self) -> int | None:
        return FORMATS[self.fmt].group_size

    @property
    def nbytes(self) -> int:
        return self.packed.numel()


def _packed_buffer(fmt: int, N_out: int, K: int, device) -> torch.Tensor:
    nbytes = getattr(_ffi.load(), FORMATS[fmt].size)(N_out, K)
    if nbytes == 0:
        raise ValueError(f"unsupported shape for {FORMATS[fmt].repack}: N={N_out} (must be even), K={K} (multiple of 64)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _row_map(row_map: torch.Tensor | None, device) -> torch.Tensor | None:
    return None if row_map is None else row_map.to(device=device, dtype=torch.int32).contiguous()


def repack(codes, scales, biases, *, bits: int, group_size: int = 64, row_map: torch.Tensor | None = None, lin_bias=None) -> PackedWeight:
    """Load-time repack of an MLX-quantised Linear -- mx.quantize's triplet: weight uint32 [N_src, K*bits/32] (6 bits: MLX's bit stream),
    scales / biases [N_src, K/group_size] -- into its streaming layout.  row_map (int32 [N_out]) selects / reorders source rows (q|k|v
    concatenation, gate/up interleave)."""
    fmt = weight_format(bits, group_size)
    for t in (codes, scales, biases):
        _dev(t)
    N_src, K = codes.shape[0], codes.shape[1] * 32 // bits
    if K * bits != codes.shape[1] * 32 or tuple(scales.shape) != (N_src, K // group_size) or tuple(biases.shape) != (N_src, K // group_size):
        raise ValueError(f"{bits}-bit rows must hold whole codes and scales / biases must be [{N_src}, {K // group_size}]; got "
                         f"{tuple(codes.shape)} / {tuple(scales.shape)} / {tuple(biases.shape)}")
    N_out = N_src if row_map is None else int(row_map.numel())
    packed, row_map = _packed_buffer(fmt, N_out, K, codes.device), _row_map(row_map, codes.device)
    _ffi.check(getattr(_ffi.load(), FORMATS[fmt].repack)(_ffi.p(codes), _ffi.p(scales), _ffi.p(biases), N_src, K, _ffi.p(row_map), N_out,
                                                         _ffi.p(packed), _ffi.stream()))
    return PackedWeight(packed, N_out, K, scales.dtype, fmt, lin_bias)


# repack for one format each, like the C ABI's pie_repack_w4g64 .. pie_repack_w8g32 (repack_w4s32(bits=8) is repack_w8s32)
repack_w4s, repack_w8s, repack_w2s, repack_w6s = (functools.partial(repack, bits=b) for b in (4, 8, 2, 6))
repack_w4s32, repack_w8s32 = functools.partial(repack, bits=4, group_size=32), functools.partial(repack, bits=8, group_size=32)


def repack_dense(w: torch.Tensor, row_map: torch.Tensor | None = None, lin_bias=None) -> PackedWeight:
    """Load-time repack of an nn.Linear weight [N_src, K] (bf16 / f16) into W16S; row_map as for repack."""
    _dev(w)
    if w.dtype not in (torch.bfloat16, torch.float16) or w.dim() != 2:
        raise ValueError("dense weights must be 2-D bfloat16 / float16")
    N_src, K = w.shape
    N_out = N_src if row_map is None else int(row_map.numel())
    packed, row_map = _packed_buffer(_ffi.PIE_W_DENSE, N_out, K, w.device), _row_map(row_map, w.device)
    _ffi.check(_ffi.load().pie_repack_dense(_ffi.p(w), N_src, K, _ffi.p(row_map), N_out, _ffi.p(packed), _ffi.stream()))
    return PackedWeight(packed, N_out, K, w.dtype, _ffi.PIE_W_DENSE, lin_bias)


def linear(x: torch.Tensor, w: PackedWeight) -> torch.Tensor:
    """nn.Linear.__call__ / nn.QuantizedLinear.__call__ on a packed weight: x [..., K] -> [..., N]; fp32 accumulate, one rounding
    (+ bias in T), on the format's streaming-GEMV entry point."""
    _dev(x)
    if x.shape[-1] != w.K or x.dtype != w.dtype:
        raise ValueError(f"x [..., {x.shape[-1]}] {x.dtype} does not match weight K={w.K} {w.dtype}")
    M = x.numel() // w.K
    y = torch.empty((*x.shape[:-1], w.N), dtype=x.dtype, device=x.device)
    _ffi.check(getattr(_ffi.load(), FORMATS[w.fmt].gemv)(_ffi.p(x), M, _ffi.p(w.packed), w.N, w.K, _ffi.p(w.lin_bias), _ffi.p(y),
                                                        _ffi.dtype_code(x.dtype), _ffi.stream()))
    return y


def embedding_dense(ids: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """nn.Embedding.__call__: ids int32 [L] -> [L, H] rows of the T [V, H] table."""
    _dev(ids)
    _dev(table)
    ids = ids.to(torch.int32).contiguous().view(-1)
    V, H = table.shape
    out = torch.empty((ids.numel(), H), dtype=table.dtype, device=table.device)
    _ffi.check(_ffi.load().pie_embedding_dense(_ffi.p(ids), ids.numel(), _ffi.p(table), V, H, _ffi.dtype_code(table.dtype), _ffi.p(out),
                                               _ffi.stream()))
    return out


def quantized_matmul(x: torch.Tensor, w: PackedWeight, transpose: bool = True, group_size: int | None = None, bits: int | None = None):
    """mx.quantized_matmul(x, w, scales, biases, transpose=True, group_size, bits) on a packed weight: x [..., K] -> [..., N]; fp32
    accumulate, result in x.dtype (+ nn.QuantizedLinear's bias when present)."""
    if not transpose or (group_size is not None and group_size != w.group_size) or (bits is not None and bits != w.bits):
        raise ValueError("only transpose=True with the weight's own group size and bit width is implemented (the nn.QuantizedLinear form)")
    return linear(x, w)


def quantized_matmul_partial(x: torch.Tensor, w: PackedWeight) -> torch.Tensor:
    """The fp32 row sums of quantized_matmul before their rounding to T: x [..., K] -> fp32 [..., N].  Row-parallel shards of a
    tensor-parallel Linear are summed over the ranks in this form (tp.py)."""
    _dev(x)
    if w.fmt != _ffi.PIE_W_INT4_G64 or x.shape[-1] != w.K or x.dtype != w.dtype:
        raise ValueError("quantized_matmul_partial takes an int4 group-64 weight matching x's last dimension and dtype")
    M = x.numel() // w.K
    y = torch.empty((*x.shape[:-1], w.N), dtype=torch.float32, device=x.device)
    _ffi.check(_ffi.load().pie_qgemv_w4g64_f32(_ffi.p(x), M, _ffi.p(w.packed), w.N, w.K, _ffi.p(y), _ffi.dtype_code(x.dtype), _ffi.stream()))
    return y


def embedding(ids: torch.Tensor, codes, scales, biases, bits: int = 4, group_size: int = 64) -> torch.Tensor:
    """nn.QuantizedEmbedding.__call__: ids int32 [L] -> [L, H]."""
    _dev(ids)
    ids = ids.to(torch.int32).contiguous().view(-1)
    V, H = codes.shape[0], codes.shape[1] * 32 // bits
    out = torch.empty((ids.numel(), H), dtype=scales.dtype, device=codes.device)
    if group_size == 32:
        _ffi.check(_ffi.load().pie_embedding_g32(_ffi.p(ids), ids.numel(), _ffi.p(codes), _ffi.p(scales), _ffi.p(biases), V, H, bits,
                                                 _ffi.dtype_code(scales.dtype), _ffi.p(out), _ffi.stream()))
        return out
    _ffi.check(_ffi.load().pie_embedding_g64(_ffi.p(ids), ids.numel(), _ffi.p(codes), _ffi.p(scales), _ffi.p(biases), V, H, bits,
                                             _ffi.dtype_code(scales.dtype), _ffi.p(out), _ffi.stream()))
    return out


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """mx.fast.rms_norm(x, weight, eps) over the last axis."""
    _dev(x), _dev(weight)
    H = x.shape[-1]
    y = torch.empty_like(x)
    _ffi.check(_ffi.load().pie_rms_norm(_ffi.p(x), _ffi.p(weight), float(eps), x.numel() // H, H, _ffi.dtype_code(x.dtype),
                                        _ffi.p(y), _ffi.stream()))
    return y


def rope(x: torch.Tensor, dims: int, traditional: bool = False, base=None, scale: float = 1.0, offset: int = 0,
         freqs: torch.Tensor | None = None) -> torch.Tensor:
    """mx.fast.rope(x[..., heads, L, D], dims, traditional, base=None, scale=1.0, offset, freqs)."""
    if base is not None or scale != 1.0 or freqs is None or dims != x.shape[-1]:
        raise ValueError("only the Llama3RoPE form is implemented: base=None, scale=1.0, freqs given, dims=D")
    _dev(x), _dev(freqs)
    L, D = x.shape[-2:]
    y = torch.empty_like(x)
    _ffi.check(_ffi.load().pie_rope_ex(_ffi.p(x), x.numel() // (L * D), L, D, _ffi.p(freqs), int(offset), int(bool(traditional)),
                                       _ffi.dtype_code(x.dtype), _ffi.p(y), _ffi.stream()))
    return y


_sdpa_ws: dict = {}


def scaled_dot_product_attention(q, k, v, scale: float, mask=None, T: int | None = None) -> torch.Tensor:
    """mx.fast.scaled_dot_product_attention for the decode step: q [1,Hq,1,D]; k,v [1,Hkv,cap,D] buffers whose
    first T positions are attended (default: all); mask must be None (L == 1: models/base.py:39-53)."""
    if q.shape[0] != 1:
        raise NotImplementedError("batch 1 only")
    if q.shape[-2] != 1:  # prompt form: mask must be the causal one ("causal"; models/base.py:37-53 builds exactly that)
        if not (isinstance(mask, str) and mask == "causal"):
            raise NotImplementedError("L > 1 needs mask='causal' (the additive causal mask of models/base.py:18-53)")
        for t in (q, k, v):
            _dev(t)
        _, Hq, L, D = q.shape
        Hkv, cap = k.shape[1], k.shape[2]
        total = cap if T is None else int(T)
        qt = q[0].transpose(0, 1).contiguous()                      # [L, Hq, D]
        out = torch.empty_like(qt)
        _ffi.check(_ffi.load().pie_sdpa_prefill(_ffi.p(qt), _ffi.p(k), _ffi.p(v), Hq, Hkv, L, total - L, cap, D, float(scale),
                                                _ffi.dtype_code(q.dtype), _ffi.p(out), _ffi.stream()))
        return out.transpose(0, 1).unsqueeze(0).contiguous()         # [1, Hq, L, D]
    if mask is not None and not (isinstance(mask, str) and mask == "causal"):  # one query row: the causal mask hides nothing
        raise NotImplementedError("decode form: one query position, mask=None")
    for t in (q, k, v):
        _dev(t)
    Hq, D = q.shape[1], q.shape[3]
    Hkv, cap = k.shape[1], k.shape[2]
    T = cap if T is None else int(T)
    key = (q.device, Hq, D)
    ws = _sdpa_ws.get(key)
    if ws is None:
        ws = torch.empty(_ffi.load().pie_sdpa_decode_workspace_bytes(Hq, D), dtype=torch.uint8, device=q.device)
        _sdpa_ws[key] = ws
    out = torch.empty_like(q)
    _ffi.check(_ffi.load().pie_sdpa_decode(_ffi.p(q), _ffi.p(k), _ffi.p(v), Hq, Hkv, T, cap, D, float(scale),
                                           _ffi.dtype_code(q.dtype), _ffi.p(out), _ffi.p(ws), _ffi.stream()))
    return out


def kv_quantize_rows(x: torch.Tensor, n: int, codes: torch.Tensor, scales: torch.Tensor, biases: torch.Tensor, group_size: int = 64,
                     bits: int = 8) -> None:
    """mx.quantize of the first n rows of every head of x [B, H, cap, D] (T) into the same rows of a quantized KV cache's
    codes [B, H, cap', D*bits/32] (uint32), scales / biases [B, H, cap', D/group_size] (T), bit-identical with mx.quantize."""
    for t in (x, codes, scales, biases):
        _dev(t)
    B, H, cap, D = x.shape
    dcap = codes.shape[2]
    if codes.shape != (B, H, dcap, D * bits // 32) or scales.shape != (B, H, dcap, D // group_size) or biases.shape != scales.shape:
        raise ValueError("kv_quantize_rows: codes / scales / biases do not match x, group_size and bits")
    if codes.element_size() != 4 or scales.dtype != x.dtype or biases.dtype != x.dtype:
        raise ValueError("kv_quantize_rows: codes must be 32-bit words, scales / biases of x's dtype")
    _ffi.check(_ffi.load().pie_kv_quantize(_ffi.p(x), B * H, int(n), cap, D, group_size, bits, _ffi.dtype_code(x.dtype), _ffi.p(codes),
                                           _ffi.p(scales), _ffi.p(biases), dcap, _ffi.stream()))


def kv_quantize(x: torch.Tensor, group_size: int = 64, bits: int = 8):
    """mx.quantize(x, group_size, bits) of K / V rows x [..., L, D] -> (codes uint32 [..., L, D*bits/32], scales, biases [..., L, D/group_size])."""
    _dev(x)
    *lead, L, D = x.shape
    if bits not in (4, 8) or group_size not in (32, 64, 128) or D % group_size:
        raise ValueError(f"kv_quantize: bits 4 / 8 and group_size 32 / 64 / 128 dividing the row ({D}) only; got bits={bits}, group_size={group_size}")
    x4 = x.reshape(1, -1, L, D)
    codes = torch.empty((*lead, L, D * bits // 32), dtype=torch.uint32, device=x.device)
    scales = torch.empty((*lead, L, D // group_size), dtype=x.dtype, device=x.device)
    biases = torch.empty_like(scales)
    kv_quantize_rows(x4, L, codes.reshape(1, -1, L, D * bits // 32), scales.reshape(1, -1, L, D // group_size),
                     biases.reshape(1, -1, L, D // group_size), group_size, bits)
    return codes, scales, biases


def attn_decode_quant(q: torch.Tensor, k: tuple, v: tuple, scale: float, group_size: int = 64, bits: int = 8, T: int | None = None) -> torch.Tensor:
    """quantized_scaled_dot_product_attention (models/base.py:56-89) for one query row: q [Hq, D] (or [1, Hq, 1, D]) T, k / v the
    (codes, scales, biases) triples of a QuantizedKVCache layer ([1, Hkv, cap, ...] or [Hkv, cap, ...]); the first T positions
    (default: all) are attended.  Returns the shape of q."""
    shape = q.shape
    q2 = q.reshape(-1, shape[-1])
    kk = [t.reshape(-1, t.shape[-2], t.shape[-1]) for t in k]
    vv = [t.reshape(-1, t.shape[-2], t.shape[-1]) for t in v]
    for t in (q2, *kk, *vv):
        _dev(t)
    Hq, D = q2.shape
    Hkv, cap = kk[0].shape[0], kk[0].shape[1]
    if bits not in (4, 8) or group_size not in (32, 64, 128) or D % group_size:
        raise ValueError(f"attn_decode_quant: bits 4 / 8 and group_size 32 / 64 / 128 dividing head_dim ({D}) only; got bits={bits}, group_size={group_size}")
    for trip, what in ((kk, "k"), (vv, "v")):
        c, sc, bi = trip
        if c.shape != (Hkv, cap, D * bits // 32) or sc.shape != (Hkv, cap, D // group_size) or bi.shape != sc.shape:
            raise ValueError(f"attn_decode_quant: {what} triple {[tuple(t.shape) for t in trip]} does not match {Hkv} kv-heads x {cap} positions, "
                             f"head_dim {D}, bits {bits}, group_size {group_size}")
        if c.element_size() != 4 or sc.dtype != q.dtype or bi.dtype != q.dtype:
            raise ValueError(f"attn_decode_quant: {what} codes must be 32-bit words, scales / biases of q's dtype")
    T = cap if T is None else int(T)
    key = (q.device, Hq, D)
    ws = _sdpa_ws.get(key)
    if ws is None:
        ws = torch.empty(_ffi.load().pie_sdpa_decode_workspace_bytes(Hq, D), dtype=torch.uint8, device=q.device)
        _sdpa_ws[key] = ws
    out = torch.empty_like(q2)
    _ffi.check(_ffi.load().pie_attn_decode_quant(_ffi.p(q2), *(_ffi.p(t) for t in kk), *(_ffi.p(t) for t in vv), Hq, Hkv, T, cap, D,
                                                 group_size, bits, float(scale), _ffi.dtype_code(q.dtype), _ffi.p(out), _ffi.p(ws), _ffi.stream()))
    return out.reshape(shape)


def paged_kv_append(k: torch.Tensor, v: torch.Tensor, slab: torch.Tensor, n_pages: int, block_table: torch.Tensor,
                    positions: torch.Tensor) -> None:
    """Stores the new K / V rows [B, Hkv, D] of B sequences in their pages (sequence s at positions[s]; < 0 = idle).
    slab: one layer's page slab (cache/kv_cache/paged.py); block_table int32 [B, max_blocks]; positions int32 [B]."""
    for t in (k, v, slab, block_table, positions):
        _dev(t)
    if block_table.dtype != torch.int32 or positions.dtype != torch.int32:
        raise TypeError("block_table and positions must be int32")
    B, Hkv, D = k.shape
    if v.shape != k.shape or block_table.shape[0] != B or positions.shape[0] != B:
        raise ValueError("paged_kv_append: k, v [B, Hkv, D]; block_table [B, max_blocks]; positions [B]")
    if slab.numel() * slab.element_size() < n_pages * 2 * 64 * Hkv * D * 2:
        raise ValueError("paged_kv_append: slab smaller than n_pages pages")
    _ffi.check(_ffi.load().pie_paged_kv_append(_ffi.p(k), _ffi.p(v), _ffi.p(slab), n_pages, _ffi.p(block_table), block_table.shape[1],
                                               _ffi.p(positions), B, Hkv, D, _ffi.dtype_code(k.dtype), _ffi.stream()))


def paged_attention_decode(q: torch.Tensor, slab: torch.Tensor, n_pages: int, block_table: torch.Tensor, context_lens: torch.Tensor,
                           n_kv_heads: int, scale: float) -> torch.Tensor:
    """One decode query per sequence against its paged KV: q [B, Hq, D]; block_table int32 [B, max_blocks];
    context_lens int32 [B] = positions attended including the current one (0 = idle slot -> zeros).  What the
    reference's Attention::invoke_paged_attention_kernel placeholder stands for (src/layers/attention.cpp:71-83)."""
    for t in (q, slab, block_table, context_lens):
        _dev(t)
    if block_table.dtype != torch.int32 or context_lens.dtype != torch.int32:
        raise TypeError("block_table and context_lens must be int32")
    B, Hq, D = q.shape
    if block_table.shape[0] != B or context_lens.shape[0] != B:
        raise ValueError("paged_attention_decode: block_table [B, max_blocks]; context_lens [B]")
    if slab.numel() * slab.element_size() < n_pages * 2 * 64 * n_kv_heads * D * 2:
        raise ValueError("paged_attention_decode: slab smaller than n_pages pages")
    key = ("paged", q.device, B, Hq, D)
    ws = _sdpa_ws.get(key)
    if ws is None:
        ws = torch.empty(_ffi.load().pie_paged_attn_workspace_bytes(B, Hq, D), dtype=torch.uint8, device=q.device)
        _sdpa_ws[key] = ws
    out = torch.empty_like(q)
    _ffi.check(_ffi.load().pie_paged_attn_decode(_ffi.p(q), _ffi.p(slab), n_pages, _ffi.p(block_table), block_table.shape[1],
                                                 _ffi.p(context_lens), B, Hq, n_kv_heads, D, float(scale), _ffi.dtype_code(q.dtype),
                                                 _ffi.p(out), _ffi.p(ws), _ffi.stream()))
    return out


def _i8_slab_check(slab: torch.Tensor, n_pages: int, Hkv: int, D: int, who: str) -> None:
    if slab.numel() * slab.element_size() < n_pages * _ffi.load().pie_page_i8_bytes(Hkv, D):
        raise ValueError(f"{who}: slab smaller than n_pages int8 pages")


def page_i8_set_scales(slab: torch.Tensor, n_pages: int, n_kv_heads: int, head_dim: int, k_scales: torch.Tensor | None,
                       v_scales: torch.Tensor | None, page_ids: torch.Tensor | None = None) -> None:
    """Writes the per-head fp16 scales of int8 pages (page.hpp:31-32: key_cache_scale_ / value_cache_scale_, [heads, 1]; None = ones, the
    reference constructor's value) into the pages `page_ids` (int32, device; None = all n_pages)."""
    _dev(slab)
    for t in (k_scales, v_scales):
        if t is not None:
            _dev(t)
            if t.dtype != torch.float16 or t.numel() != n_kv_heads:
                raise ValueError("page_i8_set_scales: scales are float16 [n_kv_heads]")
    if page_ids is not None and page_ids.dtype != torch.int32:
        raise TypeError("page_ids must be int32")
    _i8_slab_check(slab, n_pages, n_kv_heads, head_dim, "page_i8_set_scales")
    n = n_pages if page_ids is None else page_ids.numel()
    _ffi.check(_ffi.load().pie_page_i8_set_scales(_ffi.p(slab), n_pages, n_kv_heads, head_dim, _ffi.p(page_ids), n, _ffi.p(k_scales), _ffi.p(v_scales),
                                                  _ffi.stream()))


def paged_kv_append_i8(k: torch.Tensor, v: torch.Tensor, slab: torch.Tensor, n_pages: int, block_table: torch.Tensor, positions: torch.Tensor) -> None:
    """paged_kv_append onto int8 pages: each row is quantised with its page's per-head scale, q = clamp(rint(x / s), -127, 127)."""
    for t in (k, v, slab, block_table, positions):
        _dev(t)
    if block_table.dtype != torch.int32 or positions.dtype != torch.int32:
        raise TypeError("block_table and positions must be int32")
    B, Hkv, D = k.shape
    if v.shape != k.shape or block_table.shape[0] != B or positions.shape[0] != B:
        raise ValueError("paged_kv_append_i8: k, v [B, Hkv, D]; block_table [B, max_blocks]; positions [B]")
    _i8_slab_check(slab, n_pages, Hkv, D, "paged_kv_append_i8")
    _ffi.check(_ffi.load().pie_paged_kv_append_i8(_ffi.p(k), _ffi.p(v), _ffi.p(slab), n_pages, _ffi.p(block_table), block_table.shape[1],
                                                  _ffi.p(positions), B, Hkv, D, _ffi.dtype_code(k.dtype), _ffi.stream()))


def paged_attention_decode_i8(q: torch.Tensor, slab: torch.Tensor, n_pages: int, block_table: torch.Tensor, context_lens: torch.Tensor,
                              n_kv_heads: int, scale: float) -> torch.Tensor:
    """paged_attention_decode over int8 pages: K / V rows are read as fp32(q) * fp32(scale of the page's head), the rest in fp32."""
    for t in (q, slab, block_table, context_lens):
        _dev(t)
    if block_table.dtype != torch.int32 or context_lens.dtype != torch.int32:
        raise TypeError("block_table and context_lens must be int32")
    B, Hq, D = q.shape
    if block_table.shape[0] != B or context_lens.shape[0] != B:
        raise ValueError("paged_attention_decode_i8: block_table [B, max_blocks]; context_lens [B]")
    _i8_slab_check(slab, n_pages, n_kv_heads, D, "paged_attention_decode_i8")
    key = ("paged", q.device, B, Hq, D)
    ws = _sdpa_ws.get(key)
    if ws is None:
        ws = torch.empty(_ffi.load().pie_paged_attn_workspace_bytes(B, Hq, D), dtype=torch.uint8, device=q.device)
        _sdpa_ws[key] = ws
    out = torch.empty_like(q)
    _ffi.check(_ffi.load().pie_paged_attn_decode_i8(_ffi.p(q), _ffi.p(slab), n_pages, _ffi.p(block_table), block_table.shape[1],
                                                    _ffi.p(context_lens), B, Hq, n_kv_heads, D, float(scale), _ffi.dtype_code(q.dtype),
                                                    _ffi.p(out), _ffi.p(ws), _ffi.stream()))
    return out


def silu_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """nn.silu(a) * b (models/llama/language.py:127)."""
    _dev(a), _dev(b)
    y = torch.empty_like(a)
    _ffi.check(_ffi.load().pie_silu_mul(_ffi.p(a), _ffi.p(b), a.numel(), _ffi.dtype_code(a.dtype), _ffi.p(y), _ffi.stream()))
    return y


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _dev(a), _dev(b)
    y = torch.empty_like(a)
    _ffi.check(_ffi.load().pie_add(_ffi.p(a), _ffi.p(b), a.numel(), _ffi.dtype_code(a.dtype), _ffi.p(y), _ffi.stream()))
    return y


def logprobs_argmax(logits: torch.Tensor):
    """engine/inference_engine.py:268-271 + greedy sampler: returns (token int32 [1], logprobs fp32 [V])."""
    _dev(logits)
    logits = logits.reshape(-1)
    V = logits.numel()
    lp = torch.empty(V, dtype=torch.float32, device=logits.device)
    tok = torch.empty(1, dtype=torch.int32, device=logits.device)
    _ffi.check(_ffi.load().pie_logprobs_argmax(_ffi.p(logits), V, _ffi.dtype_code(logits.dtype), _ffi.p(lp), _ffi.p(tok),
                                               _ffi.stream()))
    return tok, lp


def logits_penalty(logits: torch.Tensor, ids: torch.Tensor, penalty: float) -> torch.Tensor:
    """The repetition penalty (logits_processors/repetition.py:11-22) on 16-bit logits [V], IN PLACE: every distinct id of `ids` (device
    int32, 1..1024 of them) once, x < 0 ? x * penalty : x / penalty in fp32, one rounding; ids outside [0, V) are skipped.  Returns logits."""
    _dev(logits), _dev(ids)
    if not logits.is_contiguous() or ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError("logits_penalty: contiguous logits and contiguous int32 ids")
    _ffi.check(_ffi.load().pie_logits_penalty(_ffi.p(logits), logits.numel(), _ffi.dtype_code(logits.dtype), _ffi.p(ids), ids.numel(), float(penalty),
                                              _ffi.stream()))
    return logits


def pack_token_mask(allowed, vocab_size: int) -> torch.Tensor:
    """The token mask of structured decoding as the kernels read it: HOST int32 [ceil(V / 32)], token i is allowed iff bit i & 31 of
    word i >> 5 is set (LSB first; bit 31 is the int32's sign).  allowed: a bool [V] tensor, or an iterable of token ids.  Host
    arithmetic; ValueError for ids outside [0, V), a bool tensor of another length and an empty set (an all-zero mask leaves no token)."""
    import numpy as np
    V = int(vocab_size)
    if V < 1:
        raise ValueError("pack_token_mask: vocab_size must be positive")
    if isinstance(allowed, torch.Tensor) and allowed.dtype == torch.bool:
        if allowed.numel() != V:
            raise ValueError(f"pack_token_mask: a bool mask needs {V} entries, got {allowed.numel()}")
        bits = allowed.detach().reshape(-1).cpu().numpy()
    else:
        ids = np.asarray(allowed.detach().cpu().numpy() if isinstance(allowed, torch.Tensor) else list(allowed), dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= V):
            raise ValueError(f"pack_token_mask: token ids must be in [0, {V})")
        bits = np.zeros(V, dtype=bool)
        bits[ids] = True
    if not bits.any():
        raise ValueError("pack_token_mask: no token is allowed")
    words = np.packbits(np.pad(bits, (0, -V % 32)), bitorder="little").view("<u4")
    return torch.from_numpy(words.astype(np.uint32).view(np.int32).copy())


def logprobs_argmax_masked(logits: torch.Tensor, mask_words: torch.Tensor):
    """logprobs_argmax with a token mask (pack_token_mask's layout, device int32 [>= ceil(V / 32)]): `logits` [V] are masked IN PLACE
    (-inf at every disallowed id, the others keep their bits), then (token int32 [1], logprobs fp32 [V]) are logprobs_argmax of them."""
    _dev(logits), _dev(mask_words)
    if not logits.is_contiguous() or mask_words.dtype != torch.int32 or mask_words.dim() != 1 or mask_words.stride(0) != 1:
        raise ValueError("logprobs_argmax_masked: contiguous logits and contiguous int32 mask words")
    V = logits.numel()
    lp = torch.empty(V, dtype=torch.float32, device=logits.device)
    tok = torch.empty(1, dtype=torch.int32, device=logits.device)
    _ffi.check(_ffi.load().pie_logprobs_argmax_masked(_ffi.p(logits), V, _ffi.dtype_code(logits.dtype), _ffi.p(mask_words), mask_words.numel(),
                                                      _ffi.p(lp), _ffi.p(tok), _ffi.stream()))
    return tok, lp


def logits_bias(logits: torch.Tensor, ids: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """logit_bias on 16-bit logits [V], IN PLACE: logits[ids[t]] = T(f32(logits[ids[t]]) + bias[t]) (one fp32 addition, one rounding) for
    every entry whose id is in [0, V) and not held by an earlier entry; ids device int32 [n], bias device float32 [n], 1 <= n <= 1024.
    Returns logits."""
    _dev(logits), _dev(ids), _dev(bias)
    if not logits.is_contiguous() or ids.dtype != torch.int32 or bias.dtype != torch.float32 or not ids.is_contiguous() or not bias.is_contiguous() or \
            ids.numel() != bias.numel():
        raise ValueError("logits_bias: contiguous logits, contiguous int32 ids and as many contiguous float32 biases")
    _ffi.check(_ffi.load().pie_logits_bias(_ffi.p(logits), logits.numel(), _ffi.dtype_code(logits.dtype), _ffi.p(ids), _ffi.p(bias), ids.numel(),
                                           _ffi.stream()))
    return logits


# ---------------------------------------------------------------- token automaton (include/pie_hip.h: pie_row_dfa)
DFA_WORDS = C.sizeof(_ffi.pie_row_dfa) // 4  # a record as int32 words: a device table is an int32 [rows, DFA_WORDS] tensor


def token_dfa_records(records, device=None) -> torch.Tensor:
    """Per-row automaton records as an int32 [rows, DFA_WORDS] tensor, on `device` when given.  An entry is (cls_off, trans_off, n_states,
    n_classes) -- word offsets into the arena and the table's shape -- or None: the all-zero record of an unarmed row."""
    rows = [(0, 0, 0, 0) if r is None else tuple(int(v) for v in r) for r in records]
    if not rows or any(len(r) != DFA_WORDS or any(not -2 ** 31 <= v < 2 ** 31 for v in r) for r in rows):
        raise ValueError("token_dfa_records: at least one entry, each None or (cls_off, trans_off, n_states, n_classes) of int32 values")
    t = torch.tensor(rows, dtype=torch.int32)
    return t if device is None else t.to(device)


def _dfa_rows(who: str, records: torch.Tensor, states: torch.Tensor, tables: torch.Tensor) -> int:
    for t in (records, states, tables):
        _dev(t)
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f"{who}: records, states and tables are contiguous int32 device tensors")
    rows = states.numel()
    if records.numel() != rows * DFA_WORDS:
        raise ValueError(f"{who}: records is int32 [rows, {DFA_WORDS}] (token_dfa_records) for states [rows]")
    return rows


def token_dfa_mask(records: torch.Tensor, states: torch.Tensor, tables: torch.Tensor, vocab_size: int, masks: torch.Tensor,
                   mask_on: torch.Tensor | None = None) -> torch.Tensor:
    """pie_token_dfa_mask: every armed row's token mask, derived from its state, into masks int32 [rows, words >= ceil(V / 32)] IN PLACE
    (pack_token_mask's layout); mask_on int32 [rows] gets 1 for a row that was written and 0 for an armed row whose state has left the
    automaton -- without mask_on such a row is written all-allowed.  An unarmed row is not touched.  Returns masks."""
    rows = _dfa_rows("token_dfa_mask", records, states, tables)
    _dev(masks)
    if masks.dtype != torch.int32 or not masks.is_contiguous() or masks.dim() != 2 or masks.shape[0] != rows:
        raise ValueError("token_dfa_mask: masks is a contiguous int32 [rows, words] device tensor")
    if mask_on is not None:
        _dev(mask_on)
        if mask_on.dtype != torch.int32 or not mask_on.is_contiguous() or mask_on.numel() != rows:
            raise ValueError("token_dfa_mask: mask_on is a contiguous int32 [rows] device tensor")
    _ffi.check(_ffi.load().pie_token_dfa_mask(_ffi.p(records), _ffi.p(states), _ffi.p(tables), tables.numel(), rows, int(vocab_size), _ffi.p(masks),
                                              masks.shape[1], _ffi.p(mask_on), _ffi.stream()))
    return masks


def token_dfa_advance(records: torch.Tensor, states: torch.Tensor, tables: torch.Tensor, vocab_size: int, tokens: torch.Tensor) -> torch.Tensor:
    """pie_token_dfa_advance: every armed row's state moves by tokens[row] (device int32 [rows]) IN PLACE: the table's next state, -1 for
    a token that is not allowed or not an id; a state outside the automaton stays what it is.  Returns states."""
    rows = _dfa_rows("token_dfa_advance", records, states, tables)
    _dev(tokens)
    if tokens.dtype != torch.int32 or not tokens.is_contiguous() or tokens.numel() != rows:
        raise ValueError("token_dfa_advance: tokens is a contiguous int32 [rows] device tensor")
    _ffi.check(_ffi.load().pie_token_dfa_advance(_ffi.p(records), _ffi.p(states), _ffi.p(tables), tables.numel(), rows, int(vocab_size), _ffi.p(tokens),
                                                 _ffi.stream()))
    return states


DFA_MAX_DRAFT = 31  # the ids a speculative pass verifies at most (SPEC_MAX_ROWS - 1)


def token_dfa_forced(automaton, device=None) -> torch.Tensor:
    """TokenAutomaton.forced() as the int32 [S, 2] tensor token_dfa_draft takes, on `device` when given."""
    t = torch.from_numpy(automaton.forced().copy())  # (the cached table is read-only)
    return t if device is None else t.to(device)


def _dfa_one(who: str, record: torch.Tensor, state: torch.Tensor, tables: torch.Tensor) -> None:
    if _dfa_rows(who, record, state, tables) != 1:
        raise ValueError(f"{who}: one record (int32 [1, {DFA_WORDS}]) and one state (int32 [1])")


def token_dfa_walk(record: torch.Tensor, state: torch.Tensor, tables: torch.Tensor, vocab_size: int, tokens: torch.Tensor,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """pie_token_dfa_walk: the automaton's states along tokens (device int32 [n], 1 <= n <= 31) from `state` (int32 [1], not modified) ->
    int32 [n + 1]: out[0] = the state, out[i + 1] = token_dfa_advance's result for out[i] and tokens[i].  A state outside the automaton
    stays what it is; an unarmed record copies the state to every slot.  out: at least n + 1 words to write into."""
    who = "token_dfa_walk"
    _dfa_one(who, record, state, tables)
    _dev(tokens)
    n = tokens.numel()
    if tokens.dtype != torch.int32 or not tokens.is_contiguous() or not 1 <= n <= DFA_MAX_DRAFT:
        raise ValueError(f"{who}: tokens is a contiguous int32 device tensor of 1..{DFA_MAX_DRAFT} ids")
    if out is None:
        out = torch.empty(n + 1, dtype=torch.int32, device=tokens.device)
    _dev(out)
    if out.dtype != torch.int32 or not out.is_contiguous() or out.numel() < n + 1:
        raise ValueError(f"{who}: out is a contiguous int32 device tensor of at least n + 1 words")
    _ffi.check(_ffi.load().pie_token_dfa_walk(_ffi.p(record), _ffi.p(state), _ffi.p(tables), tables.numel(), int(vocab_size), _ffi.p(tokens), n, _ffi.p(out),
                                              _ffi.stream()))
    return out[:n + 1]


def token_dfa_draft(record: torch.Tensor, state: torch.Tensor, tables: torch.Tensor, forced: torch.Tensor, vocab_size: int, cand: torch.Tensor,
                    cand_count: torch.Tensor, k: int, out: tuple | None = None):
    """pie_token_dfa_draft, the grammar-aware drafter: forced int32 [S', 2] (token_dfa_forced; a hint, re-derived from the
    tables), cand int32 [>= 31] a candidate draft and cand_count int32 [1] its length (clamped to 0..31 on the device), k in 1..31 ->
    (draft int32 [k], count int32 [1]), no host sync: the candidate cut at the first id the grammar forbids, with every forced id put in
    (a forced id that differs from the candidate ends the candidate's part); an unarmed record or a state outside the automaton passes
    the candidate through.  out = (draft, count) to write into -- they may be (cand, cand_count) -- else fresh tensors of -1 and 0."""
    who = "token_dfa_draft"
    _dfa_one(who, record, state, tables)
    _dev(forced)
    if forced.dtype != torch.int32 or not forced.is_contiguous() or forced.dim() != 2 or forced.shape[1] != 2 or forced.shape[0] < 1:
        raise ValueError(f"{who}: forced is a contiguous int32 [states, 2] device tensor (token_dfa_forced)")
    if not 1 <= int(k) <= DFA_MAX_DRAFT:
        raise ValueError(f"{who}: 1 <= k <= {DFA_MAX_DRAFT}")
    _dev(cand), _dev(cand_count)
    if cand.dtype != torch.int32 or not cand.is_contiguous() or cand.numel() < DFA_MAX_DRAFT or cand_count.dtype != torch.int32 or cand_count.numel() != 1:
        raise ValueError(f"{who}: cand is a contiguous int32 device tensor of at least {DFA_MAX_DRAFT} ids and cand_count int32 [1]")
    if out is None:
        out = (torch.full((int(k),), -1, dtype=torch.int32, device=cand.device), torch.zeros(1, dtype=torch.int32, device=cand.device))
    draft, count = out
    _dev(draft), _dev(count)
    if draft.dtype != torch.int32 or not draft.is_contiguous() or draft.numel() < int(k) or count.dtype != torch.int32 or count.numel() != 1:
        raise ValueError(f"{who}: out is (int32 [>= k], int32 [1]) on the device")
    _ffi.check(_ffi.load().pie_token_dfa_draft(_ffi.p(record), _ffi.p(state), _ffi.p(tables), tables.numel(), _ffi.p(forced), forced.shape[0], int(vocab_size),
                                               _ffi.p(cand), _ffi.p(cand_count), int(k), _ffi.p(draft), _ffi.p(count), _ffi.stream()))
    return draft, count


def qkv_row_map(n_heads: int, n_kv_heads: int, head_dim: int) -> torch.Tensor:
    n = (n_heads + 2 * n_kv_heads) * head_dim
    arr = (C.c_int32 * n)()
    _ffi.check(_ffi.load().pie_qkv_row_map(n_heads, n_kv_heads, head_dim, arr))
    return torch.tensor(list(arr), dtype=torch.int32)


def gateup_row_map(inter: int) -> torch.Tensor:
    arr = (C.c_int32 * (2 * inter))()
    _ffi.check(_ffi.load().pie_gateup_row_map(inter, arr))
    return torch.tensor(list(arr), dtype=torch.int32)


# ---------------------------------------------------------------------------- vision tower ops
class PackedLinear:
    """An nn.Linear weight [N, K] (16-bit) as W16M tiles: 32 output rows x 64 columns in MFMA operand order, zero-padded
    (csrc/w16_gemm.hpp) -- what the hand-written 16-bit GEMM streams straight into its fragment registers.  Built once per matrix."""

    def __init__(self, weight: torch.Tensor):
        _dev(weight)
        if weight.dim() != 2 or weight.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("PackedLinear: weight [N, K] in bfloat16 or float16")
        weight = weight.contiguous()
        self.N, self.K = (int(v) for v in weight.shape)
        self.shape = (self.N, self.K)  # of the Linear's weight
        self.dtype = weight.dtype
        lib = _ffi.load()
        self.tiles = torch.empty(int(lib.pie_w16m_bytes(self.N, self.K)), dtype=torch.uint8, device=weight.device)
        _ffi.check(lib.pie_repack_w16m(_ffi.p(weight), self.N, self.K, _ffi.dtype_code(weight.dtype), _ffi.p(self.tiles), _ffi.stream()))


def pack_linear(weight: torch.Tensor) -> PackedLinear:
    return PackedLinear(weight)


def interleave_gate_up(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    """Rows (or entries) of gate_proj and up_proj interleaved (gate_0, up_0, gate_1, ...): the order linear_rows(..., swiglu=True) wants."""
    return torch.stack((gate, up), dim=1).reshape(2 * gate.shape[0], *gate.shape[1:]).contiguous()


def linear_rows(x: torch.Tensor, weight, bias: torch.Tensor | None = None, *, swiglu: bool = False, pad_to: int = 0) -> torch.Tensor:
    """nn.Linear on a block of rows: x [M, K] @ weight [N, K].T (+ bias [N]) -> [M, N]; dense 16-bit weights on the hand-written MFMA GEMM
    (fp32 accumulation; models/intern/vision.py:150-151,192-194,129-133; PatchEmbed's Conv3d with stride = kernel is the same product
    over flattened patches, vision.py:97-121).  weight: a PackedLinear (pack_linear: once per matrix), or the plain [N, K] tensor (packed
    on the spot).  x may carry 64 * ceil(K / 64) columns, zeros past K; with just K columns and K % 64 != 0 it is padded here.
    swiglu: weight rows (and bias) interleave gate and up (interleave_gate_up): returns silu(gate) * up [M, N / 2] (MLP, vision.py:196-197),
    bias and activation in the GEMM's epilogue.  pad_to: the output rows are zero-padded to a multiple of it (the next GEMM's operand)."""
    _dev(x)
    pk = weight if isinstance(weight, PackedLinear) else PackedLinear(weight)
    N, K = pk.N, pk.K
    Kx = -(-K // 64) * 64
    if x.dim() != 2 or x.shape[1] not in (K, Kx) or x.dtype != pk.dtype:
        raise ValueError("linear_rows: x [M, K] (or zero-padded to a multiple of 64 columns), weight [N, K] of one dtype")
    if bias is not None and (bias.shape != (N,) or bias.dtype != x.dtype):
        raise ValueError("linear_rows: bias must be [N] in the activation dtype")
    if swiglu and N % 8:
        raise ValueError("linear_rows: swiglu needs N % 8 == 0 (interleaved gate | up rows)")
    if x.shape[1] != Kx:
        x = torch.nn.functional.pad(x, (0, Kx - K))
    if x.stride(1) != 1 or x.stride(0) % 8 or x.stride(0) < Kx:
        x = x.contiguous()
    M = x.shape[0]
    cols = N // 2 if swiglu else N
    ldy = -(-cols // pad_to) * pad_to if pad_to else cols
    y = (torch.zeros if ldy != cols else torch.empty)((M, ldy), dtype=x.dtype, device=x.device)
    lib = _ffi.load()
    wsb = 0 if swiglu else int(lib.pie_linear_w16m_workspace(M, N, K))
    if wsb and ldy != cols:
        raise ValueError("linear_rows: pad_to is not available for shapes that split K")
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device) if wsb else None
    _ffi.check(lib.pie_linear_w16m(_ffi.p(x), x.stride(0), _ffi.p(pk.tiles), _ffi.p(bias.contiguous() if bias is not None else None), M, N, K,
                                   _ffi.dtype_code(x.dtype), _ffi.p(y), ldy, int(swiglu), _ffi.p(ws), wsb, _ffi.stream()))
    return y


def gelu(x: torch.Tensor) -> torch.Tensor:
    """nn.GELU() (exact erf form; PatchMerger, vision.py:130)."""
    _dev(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    _ffi.check(_ffi.load().pie_gelu(_ffi.p(x), x.numel(), _ffi.dtype_code(x.dtype), _ffi.p(y), _ffi.stream()))
    return y


def vision_qkv_rope(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, num_heads: int, padded_head_dim: int | None = None,
                    bias: torch.Tensor | None = None):
    """qkv [N, 3 * H * D] (the qkv Linear's output, vision.py:152-156) -> (q [N, H, DP], k [H, N, DP], v [H, N, DP]) with
    apply_rotary_pos_emb_vision (vision.py:55-70) on q and k; cos / sin fp32 [N, D/2]; head dims D..DP-1 are zero.
    bias [3 * H * D]: the qkv Linear's bias when the GEMM was run without it (added here, same values)."""
    _dev(qkv), _dev(cos), _dev(sin)
    N = qkv.shape[0]
    D = qkv.shape[1] // (3 * num_heads)
    if qkv.dim() != 2 or qkv.shape[1] != 3 * num_heads * D or D % 2:
        raise ValueError("vision_qkv_rope: qkv must be [N, 3 * H * D] with even D")
    DP = padded_head_dim or (64 if D <= 64 else 128)
    if cos.shape != (N, D // 2) or sin.shape != (N, D // 2) or cos.dtype != torch.float32 or sin.dtype != torch.float32:
        raise ValueError("vision_qkv_rope: cos / sin must be float32 [N, D/2]")
    q = torch.empty((N, num_heads, DP), dtype=qkv.dtype, device=qkv.device)
    k = torch.empty((num_heads, N, DP), dtype=qkv.dtype, device=qkv.device)
    v = torch.empty((num_heads, N, DP), dtype=qkv.dtype, device=qkv.device)
    if bias is not None and (bias.shape != (qkv.shape[1],) or bias.dtype != qkv.dtype):
        raise ValueError("vision_qkv_rope: bias must be [3 * H * D] in the activation dtype")
    _ffi.check(_ffi.load().pie_vision_qkv_rope(_ffi.p(qkv.contiguous()), _ffi.p(bias.contiguous() if bias is not None else None), _ffi.p(cos.contiguous()), _ffi.p(sin.contiguous()), N, num_heads, D, DP,
                                               _ffi.dtype_code(qkv.dtype), _ffi.p(q), _ffi.p(k), _ffi.p(v), _ffi.stream()))
    return q, k, v


def segment_bounds(cu_seqlens, device) -> tuple[torch.Tensor, torch.Tensor]:
    """cu_seqlens (host ints, [0, ..., N]) -> per-row key ranges (seg_lo, seg_hi) int32 [N] on the device: the 0 blocks of the
    additive mask vision.py:160-167 builds."""
    import numpy as np
    cu = np.asarray([int(c) for c in cu_seqlens], dtype=np.int64)
    if cu.size < 2 or cu[0] != 0 or np.any(np.diff(cu) < 0):
        raise ValueError("cu_seqlens must start at 0 and be non-decreasing")
    lens = np.diff(cu)
    lo = np.repeat(cu[:-1], lens).astype(np.int32)
    hi = np.repeat(cu[1:], lens).astype(np.int32)
    return torch.from_numpy(lo).to(device), torch.from_numpy(hi).to(device)


def sdpa_segments(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, seg_lo: torch.Tensor, seg_hi: torch.Tensor, scale: float) -> torch.Tensor:
    """mx.fast.scaled_dot_product_attention with the block-diagonal mask of vision.py:160-176: q [N, H, D], k / v [H, N, D]
    (D = 64 or 128), row r attends keys [seg_lo[r], seg_hi[r]) -> [N, H, D]."""
    for t in (q, k, v, seg_lo, seg_hi):
        _dev(t)
    N, H, D = q.shape
    if k.shape != (H, N, D) or v.shape != (H, N, D) or seg_lo.shape != (N,) or seg_hi.shape != (N,):
        raise ValueError("sdpa_segments: q [N, H, D]; k, v [H, N, D]; seg_lo, seg_hi [N]")
    if seg_lo.dtype != torch.int32 or seg_hi.dtype != torch.int32:
        raise TypeError("segment bounds must be int32")
    out = torch.empty_like(q)
    _ffi.check(_ffi.load().pie_sdpa_segments(_ffi.p(q.contiguous()), _ffi.p(k.contiguous()), _ffi.p(v.contiguous()), _ffi.p(seg_lo), _ffi.p(seg_hi),
                                             N, H, D, float(scale), _ffi.dtype_code(q.dtype), _ffi.p(out), _ffi.stream()))
    return out


def bias_silu_mul(gate: torch.Tensor, up: torch.Tensor, bias_gate: torch.Tensor, bias_up: torch.Tensor) -> torch.Tensor:
    """silu(gate + bias_gate) * (up + bias_up) on [M, N] GEMM outputs (MLP of vision.py:196-197, biases folded in).  gate and up
    may be the two column halves of one [M, 2N] GEMM output (equal row strides, unit column stride)."""
    _dev(bias_gate), _dev(bias_up)
    if not (gate.is_cuda and up.is_cuda):
        raise ValueError("pie_hip ops take device tensors (ROCm); got a CPU tensor")
    M, N = gate.shape
    if up.shape != (M, N) or bias_gate.shape != (N,) or bias_up.shape != (N,):
        raise ValueError("bias_silu_mul: gate, up [M, N]; biases [N]")
    if gate.stride(1) != 1 or up.stride(1) != 1 or gate.stride(0) != up.stride(0):
        gate, up = gate.contiguous(), up.contiguous()
    y = torch.empty((M, N), dtype=gate.dtype, device=gate.device)
    _ffi.check(_ffi.load().pie_bias_silu_mul(_ffi.p(gate), _ffi.p(up), _ffi.p(bias_gate.contiguous()), _ffi.p(bias_up.contiguous()),
                                             M, N, gate.stride(0) if M > 1 else N, _ffi.dtype_code(gate.dtype), _ffi.p(y), _ffi.stream()))
    return y


def add_bias(x: torch.Tensor, r: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """x + (r + bias) on [M, N] (residual add with the preceding Linear's bias folded in, vision.py:212-218)."""
    for t in (x, r, bias):
        _dev(t)
    M, N = x.shape
    if r.shape != (M, N) or bias.shape != (N,):
        raise ValueError("add_bias: x, r [M, N]; bias [N]")
    y = torch.empty_like(x)
    _ffi.check(_ffi.load().pie_add_bias(_ffi.p(x.contiguous()), _ffi.p(r.contiguous()), _ffi.p(bias.contiguous()), M, N, _ffi.dtype_code(x.dtype),
                                        _ffi.p(y), _ffi.stream()))
    return y


def add_bias_rms_norm(x: torch.Tensor, r: torch.Tensor, bias: torch.Tensor, norm_weight: torch.Tensor, eps: float):
    """(y, rms_norm(y)) with y = x + (r + bias): the residual add and the norm after it in one pass over the rows."""
    for t in (x, r, bias, norm_weight):
        _dev(t)
    M, N = x.shape
    if r.shape != (M, N) or bias.shape != (N,) or norm_weight.shape != (N,):
        raise ValueError("add_bias_rms_norm: x, r [M, N]; bias, norm_weight [N]")
    y, xn = torch.empty_like(x), torch.empty_like(x)
    _ffi.check(_ffi.load().pie_add_bias_rms_norm(_ffi.p(x.contiguous()), _ffi.p(r.contiguous()), _ffi.p(bias.contiguous()), _ffi.p(norm_weight.contiguous()),
                                                 float(eps), M, N, _ffi.dtype_code(x.dtype), _ffi.p(y), _ffi.p(xn), _ffi.stream()))
    return y, xn


def quantized_matmul_rows(x: torch.Tensor, w: PackedWeight, w4m: torch.Tensor | None = None) -> torch.Tensor:
    """mx.quantized_matmul in its many-row regime -- weights dequantised to T, T x T products on the MFMA units, fp32
    accumulation -- reading the int4 weights in 4-bit form.  pie_qgemm_w4m goes through the library's one many-row int4 entry (w4_rows_launch,
    w4m_gemm.hip), as a plain store without bias: the weight-streaming k_w4r_gemm wherever it serves (up to 256 rows, K of at least 256, 128 beyond
    64 rows), else the few-row kernel up to 32 rows and the tile kernels beyond; a K-split shape is reduced inside the call.  Unlike the decoder, this call
    does not follow knob small_m (the w4r knob does apply), so that tests can reach each kernel by its row count.  x [M, K]; w: the W4S matrix (N % 32 == 0); w4m: its W4M tile copy from `repack_w4m` (built here when absent)."""
    _dev(x)
    if w.fmt != _ffi.PIE_W_INT4_G64:
        raise TypeError("quantized_matmul_rows takes an int4 group-64 weight")
    M, K = x.shape
    if K != w.K or M < 1 or w.N % 32:
        raise ValueError("quantized_matmul_rows: x [M, K], N % 32 == 0")
    if w4m is None:
        w4m = repack_w4m(w)
    y = torch.empty((M, w.N), dtype=x.dtype, device=x.device)
    _ffi.check(_ffi.load().pie_qgemm_w4m(_ffi.p(x.contiguous()), _ffi.p(w4m), M, w.N, K, _ffi.dtype_code(x.dtype), _ffi.p(y), _ffi.stream()))
    if w.lin_bias is not None:
        y = add(y, w.lin_bias.expand_as(y).contiguous())
    return y


def repack_w4m(w: PackedWeight) -> torch.Tensor:
    """W4S stream -> W4M tiles (32 rows x 64 columns, MFMA operand order; include/pie_hip.h), same bytes per weight."""
    lib = _ffi.load()
    n = lib.pie_w4m_bytes(w.N, w.K)
    if n == 0:
        raise ValueError("repack_w4m: N must be a multiple of 32 and K of 64")
    out = torch.empty(n, dtype=torch.uint8, device=w.packed.device)
    _ffi.check(lib.pie_repack_w4s_to_w4m(_ffi.p(w.packed), w.N, w.K, _ffi.p(out), _ffi.stream()))
    return out


SAMPLE_MODES = {"categorical": 0, "top_k": 1, "top_p": 2, "min_p": 3}


# ---------------------------------------------------------------- XTC (include/pie_hip.h: pie_xtc)
XTC_SPECIAL_MAX = _ffi.PIE_XTC_SPECIAL_MAX
XTC_WORDS = C.sizeof(_ffi.pie_xtc) // 4   # a record as int32 words: a device table is an int32 [rows, XTC_WORDS] tensor
XTC_PROBABILITY_WORD = 1                  # the fp32 `probability` of a record, as a word index (an engine rewrites it between replays)


def xtc_pack(probability: float = 0.0, threshold: float = 0.1, special=()) -> _ffi.pie_xtc:
    """One XTC record (pie_xtc_pack) in host memory: probability in [0, 1] (0: off), threshold in (0, 0.5], at most 16 special token ids
    that are never removed.  ValueError outside the ABI's rules.  Needs no device."""
    ids = [int(i) for i in special]
    if len(ids) > XTC_SPECIAL_MAX or any(not -2 ** 31 <= i < 2 ** 31 for i in ids):
        raise ValueError(f"xtc_pack: at most {XTC_SPECIAL_MAX} special tokens, each an int32 token id")
    rec = _ffi.pie_xtc()
    arr = (C.c_int32 * max(len(ids), 1))(*ids)
    _ffi.check(_ffi.load().pie_xtc_pack(float(probability), float(threshold), C.cast(arr, C.c_void_p), len(ids), C.byref(rec)))
    return rec


def xtc_records(records, device=None) -> torch.Tensor:
    """Records (xtc_pack) as an int32 [rows, XTC_WORDS] tensor, on `device` when given."""
    import numpy as np
    host = np.frombuffer(b"".join(bytes(r) for r in records), dtype=np.int32).reshape(len(records), XTC_WORDS).copy()
    t = torch.from_numpy(host)
    return t if device is None else t.to(device)


def _xtc(xtc, rows: int, device, who: str) -> torch.Tensor:
    """xtc as a device int32 [>= rows, XTC_WORDS] tensor: a host record (xtc_pack) is uploaded, a device tensor is checked."""
    if isinstance(xtc, _ffi.pie_xtc):
        return xtc_records([xtc] * rows, device)
    _dev(xtc)
    if xtc.dtype != torch.int32 or not xtc.is_contiguous() or xtc.numel() < rows * XTC_WORDS or xtc.numel() % XTC_WORDS:
        raise ValueError(f"{who}: xtc is a record (xtc_pack) or a contiguous int32 [>= rows, {XTC_WORDS}] device tensor (xtc_records)")
    return xtc


def sample(logprobs: torch.Tensor, mode: str, temp: float, p: float = 0.0, k: int = 0, want_mask: bool = False, xtc=None,
           want_removed: bool = False, rng: tuple | None = None):
    """The stochastic branches of make_sampler (samplers/__init__.py:39-46) as ONE HIP kernel (pie_sample): logprobs fp32 [rows, V] or [V]
    on the GPU -> token ids int32 [rows] on the same device, no host sync.  want_mask: also return (kept_count int32 [rows], kept uint8
    [rows, V]) -- the filter's kept set, for tests.  xtc: one record shared by the rows (xtc_pack, or its device form) -- the draw is
    pie_sample_xtc's; want_removed: the int32 [rows] count of ids XTC removed joins the result as its last member.  rng = (seed,
    counter int64 [2] device): another stream than the samplers' own (samplers._rng), e.g. a draft model's."""
    from .samplers import _rng
    x = logprobs
    if not x.is_cuda:
        raise ValueError("the samplers take device tensors (ROCm): there is no host path; got a CPU tensor")
    if x.dim() == 1:
        x = x[None]
    if x.dtype != torch.float32:
        x = x.float()
    x = x.contiguous()
    rows, V = x.shape
    lib = _ffi.load()
    if int(lib.pie_sample_workspace_bytes(rows, V)) == 0:  # V > 524288 (1024 workgroups of 512 ids) or an empty block: refused, nothing launched
        raise ValueError(f"sample: a [rows, V] block with rows >= 1 and 1 <= V <= 524288, got [{rows}, {V}]")
    seed, counter = _rng.hip_state(x.device) if rng is None else rng
    ws = sample_workspace(x.device, rows, V)
    tokens = torch.empty(rows, dtype=torch.int32, device=x.device)
    kept = torch.empty(rows, dtype=torch.int32, device=x.device) if want_mask else None
    mask = torch.empty((rows, V), dtype=torch.uint8, device=x.device) if want_mask else None
    if xtc is None and not want_removed:
        _ffi.check(lib.pie_sample(_ffi.p(x), rows, V, SAMPLE_MODES[mode], float(temp), float(p), int(k), seed, _ffi.p(counter), _ffi.p(ws), _ffi.p(tokens),
                                  _ffi.p(kept) if want_mask else None, _ffi.p(mask) if want_mask else None, _ffi.stream()))
        return (tokens, kept, mask) if want_mask else tokens
    rec = None if xtc is None else _xtc(xtc, 1, x.device, "sample")
    removed = torch.zeros(rows, dtype=torch.int32, device=x.device) if want_removed else None
    _ffi.check(lib.pie_sample_xtc(_ffi.p(x), rows, V, SAMPLE_MODES[mode], float(temp), float(p), int(k), seed, _ffi.p(counter), _ffi.p(ws), _ffi.p(tokens),
                                  _ffi.p(kept), _ffi.p(mask), _ffi.p(rec), _ffi.p(removed), _ffi.stream()))
    out = (tokens, kept, mask) if want_mask else (tokens,)
    out = out + (removed,) if want_removed else out
    return out if len(out) > 1 else tokens


_sample_ws: dict = {}


def sample_workspace(device, rows: int, V: int) -> torch.Tensor:
    """pie_sample's workspace for a [rows, V] block on `device`: zeroed once, the kernels leave it ready for the next call.  The decode
    step's tail (Model.set_step_tail) draws through the same one, in stream order with sample()."""
    key = (str(device), rows, V)
    ws = _sample_ws.get(key)
    if ws is None:
        if len(_sample_ws) > 8:
            _sample_ws.clear()
        ws = _sample_ws[key] = torch.zeros(int(_ffi.load().pie_sample_workspace_bytes(rows, V)) // 8, dtype=torch.int64, device=device)
    return ws


# ---------------------------------------------------------------- per-row tails (include/pie_hip.h: pie_row_tail)
ROW_TAIL_WORDS = C.sizeof(_ffi.pie_row_tail) // 8   # a record as int64 words: a device table is an int64 [rows, ROW_TAIL_WORDS] tensor
RECENT_IDS = 1024                                    # ring positions per row


def row_tail_pack(mode: str | None = None, temp: float = 1.0, p: float = 0.0, k: int = 0, seed: int = 0, calls: int = 0, penalty: float = 1.0,
                  context_size: int = 60) -> _ffi.pie_row_tail:
    """One row's record (pie_row_tail_pack) in host memory: mode None = greedy, else one of SAMPLE_MODES with hip_ops.sample's arguments;
    seed / calls: the row's own random stream and how many tokens it has drawn; penalty (1.0: none) over the last context_size fed ids.
    ValueError for whatever pie_sample / pie_logits_penalty refuse.  Needs no device."""
    rec = _ffi.pie_row_tail()
    code = _ffi.PIE_SAMPLE_GREEDY if mode is None else SAMPLE_MODES[mode]
    _ffi.check(_ffi.load().pie_row_tail_pack(code, float(temp), float(p), int(k), int(seed) & (2 ** 64 - 1), int(calls), float(penalty), int(context_size),
                                             C.byref(rec)))
    return rec


def row_tail_table(records, device=None) -> torch.Tensor:
    """Records (row_tail_pack) as an int64 [rows, ROW_TAIL_WORDS] tensor, on `device` when given."""
    import numpy as np
    host = np.frombuffer(b"".join(bytes(r) for r in records), dtype=np.int64).reshape(len(records), ROW_TAIL_WORDS).copy()
    t = torch.from_numpy(host)
    return t if device is None else t.to(device)


def _table(table: torch.Tensor, rows: int, who: str) -> None:
    _dev(table)
    if table.dtype != torch.int64 or not table.is_contiguous() or table.dim() != 2 or table.shape[1] != ROW_TAIL_WORDS or table.shape[0] < rows:
        raise ValueError(f"{who}: the table is a contiguous int64 [>= rows, {ROW_TAIL_WORDS}] device tensor (row_tail_table)")


def sample_rows(logprobs: torch.Tensor, table: torch.Tensor, tokens: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
                want_mask: bool = False, xtc: torch.Tensor | None = None, want_removed: bool = False):
    """pie_sample_rows: row r of logprobs fp32 [rows, V] drawn with table[r]'s own sampler, seed and call counter (advanced on the device);
    greedy rows keep tokens[r] as given (zeros when tokens is None).  Returns tokens int32 [rows], with want_mask also (kept_count, kept
    uint8 [rows, V]) -- rows of greedy records are left unwritten.  xtc: int32 [>= rows, XTC_WORDS] device records (xtc_records), row r's
    for row r -- the draw is pie_sample_rows_xtc's; want_removed: the int32 [rows] counts of removed ids join the result last."""
    x = logprobs
    _dev(x)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("sample_rows: contiguous fp32 [rows, V] log-probabilities")
    rows, V = x.shape
    _table(table, rows, "sample_rows")
    lib = _ffi.load()
    if int(lib.pie_sample_workspace_bytes(rows, V)) == 0:
        raise ValueError(f"sample_rows: a [rows, V] block with rows >= 1 and 1 <= V <= 524288, got [{rows}, {V}]")
    ws = sample_workspace(x.device, rows, V) if workspace is None else workspace
    if tokens is None:
        tokens = torch.zeros(rows, dtype=torch.int32, device=x.device)
    kept = torch.zeros(rows, dtype=torch.int32, device=x.device) if want_mask else None
    mask = torch.zeros((rows, V), dtype=torch.uint8, device=x.device) if want_mask else None
    if xtc is None and not want_removed:
        _ffi.check(lib.pie_sample_rows(_ffi.p(x), rows, V, _ffi.p(table), _ffi.p(ws), _ffi.p(tokens), _ffi.p(kept), _ffi.p(mask), _ffi.stream()))
        return (tokens, kept, mask) if want_mask else tokens
    if isinstance(xtc, _ffi.pie_xtc):
        raise ValueError("sample_rows: xtc is a device table of one record per row (xtc_records)")
    rec = None if xtc is None else _xtc(xtc, rows, x.device, "sample_rows")
    removed = torch.zeros(rows, dtype=torch.int32, device=x.device) if want_removed else None
    _ffi.check(lib.pie_sample_rows_xtc(_ffi.p(x), rows, V, _ffi.p(table), _ffi.p(ws), _ffi.p(tokens), _ffi.p(kept), _ffi.p(mask), _ffi.p(rec),
                                       _ffi.p(removed), _ffi.stream()))
    out = (tokens, kept, mask) if want_mask else (tokens,)
    out = out + (removed,) if want_removed else out
    return out if len(out) > 1 else tokens


def logits_penalty_rows(logits: torch.Tensor, table: torch.Tensor, recent_ids: torch.Tensor, ids: torch.Tensor, ctx: torch.Tensor,
                        out_rows: torch.Tensor | None = None) -> torch.Tensor:
    """pie_logits_penalty_rows on 16-bit logits [rows, V], IN PLACE: row s with source row i = out_rows[s] (or s) records ids[i] at
    recent_ids[s][(ctx[i] - 1) & 1023] and is penalised over its last table[s].context_size fed ids.  recent_ids int32 [rows, 1024];
    ids / ctx (/ out_rows) int32 device tensors.  Returns logits."""
    _dev(logits), _dev(recent_ids)
    if logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError("logits_penalty_rows: contiguous [rows, V] logits")
    rows, V = logits.shape
    _table(table, rows, "logits_penalty_rows")
    for t in (recent_ids, ids, ctx) + ((out_rows,) if out_rows is not None else ()):
        _dev(t)
        if t.dtype != torch.int32:
            raise ValueError("logits_penalty_rows: contiguous int32 index tensors")
    if recent_ids.shape != (recent_ids.shape[0], RECENT_IDS) or recent_ids.shape[0] < rows or ids.numel() != ctx.numel() or \
            (out_rows is not None and out_rows.numel() != rows):
        raise ValueError("logits_penalty_rows: recent_ids [>= rows, 1024], ids and ctx of one length, out_rows [rows]")
    _ffi.check(_ffi.load().pie_logits_penalty_rows(_ffi.p(logits), rows, V, _ffi.dtype_code(logits.dtype), _ffi.p(table), _ffi.p(recent_ids), _ffi.p(ids),
                                                   _ffi.p(ctx), _ffi.p(out_rows), ids.numel(), _ffi.stream()))
    return logits


# ---------------------------------------------------------------- per-row token masks and logit biases
def logprobs_argmax_rows_masked(logits: torch.Tensor, masks: torch.Tensor, mask_on: torch.Tensor):
    """pie_logprobs_argmax_rows_masked: row r of 16-bit logits [rows, V] is masked IN PLACE with masks[r] (pack_token_mask's layout, device
    int32 [rows, >= ceil(V / 32)]) when mask_on[r] (device int32 [rows]) is nonzero and left bit for bit otherwise; returns (tokens int32
    [rows], logprobs fp32 [rows, V]) -- every row what logprobs_argmax_masked (armed) or logprobs_argmax (off) gives that row alone."""
    _dev(logits), _dev(masks), _dev(mask_on)
    if logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError("logprobs_argmax_rows_masked: contiguous [rows, V] logits")
    rows, V = logits.shape
    if masks.dtype != torch.int32 or masks.dim() != 2 or not masks.is_contiguous() or masks.shape[0] < rows or \
            mask_on.dtype != torch.int32 or not mask_on.is_contiguous() or mask_on.numel() < rows:
        raise ValueError("logprobs_argmax_rows_masked: contiguous int32 masks [>= rows, words] and mask_on [>= rows]")
    lp = torch.empty((rows, V), dtype=torch.float32, device=logits.device)
    tok = torch.empty(rows, dtype=torch.int32, device=logits.device)
    _ffi.check(_ffi.load().pie_logprobs_argmax_rows_masked(_ffi.p(logits), rows, V, _ffi.dtype_code(logits.dtype), _ffi.p(masks), masks.shape[1],
                                                           _ffi.p(mask_on), _ffi.p(lp), _ffi.p(tok), _ffi.stream()))
    return tok, lp


def logits_bias_rows(logits: torch.Tensor, ids: torch.Tensor, bias: torch.Tensor, n: torch.Tensor) -> torch.Tensor:
    """pie_logits_bias_rows on 16-bit logits [rows, V], IN PLACE: row r takes the first n[r] entries (clamped to [0, cap]) of ids[r] / bias[r]
    (device int32 / float32 [rows, cap], cap 1..1024) under logits_bias's rule; n device int32 [rows], 0: the row keeps every bit.
    Returns logits."""
    _dev(logits), _dev(ids), _dev(bias), _dev(n)
    if logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError("logits_bias_rows: contiguous [rows, V] logits")
    rows, V = logits.shape
    if ids.dtype != torch.int32 or bias.dtype != torch.float32 or n.dtype != torch.int32 or ids.dim() != 2 or ids.shape != bias.shape or \
            not (ids.is_contiguous() and bias.is_contiguous() and n.is_contiguous()) or ids.shape[0] < rows or n.numel() < rows:
        raise ValueError("logits_bias_rows: contiguous int32 ids and float32 bias [>= rows, cap], int32 n [>= rows]")
    _ffi.check(_ffi.load().pie_logits_bias_rows(_ffi.p(logits), rows, V, _ffi.dtype_code(logits.dtype), _ffi.p(ids), _ffi.p(bias), _ffi.p(n),
                                                ids.shape[1], _ffi.stream()))
    return logits


# ---------------------------------------------------------------- frequency and presence penalties (include/pie_hip.h: pie_count_penalty)
COUNT_PENALTY_WORDS = C.sizeof(_ffi.pie_count_penalty) // 4   # a record as int32 words: a device table is an int32 [rows, COUNT_PENALTY_WORDS] tensor
COUNT_PENALTY_RANGE = (-2.0, 2.0)                             # what the Python layers accept for either penalty (the OpenAI range)


def check_count_penalties(frequency_penalty, presence_penalty, who: str) -> tuple[float, float]:
    """(frequency_penalty, presence_penalty) as floats, each within -2.0 .. 2.0: ValueError otherwise (NaN included)."""
    lo, hi = COUNT_PENALTY_RANGE
    f, p = float(frequency_penalty), float(presence_penalty)
    if not (lo <= f <= hi and lo <= p <= hi):
        raise ValueError(f"{who}: frequency_penalty and presence_penalty must lie in {lo} .. {hi}, got {frequency_penalty!r} and {presence_penalty!r}")
    return f, p


def count_penalty_pack(freq: float = 0.0, pres: float = 0.0, start: int = 0, counted_pos: int | None = None) -> _ffi.pie_count_penalty:
    """One row's record (pie_count_penalty_pack) in host memory: the two penalties (any finite value: the ABI's rule), `start` = the first
    position that holds a generated token (the prompt's length), counted_pos = the last position already counted (None: start - 1, nothing
    counted yet).  ValueError for NaN, inf or a negative start.  Needs no device."""
    rec = _ffi.pie_count_penalty()
    _ffi.check(_ffi.load().pie_count_penalty_pack(float(freq), float(pres), int(start), int(start) - 1 if counted_pos is None else int(counted_pos),
                                                  C.byref(rec)))
    return rec


def count_penalty_records(records, device=None) -> torch.Tensor:
    """Records (count_penalty_pack) as an int32 [rows, COUNT_PENALTY_WORDS] tensor, on `device` when given."""
    import numpy as np
    host = np.frombuffer(b"".join(bytes(r) for r in records), dtype=np.int32).reshape(len(records), COUNT_PENALTY_WORDS).copy()
    t = torch.from_numpy(host)
    return t if device is None else t.to(device)


def logits_count_penalty_rows(logits: torch.Tensor, records: torch.Tensor, counts: torch.Tensor, ids: torch.Tensor | None = None,
                              ctx: torch.Tensor | None = None, out_rows: torch.Tensor | None = None) -> torch.Tensor:
    """pie_logits_count_penalty_rows on 16-bit logits [rows, V], IN PLACE: row s with source row i = out_rows[s] (or s) first counts its
    input id ids[i] at position ctx[i] - 1 (once per position, from records[s].start on; `counts` and the record's counted_pos are
    updated), then logits[s, v] -= freq * counts[s, v] + pres wherever counts[s, v] > 0 (fp32, one rounding).  records int32 [>= rows,
    COUNT_PENALTY_WORDS] (count_penalty_records), counts int32 [>= rows, V]; ids / ctx (/ out_rows) int32 device tensors, or all None: every
    row is live and nothing is counted.  Returns logits."""
    _dev(logits), _dev(records), _dev(counts)
    if logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError("logits_count_penalty_rows: contiguous [rows, V] logits")
    rows, V = logits.shape
    if records.dtype != torch.int32 or not records.is_contiguous() or records.dim() != 2 or records.shape[1] != COUNT_PENALTY_WORDS or records.shape[0] < rows:
        raise ValueError(f"logits_count_penalty_rows: the records are a contiguous int32 [>= rows, {COUNT_PENALTY_WORDS}] device tensor (count_penalty_records)")
    if counts.dtype != torch.int32 or not counts.is_contiguous() or counts.dim() != 2 or counts.shape[1] != V or counts.shape[0] < rows:
        raise ValueError("logits_count_penalty_rows: the counts are a contiguous int32 [>= rows, V] device tensor")
    if (ids is None) != (ctx is None) or (ctx is None and out_rows is not None):
        raise ValueError("logits_count_penalty_rows: ids and ctx come together (out_rows only with them)")
    for t in (ids, ctx, out_rows):
        if t is not None:
            _dev(t)
            if t.dtype != torch.int32 or not t.is_contiguous():
                raise ValueError("logits_count_penalty_rows: contiguous int32 index tensors")
    if ids is not None and (ids.numel() != ctx.numel() or ids.numel() < 1 or (out_rows is None and ids.numel() < rows) or
                            (out_rows is not None and out_rows.numel() != rows)):
        raise ValueError("logits_count_penalty_rows: ids and ctx of one length (>= rows without out_rows), out_rows [rows]")
    _ffi.check(_ffi.load().pie_logits_count_penalty_rows(_ffi.p(logits), rows, V, _ffi.dtype_code(logits.dtype), _ffi.p(records), _ffi.p(counts), _ffi.p(ids),
                                                         _ffi.p(ctx), _ffi.p(out_rows), 0 if ids is None else ids.numel(), _ffi.stream()))
    return logits


# ---------------------------------------------------------------- DRY penalty (include/pie_hip.h: pie_dry_penalty)
DRY_MAX_MATCH = 64        # PIE_DRY_MAX_MATCH
DRY_BREAKERS_MAX = 64     # PIE_DRY_BREAKERS_MAX
DRY_PENALTY_WORDS = C.sizeof(_ffi.pie_dry_penalty) // 4   # a record as int32 words: a device table is an int32 [rows, DRY_PENALTY_WORDS] tensor


def check_dry(multiplier, base=1.75, allowed_length=2, range=1024, breakers=(), who: str = "dry") -> tuple[float, float, int, int, tuple]:
    """(multiplier, base, allowed_length, range, breaker ids) under the ABI's rules: multiplier finite and >= 0, base finite and > 0 (both
    as fp32), allowed_length 1..64, range 1..1024, at most 64 breaker ids, each an int32: ValueError otherwise (NaN included)."""
    import math
    m, b = float(multiplier), float(base)
    big = float(torch.finfo(torch.float32).max)
    if not (math.isfinite(m) and 0.0 <= m <= big):
        raise ValueError(f"{who}: the multiplier must be finite and >= 0, got {multiplier!r}")
    if not (math.isfinite(b) and 0.0 < b <= big and float(torch.tensor(b, dtype=torch.float32)) > 0.0):
        raise ValueError(f"{who}: the base must be finite and > 0, got {base!r}")
    for name, v, hi in (("allowed_length", allowed_length, DRY_MAX_MATCH), ("range", range, RECENT_IDS)):
        if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= hi:
            raise ValueError(f"{who}: {name} must be an integer in 1 .. {hi}, got {v!r}")
    ids = tuple(int(i) for i in breakers)
    if len(ids) > DRY_BREAKERS_MAX or any(not -2 ** 31 <= i < 2 ** 31 for i in ids):
        raise ValueError(f"{who}: at most {DRY_BREAKERS_MAX} sequence breakers, each an int32 token id")
    return m, b, int(allowed_length), int(range), ids


def dry_penalty_pack(multiplier: float = 0.0, base: float = 1.75, allowed_length: int = 2, range: int = 1024, n_breakers: int = 0) -> _ffi.pie_dry_penalty:
    """One row's record (pie_dry_penalty_pack) in host memory; the default is the zero record (multiplier 0: the row keeps every bit).
    ValueError outside the ABI's rules.  Needs no device."""
    rec = _ffi.pie_dry_penalty()
    _ffi.check(_ffi.load().pie_dry_penalty_pack(float(multiplier), float(base), int(allowed_length), int(range), int(n_breakers), C.byref(rec)))
    return rec


def dry_penalty_records(records, device=None) -> torch.Tensor:
    """Records (dry_penalty_pack) as an int32 [rows, DRY_PENALTY_WORDS] tensor, on `device` when given."""
    import numpy as np
    host = np.frombuffer(b"".join(bytes(r) for r in records), dtype=np.int32).reshape(len(records), DRY_PENALTY_WORDS).copy()
    t = torch.from_numpy(host)
    return t if device is None else t.to(device)


def dry_breaker_table(breakers, device=None) -> torch.Tensor:
    """One row's breaker ids as an int32 [DRY_BREAKERS_MAX] tensor (unused entries 0: the record's n_breakers bounds the reads)."""
    row = torch.zeros(DRY_BREAKERS_MAX, dtype=torch.int32)
    if len(breakers):
        row[:len(breakers)] = torch.tensor(list(breakers), dtype=torch.int32)
    return row if device is None else row.to(device)


def logits_dry_penalty(logits: torch.Tensor, ids: torch.Tensor, multiplier: float, base: float = 1.75, allowed_length: int = 2,
                       breakers=()) -> torch.Tensor:
    """pie_logits_dry_penalty on one 16-bit logit vector [V] (or [1, V]), IN PLACE: the window is ids (int32 device tensor, 1..1024 entries,
    the last one the input id; the range is its length), breakers a sequence or int32 device tensor of at most 64 ids.  Returns logits."""
    _dev(logits), _dev(ids)
    if not logits.is_contiguous() or logits.numel() != logits.shape[-1]:
        raise ValueError("logits_dry_penalty: one contiguous logit vector")
    if ids.dtype != torch.int32 or not ids.is_contiguous() or not 1 <= ids.numel() <= RECENT_IDS:
        raise ValueError("logits_dry_penalty: 1..1024 contiguous int32 ids")
    if not isinstance(breakers, torch.Tensor):
        m, b, a, _, br = check_dry(multiplier, base, allowed_length, ids.numel(), breakers, "logits_dry_penalty")
        breakers = torch.tensor(br, dtype=torch.int32, device=logits.device) if br else None
    else:
        _dev(breakers)
        if breakers.dtype != torch.int32 or not breakers.is_contiguous():
            raise ValueError("logits_dry_penalty: contiguous int32 breakers")
        m, b, a = float(multiplier), float(base), int(allowed_length)
    nb = 0 if breakers is None else breakers.numel()
    _ffi.check(_ffi.load().pie_logits_dry_penalty(_ffi.p(logits), logits.shape[-1], _ffi.dtype_code(logits.dtype), _ffi.p(ids), ids.numel(), m, b, a,
                                                  _ffi.p(breakers), nb, _ffi.stream()))
    return logits


def logits_dry_penalty_rows(logits: torch.Tensor, records: torch.Tensor, breakers: torch.Tensor, recent_ids: torch.Tensor, ids: torch.Tensor,
                            ctx: torch.Tensor, out_rows: torch.Tensor | None = None) -> torch.Tensor:
    """pie_logits_dry_penalty_rows on 16-bit logits [rows, V], IN PLACE: row s with source row i = out_rows[s] (or s) records ids[i] at
    recent_ids[s][(ctx[i] - 1) & 1023] and is penalised under records[s] / breakers[s] over its last records[s].range fed ids.  records
    int32 [>= rows, DRY_PENALTY_WORDS] (dry_penalty_records), breakers int32 [>= rows, 64], recent_ids int32 [>= rows, 1024]; ids / ctx
    (/ out_rows) int32 device tensors.  Returns logits."""
    _dev(logits)
    if logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError("logits_dry_penalty_rows: contiguous [rows, V] logits")
    rows, V = logits.shape
    for t in (records, breakers, recent_ids, ids, ctx) + ((out_rows,) if out_rows is not None else ()):
        _dev(t)
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError("logits_dry_penalty_rows: contiguous int32 records, breakers, rings and index tensors")
    if records.dim() != 2 or records.shape[1] != DRY_PENALTY_WORDS or records.shape[0] < rows or breakers.dim() != 2 or \
            breakers.shape[1] != DRY_BREAKERS_MAX or breakers.shape[0] < rows or recent_ids.dim() != 2 or recent_ids.shape[1] != RECENT_IDS or \
            recent_ids.shape[0] < rows:
        raise ValueError(f"logits_dry_penalty_rows: records [>= rows, {DRY_PENALTY_WORDS}], breakers [>= rows, 64], recent_ids [>= rows, 1024]")
    if ids.numel() != ctx.numel() or ids.numel() < 1 or (out_rows is None and ids.numel() < rows) or (out_rows is not None and out_rows.numel() != rows):
        raise ValueError("logits_dry_penalty_rows: ids and ctx of one length (>= rows without out_rows), out_rows [rows]")
    _ffi.check(_ffi.load().pie_logits_dry_penalty_rows(_ffi.p(logits), rows, V, _ffi.dtype_code(logits.dtype), _ffi.p(records), _ffi.p(breakers),
                                                       _ffi.p(recent_ids), _ffi.p(ids), _ffi.p(ctx), _ffi.p(out_rows), ids.numel(), _ffi.stream()))
    return logits


# ---------------------------------------------------------------- top-n log-probabilities (csrc/top_logprobs.hip)
TOP_LOGPROBS_MAX = _ffi.PIE_TOP_LOGPROBS_MAX


def top_logprobs_workspace(device, rows: int, V: int, n: int) -> torch.Tensor:
    """pie_top_logprobs' workspace for a [rows, V] block and `n` pairs on `device`: uninitialised, nothing is carried from call to call."""
    nbytes = int(_ffi.load().pie_top_logprobs_workspace_bytes(int(rows), int(V), int(n)))
    if nbytes == 0:
        raise ValueError(f"top_logprobs: rows >= 1, 1 <= V <= 524288 and 1 <= n <= {TOP_LOGPROBS_MAX}, got rows = {rows}, V = {V}, n = {n}")
    return torch.empty(nbytes // 8, dtype=torch.int64, device=device)


def top_logprobs(logprobs: torch.Tensor, n: int, tokens: torch.Tensor | None = None, count: torch.Tensor | None = None,
                 workspace: torch.Tensor | None = None, out: tuple | None = None):
    """get_top_logprobs (engine/utils.py:4-48) on the device (pie_top_logprobs): logprobs fp32 [rows, V] or [V] -> (ids int32 [rows, n + 1],
    vals fp32 [rows, n + 1]), no sort and no host sync.  Slot 0 is (tokens[r], its log-probability), or (-1, -inf) without tokens or for an
    id outside [0, V); slots 1.. are the best min(c, V) ids by (value descending, id ascending) -- ties to the lowest id -- with bit copies
    of their values, then (-1, -inf); c = count[r] where count (device int32 [rows]) is given, else n: c > n acts as n, c == 0 leaves slot 0
    only, c < 0 leaves the row's record as it is -- out = (ids, vals) to write into, else fresh tensors of (-1, -inf).  n 1..20."""
    x = logprobs
    _dev(x)
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("top_logprobs: contiguous fp32 [rows, V] log-probabilities")
    rows, V = x.shape
    for t, name in ((tokens, "tokens"), (count, "count")):
        if t is not None:
            _dev(t)
            if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != rows:
                raise ValueError(f"top_logprobs: {name} is a contiguous int32 [rows] device tensor")
    ws = top_logprobs_workspace(x.device, rows, V, n) if workspace is None else workspace
    if out is None:
        out = (torch.full((rows, int(n) + 1), -1, dtype=torch.int32, device=x.device),
               torch.full((rows, int(n) + 1), float("-inf"), dtype=torch.float32, device=x.device))
    ids, vals = out
    for t, dt in ((ids, torch.int32), (vals, torch.float32)):
        _dev(t)
        if t.dtype != dt or tuple(t.shape) != (rows, int(n) + 1):
            raise ValueError("top_logprobs: out is (int32 [rows, n + 1], fp32 [rows, n + 1])")
    _ffi.check(_ffi.load().pie_top_logprobs(_ffi.p(x), rows, V, int(n), _ffi.p(tokens), _ffi.p(count), _ffi.p(ids), _ffi.p(vals), _ffi.p(ws), _ffi.stream()))
    return ids, vals


# ---------------------------------------------------------------- log-probabilities of prompt tokens (csrc/prompt_logprobs.hip)
def prompt_logprobs_workspace(device, rows: int, V: int, n: int) -> torch.Tensor:
    """pie_prompt_logprobs' workspace for a [rows, V] block and `n` pairs on `device`: uninitialised, nothing is carried from call to call."""
    nbytes = int(_ffi.load().pie_prompt_logprobs_workspace_bytes(int(rows), int(V), int(n)))
    if nbytes == 0:
        raise ValueError(f"prompt_logprobs: 1 <= rows <= 65535, 1 <= V <= 524288 and 1 <= n <= {TOP_LOGPROBS_MAX}, got rows = {rows}, V = {V}, n = {n}")
    return torch.empty(nbytes // 8, dtype=torch.int64, device=device)


def prompt_logprobs(logits: torch.Tensor, n: int, targets: torch.Tensor | None = None, count: torch.Tensor | None = None,
                    workspace: torch.Tensor | None = None, out: tuple | None = None):
    """The records of `top_logprobs` straight from 16-bit logits (pie_prompt_logprobs): logits bf16 / f16 [rows, V] or [V] -> (ids int32
    [rows, n + 1], vals fp32 [rows, n + 1]), bit for bit top_logprobs(logprobs_argmax(row)) of every row, with no fp32 row in between.
    Slot 0 is (targets[r], its log-probability), or (-1, -inf) without targets or for an id outside [0, V); the other slots, `count`,
    `workspace` and `out` are top_logprobs'.  n 1..20."""
    x = logits
    _dev(x)
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or x.dtype not in (torch.bfloat16, torch.float16) or not x.is_contiguous():
        raise ValueError("prompt_logprobs: contiguous bf16 / f16 [rows, V] logits")
    rows, V = x.shape
    for t, name in ((targets, "targets"), (count, "count")):
        if t is not None:
            _dev(t)
            if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != rows:
                raise ValueError(f"prompt_logprobs: {name} is a contiguous int32 [rows] device tensor")
    ws = prompt_logprobs_workspace(x.device, rows, V, n) if workspace is None else workspace
    if out is None:
        out = (torch.full((rows, int(n) + 1), -1, dtype=torch.int32, device=x.device),
               torch.full((rows, int(n) + 1), float("-inf"), dtype=torch.float32, device=x.device))
    ids, vals = out
    for t, dt in ((ids, torch.int32), (vals, torch.float32)):
        _dev(t)
        if t.dtype != dt or tuple(t.shape) != (rows, int(n) + 1):
            raise ValueError("prompt_logprobs: out is (int32 [rows, n + 1], fp32 [rows, n + 1])")
    _ffi.check(_ffi.load().pie_prompt_logprobs(_ffi.p(x), rows, V, _ffi.dtype_code(x.dtype), int(n), _ffi.p(targets), _ffi.p(count), _ffi.p(ids), _ffi.p(vals),
                                               _ffi.p(ws), _ffi.stream()))
    return ids, vals


# ---------------------------------------------------------------- greedy speculative decoding (csrc/speculative.hip)
SPEC_MAX_ROWS, SPEC_MAX_NGRAM = 32, 8


def _int32_dev(t: torch.Tensor, n: int | None, who: str, name: str) -> None:
    _dev(t)
    if t.dtype != torch.int32 or not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError(f"{who}: {name} is a contiguous int32 device tensor" + ("" if n is None else f" of {n}"))


def _workspace(size_fn: str, zeroed: bool, who: str, hint: str, device, *dims) -> torch.Tensor:
    """A 16-byte aligned workspace of the library's size function `size_fn` over `dims`, zeroed or uninitialised; a size of 0 (the
    library refuses the dims) is `who`'s ValueError with `hint`."""
    nbytes = int(getattr(_ffi.load(), size_fn)(*(int(d) for d in dims)))
    if nbytes == 0:
        raise ValueError(f"{who}: {hint}")
    return (torch.zeros if zeroed else torch.empty)((nbytes + 15) // 16 * 2, dtype=torch.int64, device=device)


def _fp32_block(t: torch.Tensor, shape: tuple, who: str, name: str, dims: str) -> None:
    _dev(t)
    if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"{who}: {name} is a contiguous fp32 [{dims}] device tensor")


def _spec_block(who: str, logits: torch.Tensor, draft: torch.Tensor, logprobs: torch.Tensor | None, out: tuple | None, need_logprobs: bool):
    """A one-sequence verify's block, validated: logits bf16 / f16 [rows, V], draft int32 [rows - 1], logprobs fp32 [rows, V] (made here
    when the verify needs them and none are given), out = (tokens int32 [rows], n int32 [1]) or fresh ones -> (rows, V, tokens, n, logprobs)."""
    _dev(logits)
    if logits.dim() != 2 or logits.dtype not in (torch.bfloat16, torch.float16) or not logits.is_contiguous():
        raise ValueError(f"{who}: contiguous bf16 / f16 [rows, V] logits")
    rows, V = logits.shape
    _int32_dev(draft, rows - 1, who, "draft")
    if logprobs is None and need_logprobs:
        logprobs = torch.empty((rows, V), dtype=torch.float32, device=logits.device)
    if logprobs is not None:
        _fp32_block(logprobs, (rows, V), who, "logprobs", "rows, V")
    if out is None:
        out = (torch.empty(rows, dtype=torch.int32, device=logits.device), torch.empty(1, dtype=torch.int32, device=logits.device))
    tokens, n = out
    _int32_dev(tokens, rows, who, "out[0]"), _int32_dev(n, 1, who, "out[1]")
    return rows, V, tokens, n, logprobs


def ngram_draft_workspace(device) -> torch.Tensor:
    """pie_ngram_draft's workspace on `device`: uninitialised, nothing is carried from call to call."""
    return torch.empty(int(_ffi.load().pie_ngram_draft_workspace_bytes()) // 4, dtype=torch.int32, device=device)


def ngram_draft(ids: torch.Tensor, length: torch.Tensor, ngram_max: int, ngram_min: int, k: int, workspace: torch.Tensor | None = None,
                out: tuple | None = None):
    """The prompt-lookup drafter (pie_ngram_draft): ids int32 [cap] = the sequence so far (the last id the token about to be fed), length
    device int32 [1], read on the device and clamped to [0, cap] -> (draft int32 [k], count int32 [1]), no host sync.  The suffix
    ids[len - n : len] of the largest n in ngram_max .. ngram_min that occurs earlier (ending at len - 1 at the latest) is looked up at its
    LATEST occurrence, and the k ids behind it are copied, the copy running on into its own output (a period-3 tail drafts k ids);
    count = k, or 0 without a match -- out = (draft, count) to write into (a draft without a match keeps its contents), else fresh
    tensors of -1 and 0.  1 <= ngram_min <= ngram_max <= 8, 1 <= k <= 31."""
    who = "ngram_draft"
    _int32_dev(ids, None, who, "ids"), _int32_dev(length, 1, who, "length")
    if ids.numel() < 1:
        raise ValueError("ngram_draft: ids holds at least one id")
    ws = ngram_draft_workspace(ids.device) if workspace is None else workspace
    if out is None:
        out = (torch.full((max(int(k), 1),), -1, dtype=torch.int32, device=ids.device), torch.zeros(1, dtype=torch.int32, device=ids.device))
    draft, count = out
    _int32_dev(draft, None, who, "out[0]"), _int32_dev(count, 1, who, "out[1]"), _int32_dev(ws, None, who, "workspace")
    if draft.numel() < int(k) or ws.numel() * 4 < int(_ffi.load().pie_ngram_draft_workspace_bytes()):
        raise ValueError("ngram_draft: out[0] holds k ids and the workspace ngram_draft_workspace()'s size")
    _ffi.check(_ffi.load().pie_ngram_draft(_ffi.p(ids), _ffi.p(length), ids.numel(), int(ngram_max), int(ngram_min), int(k), _ffi.p(draft), _ffi.p(count),
                                           _ffi.p(ws), _ffi.stream()))
    return draft, count


def spec_verify_workspace(device, rows: int) -> torch.Tensor:
    """pie_spec_verify's workspace for `rows` rows on `device`: uninitialised, nothing is carried from call to call."""
    return _workspace("pie_spec_verify_workspace_bytes", False, "spec_verify", f"2 <= rows <= {SPEC_MAX_ROWS}, got {rows}", device, rows)


def spec_verify(logits: torch.Tensor, draft: torch.Tensor, logprobs: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
                out: tuple | None = None):
    """The verify of a speculative pass (pie_spec_verify): logits bf16 / f16 [rows, V] (row 0 the fed token's, row i the i-th draft's),
    draft int32 [rows - 1] -> (tokens int32 [rows], n int32 [1]), no host sync: the drafts are accepted while draft[i] equals row i's
    greedy token (hip_ops.logprobs_argmax of that row, bit for bit; an id outside [0, V) is never accepted), n = accepted + 1, tokens =
    the greedy tokens of rows 0 .. n - 1, then -1.  logprobs: fp32 [rows, V] to write rows 0 .. n - 1 into (logprobs_argmax's bits); the
    rows behind them keep their contents.  out = (tokens, n) to write into.  rows 2..32."""
    rows, V, tokens, n, logprobs = _spec_block("spec_verify", logits, draft, logprobs, out, False)
    ws = spec_verify_workspace(logits.device, rows) if workspace is None else workspace
    _ffi.check(_ffi.load().pie_spec_verify(_ffi.p(logits), rows, V, _ffi.dtype_code(logits.dtype), _ffi.p(draft), _ffi.p(tokens), _ffi.p(n), _ffi.p(logprobs),
                                           _ffi.p(ws), _ffi.stream()))
    return tokens, n


def spec_verify_sampled_workspace(device, rows: int, V: int) -> torch.Tensor:
    """pie_spec_verify_sampled's workspace for a [rows, V] block on `device`: zeroed once, the kernels leave it ready for the next call."""
    return _workspace("pie_spec_verify_sampled_workspace_bytes", True, "spec_verify_sampled", f"2 <= rows <= {SPEC_MAX_ROWS} and 1 <= V <= 524288, got [{rows}, {V}]",
                      device, rows, V)


def spec_verify_sampled(logits: torch.Tensor, draft: torch.Tensor, mode: str, temp: float, p: float = 0.0, k: int = 0, xtc=None,
                        logprobs: torch.Tensor | None = None, workspace: torch.Tensor | None = None, out: tuple | None = None):
    """The verify of a speculative pass under a stochastic sampler (pie_spec_verify_sampled): logits bf16 / f16 [rows, V],
    draft int32 [rows - 1], (mode, temp, p, k) as `sample` takes them -> (tokens int32 [rows], n int32 [1], logprobs fp32 [rows, V]), no
    host sync.  With c = the samplers' stream position (read on the device), row r's token is `sample`'s of that row alone at position
    c + r; the drafts are accepted while draft[i] equals row i's token (an id outside [0, V) is never accepted), n = accepted + 1, tokens =
    the tokens of rows 0 .. n - 1, then -1, and the stream position becomes c + n.  Every row of logprobs is written
    (logprobs_argmax's bits).  xtc: one record shared by the rows (xtc_pack, or its device form).  workspace:
    spec_verify_sampled_workspace's (zeroed once); out = (tokens, n) to write into.  rows 2..32."""
    from .samplers import _rng
    who = "spec_verify_sampled"
    if mode not in SAMPLE_MODES:
        raise ValueError(f"{who}: mode is one of {sorted(SAMPLE_MODES)} (the greedy verify is spec_verify)")
    rows, V, tokens, n, logprobs = _spec_block(who, logits, draft, logprobs, out, True)
    ws = spec_verify_sampled_workspace(logits.device, rows, V) if workspace is None else workspace
    seed, counter = _rng.hip_state(logits.device)
    rec = None if xtc is None else _xtc(xtc, 1, logits.device, who)
    _ffi.check(_ffi.load().pie_spec_verify_sampled(_ffi.p(logits), rows, V, _ffi.dtype_code(logits.dtype), _ffi.p(draft), SAMPLE_MODES[mode], float(temp), float(p),
                                                   int(k), seed, _ffi.p(counter), _ffi.p(rec), _ffi.p(tokens), _ffi.p(n), _ffi.p(logprobs), _ffi.p(ws),
                                                   _ffi.stream()))
    return tokens, n, logprobs


def spec_verify_draft_workspace(device, rows: int, V: int) -> torch.Tensor:
    """pie_spec_verify_draft's workspace for a [rows, V] block on `device`: zeroed once, the kernels leave it ready for the next call."""
    return _workspace("pie_spec_verify_draft_workspace_bytes", True, "spec_verify_draft", f"2 <= rows <= {SPEC_MAX_ROWS} and 1 <= V <= 524288, got [{rows}, {V}]",
                      device, rows, V)


def spec_verify_draft(logits: torch.Tensor, draft: torch.Tensor, q_logprobs: torch.Tensor, mode: str, temp: float, p: float = 0.0, k: int = 0,
                      logprobs: torch.Tensor | None = None, workspace: torch.Tensor | None = None, out: tuple | None = None,
                      want_record: bool = False, rng: tuple | None = None):
    """The verify of a block a draft MODEL proposed (pie_spec_verify_draft) -- speculative sampling: logits bf16 / f16
    [rows, V] (row 0 the fed token's, row i the i-th draft's), draft int32 [rows - 1], q_logprobs fp32 [rows - 1, V] = the drafter's
    log-probabilities at the step that drew draft[i], (mode, temp, p, k) as `sample` takes them, shared by both sides -> (tokens int32
    [rows], n int32 [1], logprobs fp32 [rows, V]), no host sync.  With P_r / Q_i the rows' distributions under the sampler's own kept
    sets and c the target stream's position (read on the device), draft i is accepted iff it lies in [0, V), Q_i(d) > 0 and
    u_i * Q_i(d) < P_i(d); behind the accepted prefix comes one token more -- `sample("categorical", 1.0)` over the residual
    log(max(0, P_j - Q_j)) at position c + j after a refusal (the row's ordinary draw when the residual is empty), the ordinary draw of
    the last row at c + rows - 1 when every draft was accepted -- then -1, n = accepted + 1, and the stream position becomes c + n.
    want_record: (accept_rec fp32 [rows - 1, 3] = (P_i(d_i), Q_i(d_i), u_i), residual fp32 [rows, V], rows 0 .. rows - 2 written) join
    the result, for tests.  rng = (seed, counter int64 [2] device): the target's stream, the samplers' own by default -- the drafter must
    have drawn under ANOTHER seed.  workspace: spec_verify_draft_workspace's (zeroed once); out = (tokens, n) to write into.  rows 2..32."""
    from .samplers import _rng
    who = "spec_verify_draft"
    if mode not in SAMPLE_MODES:
        raise ValueError(f"{who}: mode is one of {sorted(SAMPLE_MODES)} (a greedy draft is verified by spec_verify)")
    rows, V, tokens, n, logprobs = _spec_block(who, logits, draft, logprobs, out, True)
    _fp32_block(q_logprobs, (rows - 1, V), who, "q_logprobs", "rows - 1, V")
    ws = spec_verify_draft_workspace(logits.device, rows, V) if workspace is None else workspace
    seed, counter = _rng.hip_state(logits.device) if rng is None else rng
    rec = torch.zeros((rows - 1, 3), dtype=torch.float32, device=logits.device) if want_record else None
    res = torch.zeros((rows, V), dtype=torch.float32, device=logits.device) if want_record else None
    _ffi.check(_ffi.load().pie_spec_verify_draft(_ffi.p(logits), rows, V, _ffi.dtype_code(logits.dtype), _ffi.p(draft), _ffi.p(q_logprobs), SAMPLE_MODES[mode],
                                                 float(temp), float(p), int(k), int(seed), _ffi.p(counter), _ffi.p(tokens), _ffi.p(n), _ffi.p(logprobs), _ffi.p(rec),
                                                 _ffi.p(res), _ffi.p(ws), _ffi.stream()))
    return (tokens, n, logprobs, rec, res) if want_record else (tokens, n, logprobs)


# ---------------------------------------------------------------- rotating KV cache (csrc/rotating.hip, prefill.hip)
def kv_ring_order(keys: torch.Tensor, values: torch.Tensor, keep: int, n: int, shift: int, n_dst: int) -> None:
    """In place on RotatingKVCache buffers [1, H, cap, D]: rows keep + j <- rows keep + (j + shift) % n for j < n_dst."""
    for t in (keys, values):
        _dev(t)
        if t.dim() != 4 or t.shape[0] != 1 or not t.is_contiguous():
            raise ValueError("kv_ring_order: contiguous [1, H, cap, D] buffers")
    _, H, cap, D = keys.shape
    scratch = torch.empty((2, H, max(n_dst, 1), D), dtype=keys.dtype, device=keys.device)
    _ffi.check(_ffi.load().pie_kv_ring_order(_ffi.p(keys), _ffi.p(values), H, cap, D, keep, n, shift, n_dst, _ffi.p(scratch), _ffi.stream()))


def sdpa_prefill_window(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, offset: int, window: int) -> torch.Tensor:
    """Windowed causal prompt attention: q [1, Hq, L, D], k / v [1, Hkv, cap, D] with the L new rows at offset .. offset + L - 1;
    query i sees rows offset + i - window .. offset + i (create_causal_mask(L, offset, window_size=window))."""
    for t in (q, k, v):
        _dev(t)
    _, Hq, L, D = q.shape
    Hkv, cap = k.shape[1], k.shape[2]
    qt = q[0].transpose(0, 1).contiguous()
    out = torch.empty_like(qt)
    _ffi.check(_ffi.load().pie_sdpa_prefill_window(_ffi.p(qt), _ffi.p(k.contiguous()), _ffi.p(v.contiguous()), Hq, Hkv, L, offset, cap, D, window,
                                                   float(scale), _ffi.dtype_code(q.dtype), _ffi.p(out), _ffi.stream()))
    return out.transpose(0, 1).unsqueeze(0).contiguous()


def sdpa_decode_ring(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor, scale: float,
                     pos: int, window: int, keep: int, rot0: int) -> torch.Tensor:
    """The decoder's step attention on a ring: q [Hq, D]; k / v [Hkv, cap, D] ring buffers (updated in place: the new rows k_new / v_new
    [Hkv, D] go to ring row slot(pos)); attends min(pos + 1, window) rows -> [Hq, D]."""
    for t in (q, k, v, k_new, v_new):
        _dev(t)
    Hq, D = q.shape
    Hkv, cap = k.shape[0], k.shape[1]
    stage = torch.zeros((2, Hkv, 64, D), dtype=k.dtype, device=k.device)
    stage[0, :, pos % 64] = k_new
    stage[1, :, pos % 64] = v_new
    lib = _ffi.load()
    ws = torch.empty(lib.pie_sdpa_decode_workspace_bytes(Hq, D) + 32, dtype=torch.uint8, device=q.device)
    out = torch.empty_like(q)
    _ffi.check(lib.pie_sdpa_decode_ring(_ffi.p(q.contiguous()), _ffi.p(k), _ffi.p(v), _ffi.p(stage), Hq, Hkv, cap, D, pos, window, keep, rot0,
                                        float(scale), _ffi.dtype_code(q.dtype), _ffi.p(out), _ffi.p(ws), _ffi.stream()))
    return out


# ---------------------------------------------------------------- batched speculation
SPEC_SEG_ROWS, SPEC_BATCH_ROWS = 8, 256   # rows of one sequence in a batched pass (the fed token and up to 7 drafts); rows of the pass


def paged_attn_verify_splits(B: int, n_kv_heads: int, max_blocks: int) -> int:
    """The splits paged_attn_verify(splits=0) cuts a segment's positions into (pie_paged_attn_verify_splits)."""
    return int(_ffi.load().pie_paged_attn_verify_splits(int(B), int(n_kv_heads), int(max_blocks)))


def paged_attn_verify(q: torch.Tensor, slab: torch.Tensor, n_pages: int, block_tables: torch.Tensor, row_seq: torch.Tensor, row_context_lens: torch.Tensor,
                      seg_first: torch.Tensor, n_kv_heads: int, scale: float, splits: int = 0) -> torch.Tensor:
    """The attention of a batched speculative pass (pie_paged_attn_verify): q [N, Hq, D]; block_tables int32 [B, max_blocks]; seg_first
    int32 [B + 1] cuts the N rows into the sequences' segments of 1..8 consecutive rows (none: an idle slot); row_seq int32 [N] = the row's
    block-table row; row_context_lens int32 [N] = the positions the row attends including its own, in the pages of its sequence -> [N, Hq,
    D].  One launch for all segments (one more to merge the splits); a segment's K / V are read once for all its rows and heads.
    splits: 0 = paged_attn_verify_splits(B, n_kv_heads, max_blocks), else 1..32."""
    for t in (q, slab, block_tables, row_seq, row_context_lens, seg_first):
        _dev(t)
    if any(t.dtype != torch.int32 for t in (block_tables, row_seq, row_context_lens, seg_first)):
        raise TypeError("paged_attn_verify: block_tables, row_seq, row_context_lens and seg_first must be int32")
    if q.dim() != 3 or block_tables.dim() != 2:
        raise ValueError("paged_attn_verify: q [N, Hq, D]; block_tables [B, max_blocks]")
    N, Hq, D = q.shape
    B = block_tables.shape[0]
    if row_seq.numel() != N or row_context_lens.numel() != N or seg_first.numel() != B + 1:
        raise ValueError("paged_attn_verify: row_seq [N]; row_context_lens [N]; seg_first [B + 1]")
    if slab.numel() * slab.element_size() < n_pages * 2 * 64 * n_kv_heads * D * 2:
        raise ValueError("paged_attn_verify: slab smaller than n_pages pages")
    if not 0 <= int(splits) <= 32:
        raise ValueError("paged_attn_verify: splits is 0 (chosen by the library) or 1..32")
    lib = _ffi.load()
    used = int(splits) or paged_attn_verify_splits(B, n_kv_heads, block_tables.shape[1])
    ws = torch.empty(max(int(lib.pie_paged_attn_verify_workspace_bytes(N, Hq, D, used)), 16), dtype=torch.uint8, device=q.device)
    out = torch.empty_like(q)
    _ffi.check(lib.pie_paged_attn_verify(_ffi.p(q), _ffi.p(slab), n_pages, _ffi.p(block_tables), block_tables.shape[1], _ffi.p(row_seq), _ffi.p(row_context_lens),
                                         _ffi.p(seg_first), N, B, Hq, int(n_kv_heads), D, float(scale), _ffi.dtype_code(q.dtype), int(splits), _ffi.p(out),
                                         _ffi.p(ws), _ffi.stream()))
    return out


def ngram_draft_rows_workspace(device, B: int) -> torch.Tensor:
    """pie_ngram_draft_rows' workspace for B sequences on `device`: uninitialised, nothing is carried from call to call."""
    return _workspace("pie_ngram_draft_rows_workspace_bytes", False, "ngram_draft_rows", f"1 <= B <= 4096, got {B}", device, B).view(torch.int32)


def ngram_draft_rows(ids: torch.Tensor, lengths: torch.Tensor, ngram_max: int, ngram_min: int, k: int, workspace: torch.Tensor | None = None,
                     out: tuple | None = None):
    """ngram_draft on B sequences in one call (pie_ngram_draft_rows): ids int32 [B, cap], lengths device int32 [B], each clamped on the
    device to [0, cap] -> (drafts int32 [B, k], counts int32 [B]), no host sync; row s is bit for bit ngram_draft(ids[s], lengths[s]).
    out = (drafts, counts) to write into (a row without a match keeps its draft's contents), else fresh tensors of -1 and 0."""
    who = "ngram_draft_rows"
    _int32_dev(ids, None, who, "ids")
    if ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < 1:
        raise ValueError("ngram_draft_rows: ids is [B, cap] with at least one id per row")
    B, cap = ids.shape
    _int32_dev(lengths, B, who, "lengths")
    ws = ngram_draft_rows_workspace(ids.device, B) if workspace is None else workspace
    if out is None:
        out = (torch.full((B, max(int(k), 1)), -1, dtype=torch.int32, device=ids.device), torch.zeros(B, dtype=torch.int32, device=ids.device))
    drafts, counts = out
    _int32_dev(drafts, None, who, "out[0]"), _int32_dev(counts, B, who, "out[1]"), _int32_dev(ws, None, who, "workspace")
    if tuple(drafts.shape) != (B, int(k)) or ws.numel() * 4 < int(_ffi.load().pie_ngram_draft_rows_workspace_bytes(B)):
        raise ValueError("ngram_draft_rows: out[0] is [B, k] and the workspace ngram_draft_rows_workspace()'s size")
    _ffi.check(_ffi.load().pie_ngram_draft_rows(_ffi.p(ids), _ffi.p(lengths), B, cap, int(ngram_max), int(ngram_min), int(k), _ffi.p(drafts), _ffi.p(counts),
                                                _ffi.p(ws), _ffi.stream()))
    return drafts, counts


def _spec_segments(who: str, logits: torch.Tensor, seg_first: torch.Tensor, drafts: torch.Tensor, ids: torch.Tensor | None, lengths: torch.Tensor | None,
                   out: tuple | None, with_logprobs: bool):
    """A segmented verify's block, validated: logits bf16 / f16 [N, V], seg_first int32 [B + 1], drafts int32 [B, >= 1], ids int32 [B, cap]
    with lengths int32 [B] or neither, out = (tokens int32 [B, 8], n int32 [B]) -- with_logprobs: and logprobs fp32 [N, V] -- or fresh
    ones -> (N, V, B, cap, out)."""
    _dev(logits)
    if logits.dim() != 2 or logits.dtype not in (torch.bfloat16, torch.float16) or not logits.is_contiguous():
        raise ValueError(f"{who}: contiguous bf16 / f16 [N, V] logits")
    N, V = logits.shape
    _int32_dev(seg_first, None, who, "seg_first"), _int32_dev(drafts, None, who, "drafts")
    B = seg_first.numel() - 1
    if B < 1 or drafts.dim() != 2 or drafts.shape[0] != B or drafts.shape[1] < 1:
        raise ValueError(f"{who}: seg_first [B + 1] and drafts [B, >= 1]")
    if (ids is None) != (lengths is None):
        raise ValueError(f"{who}: ids and lengths come together")
    cap = 0
    if ids is not None:
        _int32_dev(ids, None, who, "ids"), _int32_dev(lengths, B, who, "lengths")
        if ids.dim() != 2 or ids.shape[0] != B or ids.shape[1] < 1:
            raise ValueError(f"{who}: ids is [B, cap]")
        cap = ids.shape[1]
    if out is None:
        out = (torch.empty((B, SPEC_SEG_ROWS), dtype=torch.int32, device=logits.device), torch.empty(B, dtype=torch.int32, device=logits.device))
        if with_logprobs:
            out += (torch.empty((N, V), dtype=torch.float32, device=logits.device),)
    _int32_dev(out[0], B * SPEC_SEG_ROWS, who, "out[0]"), _int32_dev(out[1], B, who, "out[1]")
    if with_logprobs:
        _dev(out[2])
        if out[2].dtype != torch.float32 or not out[2].is_contiguous() or out[2].numel() < N * V:
            raise ValueError(f"{who}: out[2] is a contiguous fp32 [N, V] device tensor")
    return N, V, B, cap, out


def spec_verify_rows(logits: torch.Tensor, seg_first: torch.Tensor, drafts: torch.Tensor, ids: torch.Tensor | None = None, lengths: torch.Tensor | None = None,
                     workspace: torch.Tensor | None = None, out: tuple | None = None):
    """The segmented verify of a batched speculative pass (pie_spec_verify_rows): logits bf16 / f16 [N, V]; seg_first int32 [B + 1] cuts
    the rows into the sequences' segments of 1..8 rows (none: an idle slot); drafts int32 [B, width >= 1]: sequence s's drafts, one per row
    behind its first (a row beyond the width has no draft and ends the run) -> (tokens int32 [B, 8], n int32 [B]), no host sync.  Per sequence spec_verify's rule on its own rows: the drafts are
    accepted while draft[i] equals row i's greedy token (logprobs_argmax of that row, bit for bit; an id outside [0, V) is never accepted),
    n = accepted + 1, tokens = those greedy tokens, then -1; a one-row segment gives its greedy token and n = 1, an idle slot n = 0.
    ids int32 [B, cap] / lengths int32 [B] (together, optional): the drafter's input, ids[s, lengths[s] - 1] being the token the pass was
    fed -- the n tokens are written behind it and lengths[s] += n, on the device."""
    N, V, B, cap, (tokens, n) = _spec_segments("spec_verify_rows", logits, seg_first, drafts, ids, lengths, out, False)
    lib = _ffi.load()
    if workspace is None:
        workspace = torch.empty((int(lib.pie_spec_verify_rows_workspace_bytes(N)) + 15) // 16 * 2, dtype=torch.int64, device=logits.device)
    _ffi.check(lib.pie_spec_verify_rows(_ffi.p(logits), N, V, _ffi.dtype_code(logits.dtype), _ffi.p(seg_first), B, _ffi.p(drafts), drafts.shape[1], _ffi.p(tokens),
                                        _ffi.p(n), _ffi.p(ids), _ffi.p(lengths), cap, _ffi.p(workspace), _ffi.stream()))
    return tokens, n


def spec_verify_rows_sampled_workspace(device, n_rows: int, V: int) -> torch.Tensor:
    """pie_spec_verify_rows_sampled's workspace for a [n_rows, V] block on `device`: zeroed once, reusable from call to call."""
    return _workspace("pie_spec_verify_rows_sampled_workspace_bytes", True, "spec_verify_rows_sampled",
                      f"a [n_rows, V] block with 1 <= n_rows <= 65535 and 1 <= V <= 524288, got [{n_rows}, {V}]", device, n_rows, V)


def spec_verify_rows_sampled(logits: torch.Tensor, seg_first: torch.Tensor, fed: torch.Tensor, drafts: torch.Tensor, pos0: torch.Tensor, table: torch.Tensor,
                             recent_ids: torch.Tensor, bias: tuple | None = None, xtc: torch.Tensor | None = None, ids: torch.Tensor | None = None,
                             lengths: torch.Tensor | None = None, workspace: torch.Tensor | None = None, out: tuple | None = None):
    """The segmented verify of a batched speculative pass under per-seat tails (pie_spec_verify_rows_sampled): logits bf16 /
    f16 [N, V], EDITED IN PLACE; seg_first int32 [B + 1] and drafts int32 [B, width >= 1] as spec_verify_rows takes them; fed int32 [N] =
    the rows' input ids (a segment's fed token, then its drafts); pos0 int32 [B] = the position of every segment's first row; table (row_tail_table)
    [>= B] and recent_ids int32 [>= B, 1024] = the seats' records and rings, seat s = segment s; bias = (ids int32 [>= B, cap], values fp32
    [>= B, cap], n int32 [>= B]) as logits_bias_rows takes them, or None; xtc = int32 [>= B, XTC_WORDS] device records or None.
    Row j of segment s, at position pos0[s] + j: the seat's repetition penalty over the row's own window (the ring below pos0[s], fed
    from it on), the seat's bias, log-softmax and argmax, and the draw a one-row sample makes with the seat's sampler at stream position
    calls_s + j; the drafts are accepted while each equals the draw of the row before it.  Returns (tokens int32 [B, 8], n int32 [B],
    logprobs fp32 [N, V]), no host sync; afterwards a drawing seat's calls has advanced by n[s] and its ring holds the n[s] ids the pass fed
    for good, on the device.  ids / lengths as in spec_verify_rows.  workspace: spec_verify_rows_sampled_workspace's (zeroed once)."""
    who = "spec_verify_rows_sampled"
    N, V, B, cap, (tokens, n, logprobs) = _spec_segments(who, logits, seg_first, drafts, ids, lengths, out, True)
    _int32_dev(fed, N, who, "fed"), _int32_dev(pos0, B, who, "pos0"), _int32_dev(recent_ids, None, who, "recent_ids")
    _table(table, B, who)
    if recent_ids.dim() != 2 or recent_ids.shape[1] != RECENT_IDS or recent_ids.shape[0] < B:
        raise ValueError(f"{who}: recent_ids is [>= B, {RECENT_IDS}]")
    b_ids = b_vals = b_n = None
    b_cap = 0
    if bias is not None:
        b_ids, b_vals, b_n = bias
        _dev(b_ids), _dev(b_vals), _dev(b_n)
        if b_ids.dtype != torch.int32 or b_vals.dtype != torch.float32 or b_n.dtype != torch.int32 or b_ids.dim() != 2 or b_ids.shape != b_vals.shape or \
                not (b_ids.is_contiguous() and b_vals.is_contiguous() and b_n.is_contiguous()) or b_ids.shape[0] < B or b_n.numel() < B or not 1 <= b_ids.shape[1] <= 1024:
            raise ValueError(f"{who}: bias is (int32 ids, float32 values [>= B, 1 <= cap <= 1024], int32 n [>= B]), contiguous")
        b_cap = b_ids.shape[1]
    rec = None if xtc is None else _xtc(xtc, B, logits.device, who)
    lib = _ffi.load()
    need = int(lib.pie_spec_verify_rows_sampled_workspace_bytes(N, V))
    if need == 0:
        raise ValueError(f"{who}: a [N, V] block with 1 <= N <= 65535 and 1 <= V <= 524288, got [{N}, {V}]")
    if workspace is None:
        workspace = spec_verify_rows_sampled_workspace(logits.device, N, V)
    _dev(workspace)
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"{who}: the workspace is spec_verify_rows_sampled_workspace()'s size")
    _ffi.check(lib.pie_spec_verify_rows_sampled(_ffi.p(logits), N, V, _ffi.dtype_code(logits.dtype), _ffi.p(seg_first), B, _ffi.p(fed), _ffi.p(drafts), drafts.shape[1],
                                                _ffi.p(pos0), _ffi.p(table), _ffi.p(recent_ids), _ffi.p(b_ids), _ffi.p(b_vals), _ffi.p(b_n), b_cap, _ffi.p(rec),
                                                _ffi.p(tokens), _ffi.p(n), _ffi.p(logprobs), _ffi.p(ids), _ffi.p(lengths), cap, _ffi.p(workspace), _ffi.stream()))
    return tokens, n, logprobs
