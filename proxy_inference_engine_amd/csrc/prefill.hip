// prefill.hip -- batched prompt processing: Model.__call__(inputs[1, L], cache) for L > 1
// (models/llama/language.py:199-210 with the causal mask of models/base.py:18-53), SURVEY.md 8 row f1.
//
// At L > 1 the reference's nn.QuantizedLinear reaches MLX's matrix kernels (qmm), which dequantise the int4 block to T
// and feed a T x T -> fp32 MMA; the vector kernels (qmv, exact fp32 affine math) serve only the few-row case.  This file
// follows that split: prompts of prefill_min_rows() tokens or more run here, shorter ones as iterated decode steps.
//
// MI355X design, per weight format (no library GEMM anywhere: the hipBLASLt path of rounds 1-4 was removed in round 5):
//   * int4 g=64 modules multiply their 4-bit W4M tiles directly (w4m_gemm.hip: k_w4r_gemm up to 256 rows, k_w4l2_gemm beyond);
//   * dense modules, and int8 / group-32 modules, multiply a 16-bit copy in W16M tiles (w16_gemm.hpp: k_w16l_gemm, the weights
//     straight into MFMA fragment registers, x through LDS-DMA) -- dense ones tiled from their W16S units, quantised ones from
//     k_dequant_w4s / k_dequant_w8s (the mx.dequantize arithmetic: T(fp32(s*q) + b)); 288 GB of HBM keep the copies resident;
//   * hand-written HIP for everything around it: RMSNorm rows, RoPE + cache append from the packed q|k|v rows, causal
//     attention (MFMA flash kernel), the split merge, SwiGLU on the interleaved gate/up rows, residual adds.
// The chunk is bounded (PIE_KNOB_PREFILL_CHUNK, default 4096 rows: ~0.6 GB of activation scratch on the 8B model).
#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>

#include "decoder.hpp"
#include "gemm_rows.hpp"  // the many-row GEMM family of w4m_gemm.hip: W4mRope, W4lSlabs, the int4 entry (prefill_attn.hpp comes with it)
#include "paged_attn_verify.hpp"
#include "speculative.hpp"

// ---------------------------------------------------------------- kernels
// W4S -> T row-major [N, K]; one thread per code word (8 weights, 16 B out).  Same arithmetic as k_dequantize_w4g64.
template <class T, bool G32 = false>  // G32: W4S32 units (two {scale | bias} words per lane: code piece j is its own 32-wide group)
__global__ void k_dequant_w4s(const u32 *packed, int N, int K, int ns, u16 *out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wpr = K >> 3;  // words per row
    if (idx >= (size_t)N * wpr) return;
    const int r = (int)(idx / wpr), wk = (int)(idx % wpr);
    const int g = wk >> 3, lane = (r & 1) * 32 + (g & 31), j = (wk & 7) >> 2, t = wk & 3;
    const u32 *unit = packed + ((size_t)(r >> 1) * ns + (g >> 5)) * ((G32 ? W4S32_UNIT_BYTES : W4S_UNIT_BYTES) / 4);
    const u32 word = unit[j * 256 + lane * 4 + t], sb = G32 ? unit[512 + 2 * lane + j] : unit[512 + lane];
    const float s = lo_f32<T>(sb), b = hi_f32<T>(sb);
    u32 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // codes (2i, 2i+1) sit in the low / high half at nibble i (the W4S nibble order)
        const float lo = __fadd_rn(__fmul_rn(s, (float)((word >> (4 * i)) & 0xFu)), b);
        const float hi = __fadd_rn(__fmul_rn(s, (float)((word >> (16 + 4 * i)) & 0xFu)), b);
        o[i] = pack2<T>(lo, hi);
    }
    *reinterpret_cast<uint4 *>(out + (size_t)r * K + (size_t)wk * 8) = make_uint4(o[0], o[1], o[2], o[3]);
}

// W2S -> T row-major [N, K]; one thread per code word (16 weights, 32 B out).
template <class T>
__global__ void k_dequant_w2s(const u32 *packed, int N, int K, int ns, u16 *out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wpr = K >> 4;  // words per row
    if (idx >= (size_t)N * wpr) return;
    const int r = (int)(idx / wpr), wk = (int)(idx % wpr);
    const int g = wk >> 2, lane = (r & 1) * 32 + (g & 31), t = wk & 3;
    const u32 *unit = packed + ((size_t)(r >> 1) * ns + (g >> 5)) * (W2S_UNIT_BYTES / 4);
    const u32 word = unit[lane * 4 + t], sb = unit[256 + lane];
    const float s = lo_f32<T>(sb), b = hi_f32<T>(sb);
    u32 o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // codes (2j, 2j+1) of the word sit at bits 2j of the low / high half (the W2S order)
        const float lo = __fadd_rn(__fmul_rn(s, (float)((word >> (2 * j)) & 0x3u)), b);
        const float hi = __fadd_rn(__fmul_rn(s, (float)((word >> (16 + 2 * j)) & 0x3u)), b);
        o[j] = pack2<T>(lo, hi);
    }
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)r * K + (size_t)wk * 16);
    dst[0] = make_uint4(o[0], o[1], o[2], o[3]), dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// W6S -> T row-major [N, K]; one thread per low-plane code word (8 weights, 16 B out): q = low nibble + 16 x the high plane's two bits.
template <class T>
__global__ void k_dequant_w6s(const u32 *packed, int N, int K, int ns, u16 *out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wpr = K >> 3;
    if (idx >= (size_t)N * wpr) return;
    const int r = (int)(idx / wpr), wk = (int)(idx % wpr);
    const int g = wk >> 3, lane = (r & 1) * 32 + (g & 31), w4 = wk & 7, j = w4 >> 2, t = w4 & 3;
    const u32 *unit = packed + ((size_t)(r >> 1) * ns + (g >> 5)) * (W6S_UNIT_BYTES / 4);
    const u32 word = unit[j * 256 + lane * 4 + t], sb = unit[768 + lane];
    const u32 hiw = unit[512 + lane * 4 + (w4 >> 1)] >> (8 * (w4 & 1));  // codes 8 w4 .. + 7 = pairs 4 (w4 & 1) .. + 3 of high word w4 >> 1
    const float s = lo_f32<T>(sb), b = hi_f32<T>(sb);
    u32 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u32 qa = ((word >> (4 * i)) & 0xFu) | (((hiw >> (2 * i)) & 0x3u) << 4), qb = ((word >> (16 + 4 * i)) & 0xFu) | (((hiw >> (16 + 2 * i)) & 0x3u) << 4);
        o[i] = pack2<T>(__fadd_rn(__fmul_rn(s, (float)qa), b), __fadd_rn(__fmul_rn(s, (float)qb), b));
    }
    *reinterpret_cast<uint4 *>(out + (size_t)r * K + (size_t)wk * 8) = make_uint4(o[0], o[1], o[2], o[3]);
}

// W8S -> T row-major [N, K]; one thread per code word (4 weights, 8 B out).
template <class T, bool G32 = false>  // G32: W8S32 units (code pieces 0-1 / 2-3 are two 32-wide groups)
__global__ void k_dequant_w8s(const u32 *packed, int N, int K, int ns, u16 *out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wpr = K >> 2;
    if (idx >= (size_t)N * wpr) return;
    const int r = (int)(idx / wpr), wk = (int)(idx % wpr);
    const int g = wk >> 4, lane = (r & 1) * 32 + (g & 31), j = (wk & 15) >> 2, t = wk & 3;
    const u32 *unit = packed + ((size_t)(r >> 1) * ns + (g >> 5)) * ((G32 ? W8S32_UNIT_BYTES : W8S_UNIT_BYTES) / 4);
    const u32 word = unit[j * 256 + lane * 4 + t], sb = G32 ? unit[1024 + 2 * lane + (j >> 1)] : unit[1024 + lane];
    const float s = lo_f32<T>(sb), b = hi_f32<T>(sb);
    // stored byte order (c0, c2, c1, c3)
    const float q0 = __fadd_rn(__fmul_rn(s, (float)(word & 0xFFu)), b), q2 = __fadd_rn(__fmul_rn(s, (float)((word >> 8) & 0xFFu)), b);
    const float q1 = __fadd_rn(__fmul_rn(s, (float)((word >> 16) & 0xFFu)), b), q3 = __fadd_rn(__fmul_rn(s, (float)(word >> 24)), b);
    *reinterpret_cast<uint2 *>(out + (size_t)r * K + (size_t)wk * 4) = make_uint2(pack2<T>(q0, q1), pack2<T>(q2, q3));
}

// (cos, sin) of every row's rotary angles, once per forward: the angle of pair ii at position p is the same for all heads and all
// layers, and sincosf on arguments up to ~1e5 rad (argument reduction) was most of k_rope_append_rows' 8 us per layer.
__global__ void k_rope_cs_rows(const float *freqs, const DecState *state, const int *ctx_len, int half, float *cs) {
    const int m = blockIdx.x;
    int pos = ctx_len ? ctx_len[m] - 1 : state->pos + m;
    pos = pos < 0 ? 0 : pos;
    for (int ii = threadIdx.x; ii < half; ii += blockDim.x) {
        float sn, c;
        sincosf((float)pos * (1.0f / freqs[ii]), &sn, &c);
        cs[((size_t)m * half + ii) * 2] = c, cs[((size_t)m * half + ii) * 2 + 1] = sn;
    }
}

#ifndef SLAB_BATCH
#define SLAB_BATCH 4
#endif
// V = float2 / float4: one thread's NV vectors at element offsets off[]; the slabs are fetched BATCH at a time (all BATCH x NV loads in flight
// before the first add -- a plain loop over the slabs waits out one memory latency per slab: 15 us instead of 5 for a 64-row o_proj
// consumer) and added strictly in slab order.
template <class V, int NV, int BATCH = 4>
__device__ __forceinline__ void slab_sum(const float *part, int S, size_t MN, const size_t (&off)[NV], V (&acc)[NV]) {
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = *reinterpret_cast<const V *>(part + off[v]);
    for (int z = 1; z < S; z += BATCH) {
        V b[BATCH][NV];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const size_t zz = (size_t)(z + u < S ? z + u : S - 1) * MN;  // clamp, never branch around a load
#pragma unroll
            for (int v = 0; v < NV; ++v) b[u][v] = *reinterpret_cast<const V *>(part + zz + off[v]);
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u)
            if (z + u < S) {
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    acc[v].x += b[u][v].x, acc[v].y += b[u][v].y;
                    if constexpr (sizeof(V) == 16) acc[v].z += b[u][v].z, acc[v].w += b[u][v].w;
                }
            }
    }
}

// RoPE (llama/utils.py:42-50, offset = cache.offset) + cache append (reusable.py:134-137) for M rows of the packed
// q|k|v projection: packed columns (2i, 2i+1) of a q/k head are its dims (i, i + D/2); v columns are natural.
// grid M, one thread per packed column pair.
// SLAB / I8: the two optional input / output forms as compile-time switches -- carried as run-time branches they cost the plain
// 4096-row launch 7.6 us (34.4 vs 26.8 us per layer)
template <class T, bool SLAB = false, bool I8 = false>
__global__ void __launch_bounds__(256) k_rope_append_rows(const u16 *qkv, int n_cols, const float *freqs, const DecState *state,
                                                         const unsigned long long *kv_table, int layer, int n_layers, int n_heads,
                                                         int n_kv_heads, int HD, int traditional, u16 *q_out, const int *block_table,
                                                         int n_pages, const float *rope_cs, const int *ctx_len = nullptr, int bt_stride = 0,
                                                         u16 *slab = nullptr, const int *row_seq = nullptr, u16 *kc = nullptr, u16 *vc = nullptr,
                                                         const float *part = nullptr, int S = 0, size_t MN = 0, size_t i8_page_bytes = 0) {
    // part != nullptr: the projection arrives as the fp32 slabs of a K-split GEMM (W4lSlabs) instead of qkv
    // i8_page_bytes != 0 (with `slab`): int8 pages with per-head fp16 scales (paged_i8.hip): the rotated K / the V element x, already
    // rounded to T, is stored as clamp(rint(x / s), -127, 127) with the scale of (its page, its kv-head)
    // row_seq / kc / vc (several prompts in one pass): row m belongs to sequence row_seq[m] (its block-table row), and the
    // rotated K and the V rows are also written to contiguous [n_kv_heads, rows, HD] buffers the attention of this pass reads
    // ctx_len != nullptr (multi-sequence decode step): row m is its own sequence at position ctx_len[m] - 1 with its own block
    // table row and the layer's slab given directly; otherwise row m continues the decoder's one sequence at state->pos + m
    const int m = blockIdx.x, pos = ctx_len ? ctx_len[m] - 1 : state->pos + m, half = HD >> 1;
    if (pos < 0) return;  // idle slot of the batch
    int cap = ctx_len ? 64 : state->cap, kvrow = pos;
    const int q_cols = n_heads * HD, k_cols = n_kv_heads * HD;
    u16 *kdst = slab ? slab : reinterpret_cast<u16 *>(kv_table[layer]);
    u16 *vdst = slab ? slab + (size_t)n_kv_heads * 64 * HD : reinterpret_cast<u16 *>(kv_table[n_layers + layer]);
    block_table = block_table ? block_table + (size_t)(row_seq ? row_seq[m] : m) * bt_stride : nullptr;
    const int n_rows = gridDim.x;
    char *page8 = nullptr;  // int8 pages: this row's page
    if (block_table) {  // paged KV: the row goes to slot pos % 64 of page block_table[pos / 64]
        const unsigned pg = min((unsigned)block_table[pos >> 6], (unsigned)n_pages - 1u);
        const size_t pg_off = (size_t)pg * 2 * 64 * n_kv_heads * HD;
        kdst += pg_off, vdst += pg_off, cap = 64, kvrow = pos & 63;
        if (I8 && i8_page_bytes && slab) page8 = reinterpret_cast<char *>(slab) + (size_t)pg * i8_page_bytes;
    }
    const size_t blk8 = (size_t)n_kv_heads * 64 * HD;
    auto q8 = [](float x, float sc) {
        float q = rintf(x / sc);
        q = q < -127.0f ? -127.0f : (q > 127.0f ? 127.0f : q);
        return (signed char)(q == q ? (int)q : 0);
    };
    auto f16f = [](u16 h) { return (float)__builtin_bit_cast(_Float16, h); };
    const u16 *row = qkv + (size_t)m * n_cols;
    // gridDim.y workgroups share a row (few rows summing fp32 slabs: one workgroup per row cannot keep enough loads in flight)
    for (int p = blockIdx.y * blockDim.x + threadIdx.x; p < (n_cols >> 1); p += gridDim.y * blockDim.x) {
        const int R = 2 * p;
        u32 pr;
        if (SLAB && part) {
            const size_t i[1] = {(size_t)m * n_cols + R};
            float2 a[1];
            slab_sum<float2, 1>(part, S, MN, i, a);
            pr = pack2<T>(a[0].x, a[0].y);
        } else pr = *reinterpret_cast<const u32 *>(row + R);
        const float ra = lo_f32<T>(pr), rb = hi_f32<T>(pr);
        if (R < q_cols + k_cols) {
            const int rr = R < q_cols ? R : R - q_cols;
            const int head = rr / HD, ii = (rr % HD) >> 1;
            const float2 csn = *reinterpret_cast<const float2 *>(rope_cs + ((size_t)m * half + ii) * 2);  // k_rope_cs_rows
            const float cs = csn.x, sn = csn.y;
            u16 *dst = R < q_cols ? q_out + ((size_t)m * n_heads + head) * HD : kdst + ((size_t)head * cap + kvrow) * HD;
            const int i0 = traditional ? 2 * ii : ii, i1 = traditional ? 2 * ii + 1 : ii + half;
            const u16 o0 = T::from_f32(__fsub_rn(__fmul_rn(ra, cs), __fmul_rn(rb, sn))), o1 = T::from_f32(__fadd_rn(__fmul_rn(ra, sn), __fmul_rn(rb, cs)));
            if (I8 && page8 && R >= q_cols) {
                const float sk = f16f(reinterpret_cast<const u16 *>(page8 + 2 * blk8)[head]);
                signed char *kb = reinterpret_cast<signed char *>(page8) + ((size_t)head * 64 + kvrow) * HD;
                kb[i0] = q8(T::to_f32(o0), sk), kb[i1] = q8(T::to_f32(o1), sk);
            } else dst[i0] = o0, dst[i1] = o1;
            if (kc && R >= q_cols) {
                u16 *c = kc + ((size_t)head * n_rows + m) * HD;
                c[i0] = o0, c[i1] = o1;
            }
        } else {
            const int rr = R - q_cols - k_cols;
            if (I8 && page8) {
                const int head = rr / HD;
                const float sv = f16f(reinterpret_cast<const u16 *>(page8 + 2 * blk8)[n_kv_heads + head]);
                signed char *vb = reinterpret_cast<signed char *>(page8) + blk8 + ((size_t)head * 64 + kvrow) * HD + rr % HD;
                vb[0] = q8(ra, sv), vb[1] = q8(rb, sv);
            } else *reinterpret_cast<u32 *>(vdst + ((size_t)(rr / HD) * cap + kvrow) * HD + rr % HD) = pr;
            if (vc) *reinterpret_cast<u32 *>(vc + ((size_t)(rr / HD) * n_rows + m) * HD + rr % HD) = pr;
        }
    }
}

// nn.silu(gate) * up (language.py:127) on interleaved columns (2i, 2i+1) = (gate_i, up_i); 4 outputs per thread.
template <class T>
__global__ void k_swiglu_rows(const u16 *gu, size_t n_out, u16 *act) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n_out) return;  // n_out is a multiple of 4 (inter % 64 == 0)
    const uint4 v = *reinterpret_cast<const uint4 *>(gu + 2 * i);
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    u16 o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float g = lo_f32<T>(w[k]), u = hi_f32<T>(w[k]);
        o[k] = T::from_f32(round_T<T>(g / (1.0f + expf(-g))) * u);
    }
    *reinterpret_cast<uint2 *>(act + i) = make_uint2((u32)o[0] | ((u32)o[1] << 16), (u32)o[2] | ((u32)o[3] << 16));
}

// y[m, :] = T(y[m, :] + b) for the Linear biases (y already T-rounded by the GEMM); 8 columns per thread, N % 8 == 0.
template <class T>
__global__ void k_bias_rows(u16 *y, const u16 *b, size_t n8, int N8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const uint4 v = reinterpret_cast<const uint4 *>(y)[i], bb = reinterpret_cast<const uint4 *>(b)[i % N8];
    const u32 a[4] = {v.x, v.y, v.z, v.w}, c[4] = {bb.x, bb.y, bb.z, bb.w};
    u32 o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = pack2<T>(lo_f32<T>(a[k]) + lo_f32<T>(c[k]), hi_f32<T>(a[k]) + hi_f32<T>(c[k]));
    reinterpret_cast<uint4 *>(y)[i] = make_uint4(o[0], o[1], o[2], o[3]);
}

// h = x + r (language.py:151,153) fused with the RMSNorm that follows it (language.py:137-141): x <- T(x + r) in place,
// xn <- w * T(h * rsqrt(mean(h^2) + eps)).  One workgroup per row; the row stays in registers between the two passes.
template <class T>
__global__ void __launch_bounds__(256) k_add_rms_norm_rows(u16 *x, const u16 *r, const u16 *w, float eps, int H, u16 *xn, const u16 *bias = nullptr,
                                                          const float *part = nullptr, int S = 0, size_t MN = 0) {
    // part != nullptr: the Linear's output arrives as the fp32 slabs of a K-split many-row GEMM (W4lSlabs): r = T(T(sum of the slabs) + bias)
    __shared__ float red[4];
    u16 *xr = x + (size_t)blockIdx.x * H;
    const u16 *rr = r + (size_t)blockIdx.x * H;
    u16 *yr = xn + (size_t)blockIdx.x * H;
    constexpr int MAXP = 4;  // 8-element pieces per thread: H <= 8192
    uint4 hv[MAXP];
    float ssq = 0.0f;
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
        const int i = (threadIdx.x + p * 256) * 8;
        if (i < H) {
            const uint4 a = *reinterpret_cast<const uint4 *>(xr + i);
            uint4 b;
            if (part) {
                float4 f0, f1;
                {
                    const size_t o[2] = {(size_t)blockIdx.x * H + i, (size_t)blockIdx.x * H + i + 4};
                    float4 f[2];
                    slab_sum<float4, 2, SLAB_BATCH>(part, S, MN, o, f);
                    f0 = f[0], f1 = f[1];
                }
                float v[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
                if (bias) {
                    const uint4 bb = *reinterpret_cast<const uint4 *>(bias + i);
                    const u32 bw[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[2 * j] = round_T<T>(v[2 * j]) + lo_f32<T>(bw[j]), v[2 * j + 1] = round_T<T>(v[2 * j + 1]) + hi_f32<T>(bw[j]);
                }
                b = make_uint4(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7]));
            } else {
                b = *reinterpret_cast<const uint4 *>(rr + i);
            }
            const u32 av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
            u32 o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = pack2<T>(lo_f32<T>(av[j]) + lo_f32<T>(bv[j]), hi_f32<T>(av[j]) + hi_f32<T>(bv[j]));
                const float lo = lo_f32<T>(o[j]), hi = hi_f32<T>(o[j]);
                ssq = fmaf(lo, lo, ssq);
                ssq = fmaf(hi, hi, ssq);
            }
            hv[p] = make_uint4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<uint4 *>(xr + i) = hv[p];
        }
    }
    ssq = wave_sum(ssq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ssq;
    __syncthreads();
    const float inv = 1.0f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)H + eps);
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
        const int i = (threadIdx.x + p * 256) * 8;
        if (i < H) {
            const uint4 g = *reinterpret_cast<const uint4 *>(w + i);
            const u32 vv[4] = {hv[p].x, hv[p].y, hv[p].z, hv[p].w}, gg[4] = {g.x, g.y, g.z, g.w};
            u32 o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = pack2<T>(round_T<T>(lo_f32<T>(vv[j]) * inv) * lo_f32<T>(gg[j]), round_T<T>(hi_f32<T>(vv[j]) * inv) * hi_f32<T>(gg[j]));
            *reinterpret_cast<uint4 *>(yr + i) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

template <class T>
static int add_rms_norm_rows(u16 *x, const u16 *r, const void *w, float eps, int M, int H, int dtype, u16 *xn, hipStream_t st,
                             const void *bias = nullptr, const W4lSlabs *sl = nullptr) {
    const W4lSlabs none, &p = sl && sl->S > 1 ? *sl : none;  // (mlp_rows only offers to take slabs for H <= 8192)
    if (p.S <= 1 && H > 8192) {  // wider than the register-resident row: the two separate kernels
        const int rc = pie_add(x, r, (size_t)M * H, dtype, x, st);
        return rc ? rc : pie_rms_norm(x, w, eps, M, H, dtype, xn, st);
    }
    hipLaunchKernelGGL(k_add_rms_norm_rows<T>, dim3(M), dim3(256), 0, st, x, r, (const u16 *)w, eps, H, xn, (const u16 *)bias, p.part, p.S, p.MN);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

__global__ void k_add_pos(DecState *s, int delta) { s->pos += delta; }
__global__ void k_set_pos(DecState *s, int pos) { s->pos = pos; }

// ---------------------------------------------------------------- scratch
struct PrefillScratch {
    int rows = 0;           // chunk capacity (rows)
    size_t w_elems = 0;     // capacity of the dequantised-weight buffer (elements)
    u16 *wT = nullptr, *wM = nullptr, *x = nullptr, *xn = nullptr, *qkv = nullptr, *q = nullptr, *attn = nullptr, *gu = nullptr, *act = nullptr, *r = nullptr;
    float *part_acc = nullptr, *part_ml = nullptr, *rope_cs = nullptr;
    u16 *kc = nullptr, *vc = nullptr;  // [n_kv_heads, rows, head_dim]: this pass's K / V rows, contiguous (several prompts in one pass)
    int part_splits = 0;
    // Resident T copies of the layer matrices, keyed by the packed-weight pointer: the per-chunk dequantisation moves
    // 4.6 B per parameter (7 ms of a 10.8 ms 128-token prefill on the 8B model) for 2 B per parameter of HBM; kept when
    // that is a small share of the free memory (PIE_KNOB_PREFILL_RESIDENT overrides), built on first use.
    std::map<const void *, u16 *> resident;
    // W4M tile copies (w4m_gemm.hip) of int4 matrices, the operand of every many-row int4 GEMM: 0.5625 B per weight each
    std::map<const void *, void *> resident_w4m;
    LogitStat *tail_stats = nullptr;  // multi-sequence step / several prompts per pass: per-row tail partials
    size_t tail_entries = 0;           // its capacity in ENTRIES (rows x partials per row: the two users need 256 and max(lm_head waves, 256) per row)
    // Captured multi-sequence step (pie_decoder_step_batch with PIE_STEP_GRAPH): valid while the caller's buffers (key) and every
    // device allocation baked into the launches (alloc_gen) stay what they were at capture time.
    unsigned alloc_gen = 0;
    hipGraphExec_t batch_graph = nullptr;
    std::vector<uintptr_t> batch_key, warm_key;
    unsigned batch_gen = 0, warm_gen = 0;
    void *w4l_ws = nullptr;   // fp32 partial tiles of the K-split prompt GEMM (w4m_gemm.hip)
    size_t w4l_ws_bytes = 0;
    int resident_mode = -1;   // -1: budget not fixed yet
    size_t resident_left = 0; // bytes still available for resident copies
};

// A buffer that only grows: re-allocated, its contents dropped, when `need` units exceed its capacity (captured launches are stale then)
static int scratch_grow(PrefillScratch *s, void **buf, size_t *cap, size_t need, size_t unit_bytes = 1) {
    if (*cap >= need) return PIE_OK;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr, *cap = 0;
    PIE_HIP_TRY(hipMalloc(buf, need * unit_bytes));
    *cap = need, ++s->alloc_gen;
    return PIE_OK;
}

// The tail partials are sized in entries, not rows: a prompt pass needs 256 per row, the fused few-sequence step one per lm_head GEMV
// wave (2048 at V = 128256) -- a buffer sized by the first and reused by the second was overrun 8 x.
static int tail_stats_reserve(PrefillScratch *s, size_t entries) {
    return scratch_grow(s, (void **)&s->tail_stats, &s->tail_entries, entries, sizeof(LogitStat));
}

static void scratch_release(PrefillScratch *s) {  // the chunk buffers; resident weight copies survive a re-size
    void *ptrs[] = {s->wT, s->wM, s->x, s->xn, s->qkv, s->q, s->attn, s->gu, s->act, s->r, s->part_acc, s->part_ml, s->rope_cs, s->kc, s->vc};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (s->batch_graph) (void)hipGraphExecDestroy(s->batch_graph);
    PrefillScratch fresh;  // everything back to its default, except what survives:
    fresh.resident = std::move(s->resident), fresh.resident_w4m = std::move(s->resident_w4m), fresh.resident_mode = s->resident_mode, fresh.resident_left = s->resident_left;
    fresh.tail_stats = s->tail_stats, fresh.tail_entries = s->tail_entries, fresh.w4l_ws = s->w4l_ws, fresh.w4l_ws_bytes = s->w4l_ws_bytes;
    fresh.alloc_gen = s->alloc_gen + 1;  // the chunk buffers move: captured launches are stale
    *s = std::move(fresh);
}

void prefill_free(pie_decoder *d) {
    if (!d->prefill) return;
    scratch_release(d->prefill);
    for (auto &kv : d->prefill->resident) (void)hipFree(kv.second);
    for (auto &kv : d->prefill->resident_w4m) (void)hipFree(kv.second);
    if (d->prefill->tail_stats) (void)hipFree(d->prefill->tail_stats);
    if (d->prefill->w4l_ws) (void)hipFree(d->prefill->w4l_ws);
    delete d->prefill;
    d->prefill = nullptr;
}

int prefill_min_rows() {  // read per call (not cached): tests and tools switch regimes inside one process
    const int k = pie_knob(PIE_KNOB_PREFILL_MIN);  // prompts shorter than this run as iterated decode steps (MLX's qmv regime)
    const int n = k >= 0 ? k : 6;  // MLX's own qmv limit is 6..32 rows by device and shape; 5 ms batched vs 1.35 ms per iterated row
    return n < 2 ? 2 : n;
}

static int prefill_chunk_rows() {
    const int k = pie_knob(PIE_KNOB_PREFILL_CHUNK);  // measured on the 8B model, 4096-token prompt: 512 -> 119 ms, 1024 -> 83, 2048 -> 67, 4096 -> 65
    const int n = k >= 0 ? k : 4096;
    return n < 16 ? 16 : (n > 8192 ? 8192 : n);
}

static int scratch_reserve(pie_decoder *d, int rows, size_t w_elems, int splits) {
    if (!d->prefill) d->prefill = new PrefillScratch();
    PrefillScratch *s = d->prefill;
    const pie_decoder_config &c = d->cfg;
    const size_t QD = (size_t)c.n_heads * c.head_dim, NQKV = QD + 2 * (size_t)c.n_kv_heads * c.head_dim;
    if (rows > s->rows || splits > s->part_splits) {
        const size_t we = s->w_elems > w_elems ? s->w_elems : w_elems;
        scratch_release(s);
        const size_t R = (size_t)rows;
#define PF_ALLOC(ptr, bytes) PIE_HIP_TRY(hipMalloc((void **)&(ptr), (bytes)))
        PF_ALLOC(s->x, 2 * R * c.hidden);
        PF_ALLOC(s->xn, 2 * R * c.hidden);
        PF_ALLOC(s->r, 2 * R * c.hidden);
        PF_ALLOC(s->qkv, 2 * R * NQKV);
        PF_ALLOC(s->q, 2 * R * QD);
        PF_ALLOC(s->attn, 2 * R * QD);
        PF_ALLOC(s->gu, 2 * R * 2 * c.inter);
        PF_ALLOC(s->act, 2 * R * c.inter);
        PF_ALLOC(s->part_acc, 4 * R * c.n_heads * splits * c.head_dim);
        PF_ALLOC(s->part_ml, 4 * R * c.n_heads * splits * 2);
        PF_ALLOC(s->rope_cs, 4 * R * c.head_dim);
        PF_ALLOC(s->kc, 2 * R * c.n_kv_heads * c.head_dim);
        PF_ALLOC(s->vc, 2 * R * c.n_kv_heads * c.head_dim);
        PF_ALLOC(s->wT, 2 * we);
        PF_ALLOC(s->wM, 2 * we);
        s->rows = rows, s->part_splits = splits, s->w_elems = we;
    }
    if (w_elems > s->w_elems) {
        if (s->wT) (void)hipFree(s->wT);
        if (s->wM) (void)hipFree(s->wM);
        s->wT = nullptr, s->wM = nullptr;
        PF_ALLOC(s->wT, 2 * w_elems);
        PF_ALLOC(s->wM, 2 * w_elems);
        s->w_elems = w_elems, ++s->alloc_gen;
    }
#undef PF_ALLOC
    return PIE_OK;
}

// ---------------------------------------------------------------- the batched forward

// Byte budget for resident T copies of layer matrices, fixed at the first batched prefill: half of the free device memory
// (PIE_KNOB_PREFILL_RESIDENT: 0 disables, <GiB> sets it; PIE_KNOB_PREFILL_RESIDENT_KB: the same in KiB, first).  Matrices are admitted in first-use order while the budget lasts
// (8B model: all 15 GB; 70B: ~7/8 of its 140 GB); the rest keep going through the scratch every chunk.
static size_t resident_budget(pie_decoder *d) {
    PrefillScratch *s = d->prefill;
    if (s->resident_mode < 0) {
        size_t free_b = 0, total_b = 0;
        const int k = pie_knob(PIE_KNOB_PREFILL_RESIDENT), kb = pie_knob(PIE_KNOB_PREFILL_RESIDENT_KB);
        if (kb >= 0) s->resident_left = (size_t)kb << 10;
        else if (k >= 0) s->resident_left = (size_t)k << 30;
        else s->resident_left = hipMemGetInfo(&free_b, &total_b) == hipSuccess ? free_b / 2 : 0;
        s->resident_mode = 1;
    }
    return s->resident_left;
}

// The 16-bit operand of a many-row product, as W16M tiles: dense modules straight from their W16S units, int8 / group-32 modules
// dequantised (mx.dequantize's arithmetic: the qmm regime multiplies T copies) into the row-major staging buffer and tiled from there.
template <class T>
static int expand_weights(pie_decoder *d, const void *packed, int N, int K, void *w16m, u16 *staging, hipStream_t st) {
    const int wf = d->mat_fmt(packed);  // per-module quantisation: a checkpoint may mix formats (models/utils.py:99-109)
    if (wf == PIE_W_DENSE) return w16m_from_w16s_launch(packed, N, K, w16m, st);
    // one thread per code word: 4 weights (8-bit codes), 16 (2-bit), else 8 (4-bit codes and W6S's low plane)
    const auto k = wf == PIE_W_INT8_G64 ? k_dequant_w8s<T, false> : wf == PIE_W_INT8_G32 ? k_dequant_w8s<T, true> : wf == PIE_W_INT2_G64 ? k_dequant_w2s<T>
                 : wf == PIE_W_INT6_G64 ? k_dequant_w6s<T> : wf == PIE_W_INT4_G32 ? k_dequant_w4s<T, true> : k_dequant_w4s<T, false>;
    const int bits = weight_format(wf).bits;
    const size_t words = (size_t)N * (K >> (bits == 8 ? 2 : bits == 2 ? 4 : 3));
    hipLaunchKernelGGL(k, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, (const u32 *)packed, N, K, w4s_slices(K), staging);
    PIE_LAUNCH_CHECK();
    return w16m_from_rows_launch(staging, N, K, w16m, st);
}

template <class T>
static int bias_rows(u16 *y, const void *bias, int M, int N, hipStream_t st) {
    const size_t n8 = (size_t)M * N / 8;
    hipLaunchKernelGGL(k_bias_rows<T>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, y, (const u16 *)bias, n8, N / 8);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// What a many-row Linear is asked for beyond y = x . W^T, and what it did about it
struct RowsOpts {
    const void *bias = nullptr;  // the Linear's
    bool keep = true;            // a layer matrix (eligible for a resident copy); the lm_head of a logits-on-every-position call goes through the scratch
    bool keep_w4m = false;       // ... unless this says that its int4 tiles may stay (the lm_head of the multi-sequence passes)
    u16 *act = nullptr;          // the packed gate|up matrix: the GEMM may apply the SwiGLU itself and write act [M, N / 2] instead of y (RowsDone::fused_swiglu)
    W4mRope *rope = nullptr;     // the packed q|k|v matrix: the GEMM may rotate q / k and append k / v itself instead of writing y (RowsDone::roped)
    bool slabs = false;          // the caller's consumer takes the fp32 slabs of a K-split GEMM (and the bias) instead of y (RowsDone::slabs.S > 1 tells whether it must)
};
struct RowsDone {
    bool fused_swiglu = false, roped = false;
    W4lSlabs slabs;
};

// y[M, N] = x[M, K] . W^T (+ bias) for one streaming-layout matrix, by weight format and row count:
//   * up to GEMV_ROWS_MAX rows (MLX's qmv regime) the streaming GEMVs, where the format and shape have one;
//   * int4 g=64 matrices on their resident W4M tiles through the one int4 entry (w4_rows_launch, w4m_gemm.hip: k_w4r_gemm up to 256 rows, the tile kernels
//     beyond) -- no 16-bit copy of the weights;
//   * everything else -- dense, int8 and group-32 modules, int4 shapes the tiles do not take (N not a multiple of 32) or that the residency budget has no
//     room for -- multiplies a W16M copy on k_w16l_gemm (w16_gemm.hpp).
template <class T>
static int linear_rows(pie_decoder *d, const void *packed, int N, int K, const u16 *x, int M, u16 *y, hipStream_t st, const RowsOpts &o = RowsOpts(),
                       RowsDone *done = nullptr) {
    PrefillScratch *s = d->prefill;
    RowsDone none;
    if (!done) done = &none;
    *done = RowsDone();
    const void *bias = o.bias;
    const int wf = d->mat_fmt(packed);
    const bool is_int4 = wf == PIE_W_INT4_G64;
    if ((wf == PIE_W_INT4_G32 || wf == PIE_W_INT8_G32 || wf == PIE_W_INT2_G64 || wf == PIE_W_INT6_G64) && M <= GEMV_ROWS_MAX && K <= 32768 && N % 2 == 0) {  // group-32 / 2- / 6-bit codes, qmv regime: the streaming GEMV, one pass per row
        GemvArgs a = {};
        a.fmt = wf, a.w = (const char *)packed, a.K = K, a.N = N, a.x = x, a.y = y, a.lin_bias = (const u16 *)bias;
        return w4s_gemv_launch(d->cfg.dtype, PRO_NONE, EPI_STORE, a, M, st);
    }
    // Below 6 rows MLX multiplies row by row (qmv: exact fp32 per row, mx.quantized_matmul as reached from nn.QuantizedLinear): the
    // streaming GEMV with the rows' images side by side -- one pass over the weights, each row with the batch-1 arithmetic.
    if (is_int4 && M <= GEMV_ROWS_MAX && K % 64 == 0 && N % 2 == 0 && gemv_rows_lds_bytes(K, 1) <= 160u * 1024u)
        return w4s_gemv_rows_launch(d->cfg.dtype, packed, N, K, x, M, y, (const u16 *)bias, st);
    auto w4l_reserve = [&](size_t wb) { return scratch_grow(s, &s->w4l_ws, &s->w4l_ws_bytes, wb); };  // fp32 slabs of a K-split product
    int rc = PIE_OK;
    if (is_int4 && N % 32 == 0 && K % 64 == 0) {  // every shape the W4M tiles take: get tiles, reserve, enter, add the bias if it is still ours
        // resident W4M tile copy (0.5625 B per weight, built on first use within the residency budget); none: no room, the W16M path below
        void *wm = nullptr;
        auto it = s->resident_w4m.find(packed);
        if (it != s->resident_w4m.end()) wm = it->second;
        else if (resident_budget(d) >= w4m_bytes(N, K) && hipMalloc(&wm, w4m_bytes(N, K)) == hipSuccess) {
            s->resident_w4m[packed] = wm, s->resident_left -= w4m_bytes(N, K), ++s->alloc_gen;
            if ((rc = w4m_repack_launch(packed, N, K, wm, st))) return rc;
        } else (void)hipGetLastError(), wm = nullptr;
        if (wm) {
            W4Rows q = {d->cfg.dtype, wm, x, M, N, K, y};
            q.bias = bias, q.wish = o.act ? W4R_SWIGLU : o.rope ? W4R_ROPE : W4R_STORE, q.act = o.act, q.rope = o.rope;
            // 8B prompt of 64 / 128 / 256 / 512 / 700 tokens, slabs summed by the consumers vs reduce launches: 3.70 / 4.56 / 6.13 / 9.56 / 14.26 ms
            // vs 3.96 / 4.82 / 6.20 / 9.75 / 14.38.  (With ONE workgroup per row the RoPE consumer could not keep enough slab loads in flight
            // below ~200 rows -- 4.21 ms at 64 tokens -- so few rows get four workgroups each there; that split applies to the RoPE consumer, not to the
            // add + RMSNorm consumers, whose row-wide reduction keeps them at one workgroup per row.)
            q.take_slabs = o.slabs, q.few_rows = o.keep || o.keep_w4m;
            if ((rc = w4l_reserve(w4_rows_workspace_bytes(q)))) return rc;
            W4Outcome out;
            if ((rc = w4_rows_launch(q, s->w4l_ws, st, &out))) return rc;
            done->fused_swiglu = out.epi == W4R_SWIGLU, done->roped = out.epi == W4R_ROPE;
            if (out.slabs > 1) done->slabs.part = (const float *)s->w4l_ws, done->slabs.S = out.slabs, done->slabs.MN = (size_t)M * N;
            else if (bias && !out.bias_done) return bias_rows<T>(y, bias, M, N, st);
            return PIE_OK;
        }
    }
    // Everything else -- dense modules, int8 and group-32 modules beyond the GEMV's rows -- multiplies a 16-bit copy of the matrix in W16M
    // tiles with the hand-written MFMA GEMM (w16_gemm.hpp); resident copies are built on first use within the budget.
    PIE_REQUIRE(K % 64 == 0, PIE_E_SHAPE, "prefill: a many-row Linear needs in_features % 64 == 0 (pie_set_knob(PIE_KNOB_PREFILL_MIN, 1000000) processes prompts as iterated decode steps)");
    u16 *wM = s->wM;
    bool ready = false;
    if (o.keep) {
        const size_t bytes = w16m_size(N, K);
        auto it = s->resident.find(packed);
        if (it != s->resident.end()) wM = it->second, ready = true;
        else if (resident_budget(d) >= bytes) {
            if (hipMalloc((void **)&wM, bytes) == hipSuccess) s->resident[packed] = wM, s->resident_left -= bytes, ++s->alloc_gen;
            else (void)hipGetLastError(), wM = s->wM, s->resident_left = 0;  // out of memory: scratch from here on
        }
    }
    if (!ready && (rc = expand_weights<T>(d, packed, N, K, wM, s->wT, st))) return rc;
    if ((rc = w4l_reserve(w16l_workspace_bytes(M, N, K)))) return rc;  // fp32 slabs of a K-split shape (few rows, narrow matrices)
    // gate|up: bias and SwiGLU in the GEMM's epilogue where the shape does not split K
    return w16l_gemm_launch(d->cfg.dtype, wM, x, 0, M, N, K, y, s->w4l_ws, st, bias, o.act, &done->fused_swiglu, 0);
}

// ---------------------------------------------------------------- what the many-row passes share
// Elements of the 16-bit weight scratch: the largest W16M copy a pass may build (with_lm_head: the lm_head goes through linear_rows too)
static size_t w16_copy_elems(const pie_decoder_config &c, bool with_lm_head) {
    const int H = c.hidden, NQKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, I = c.inter;
    // the 16-bit copies are W16M tiles (rows padded to 32, columns to 64)
    return std::max({w16m_size(2 * I, H), w16m_size(NQKV, H), w16m_size(H, I), with_lm_head ? w16m_size(c.vocab, H) : (size_t)0}) / 2;
}

// h = embed_tokens(ids) (language.py:176) for M rows into x
static int embed_rows(const pie_decoder *d, const int32_t *ids, int M, u16 *x, hipStream_t st) {
    const pie_decoder_config &c = d->cfg;
    if (d->mat_fmt(d->glob.embed_codes) == PIE_W_DENSE) return pie_embedding_dense(ids, M, d->glob.embed_codes, c.vocab, c.hidden, c.dtype, x, st);
    return embedding_launch(ids, M, d->glob.embed_codes, d->glob.embed_scales, d->glob.embed_biases, c.vocab, c.hidden, c.dtype, x, nullptr, nullptr,
                            nullptr, 0, st, d->mat_fmt(d->glob.embed_codes));
}

// The k_rope_append_rows form for a q|k|v projection handed over as fp32 slabs or not, appended to int8 pages or not
template <class T>
static decltype(&k_rope_append_rows<T>) rope_append_kernel(bool slabs, bool i8) {
    if (slabs) return i8 ? &k_rope_append_rows<T, true, true> : &k_rope_append_rows<T, true, false>;
    return i8 ? &k_rope_append_rows<T, false, true> : &k_rope_append_rows<T, false, false>;
}

// Where the M rows of a many-row pass sit and where their K / V go: everything the passes' layer head (qkv_rope_rows) differs in, as data.
struct RowsKv {
    const DecState *state = nullptr;              // positions: row m continues the decoder's one sequence at state->pos + m (cache capacity state->cap) ...
    const int *row_ctx = nullptr;                 // ... or row m sits at row_ctx[m] - 1 of its own sequence (< 0: idle slot)
    const unsigned long long *kv_table = nullptr; // cache: the per-layer K / V buffer (or slab) bases ...
    const void *const *slabs = nullptr;           // ... or every layer's slab directly
    const int *block_tables = nullptr;            // paged KV (nullable): a sequence's table row is bt_stride entries long (0: every row reads the one table)
    int bt_stride = 0, n_pages = 0;
    const int *row_seq = nullptr;                 // row m belongs to sequence row_seq[m] (its block-table row); nullptr: to sequence m
    u16 *kc = nullptr, *vc = nullptr;             // contiguous [n_kv_heads, M, HD] copies of the rotated K and the V rows, where the pass's own attention reads them
    bool i8 = false;                              // the pages are int8 with per-head fp16 scales (paged_i8.hip): K / V are quantised on the way in
    bool gemm_rope = false;                       // the GEMM's own RoPE epilogue (W4mRope) may be offered: it knows neither row_seq nor kc / vc
    bool split_any_rows = false;                  // four workgroups per row of slabs at any row count, not only below 512 (see qkv_rope_rows)
};

// The head of a decoder layer on M rows of s->xn (Attention.__call__ up to the cache update, language.py:75-95): the packed q|k|v Linear, RoPE on
// q / k into s->q and K / V appended where `kv` says -- by the GEMM's own epilogue where it is offered and taken, else by k_rope_append_rows.
template <class T>
static int qkv_rope_rows(pie_decoder *d, const pie_layer_weights &w, int li, int M, const RowsKv &kv, hipStream_t st) {
    const pie_decoder_config &c = d->cfg;
    const int D = c.head_dim, NQKV = (c.n_heads + 2 * c.n_kv_heads) * D;
    PrefillScratch *s = d->prefill;
    W4mRope re = {s->rope_cs, kv.state, kv.row_ctx, kv.kv_table, kv.slabs ? (u16 *)kv.slabs[li] : nullptr, kv.block_tables, kv.bt_stride, kv.n_pages, li,
                  c.n_layers, c.n_heads, c.n_kv_heads, D, c.rope_traditional, s->q, nullptr, kv.i8 ? pie_page_i8_bytes(c.n_kv_heads, D) : (size_t)0};
    RowsOpts qkv_opts;  // q|k|v as the fp32 slabs of a K-split product only without a Linear bias: RoPE takes T(x W^T + b)
    qkv_opts.bias = w.bqkv, qkv_opts.rope = kv.gemm_rope ? &re : nullptr, qkv_opts.slabs = !w.bqkv;
    RowsDone qkv_done;
    if (int rc = linear_rows<T>(d, w.wqkv, NQKV, c.hidden, s->xn, M, s->qkv, st, qkv_opts, &qkv_done)) return rc;
    if (qkv_done.roped) return PIE_OK;
    const W4lSlabs &sq = qkv_done.slabs;
    // few rows of slabs: four workgroups per row (256 tokens: 6.03 vs 6.20 ms; from 512 rows no difference).  The multi-sequence step
    // (split_any_rows) has launched the four at every row count, up to its 4096 sequences: kept as it is, not re-measured from 512.
    const unsigned row_wgs = sq.S > 1 && (M < 512 || kv.split_any_rows) ? 4u : 1u;
    hipLaunchKernelGGL(rope_append_kernel<T>(sq.S > 1, kv.i8), dim3(M, row_wgs), dim3(256), 0, st, s->qkv, NQKV, d->glob.rope_freqs, re.state, re.kv_table,
                       li, c.n_layers, c.n_heads, c.n_kv_heads, D, c.rope_traditional, s->q, re.block_table, re.n_pages, s->rope_cs, re.ctx_len, re.bt_stride,
                       re.slab, kv.row_seq, kv.kc, kv.vc, sq.part, sq.S, sq.MN, re.i8_page_bytes);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// The rest of a decoder layer after its attention, on M rows: o_proj of s->attn, the residual adds on s->x, the MLP in between, and
// the norm that follows the layer into s->xn -- next_norm: the next block's input_layernorm or the final norm (language.py:187);
// nullptr: the layer ends in the plain add and s->xn is left as it is.
template <class T>
static int mlp_rows(pie_decoder *d, const pie_layer_weights &w, int M, const void *next_norm, hipStream_t st) {
    const pie_decoder_config &c = d->cfg;
    const int H = c.hidden, QD = c.n_heads * c.head_dim, I = c.inter;
    PrefillScratch *s = d->prefill;
    RowsDone o_done, gu_done, down_done;
    int rc;
    RowsOpts o_opts;  // o_proj / down handed to their consumers as K-split fp32 slabs where the shape qualifies
    o_opts.bias = w.bo, o_opts.slabs = H <= 8192;
    if ((rc = linear_rows<T>(d, w.wo, H, QD, s->attn, M, s->r, st, o_opts, &o_done))) return rc;
    // h = x + r (language.py:151) + post_attention_layernorm(h) for MLP.__call__ (language.py:126-127)
    if ((rc = add_rms_norm_rows<T>(s->x, s->r, w.mlp_norm, c.rms_eps, M, H, c.dtype, s->xn, st, o_done.slabs.S > 1 ? w.bo : nullptr, &o_done.slabs)))
        return rc;
    RowsOpts gu_opts;
    gu_opts.bias = w.bgateup, gu_opts.act = s->act;
    if ((rc = linear_rows<T>(d, w.wgateup, 2 * I, H, s->xn, M, s->gu, st, gu_opts, &gu_done))) return rc;
    if (!gu_done.fused_swiglu) {
        const size_t n_act = (size_t)M * I;
        hipLaunchKernelGGL(k_swiglu_rows<T>, dim3((unsigned)((n_act / 4 + 255) / 256)), dim3(256), 0, st, s->gu, n_act, s->act);
        PIE_LAUNCH_CHECK();
    }
    RowsOpts down_opts;
    down_opts.bias = w.bdown, down_opts.slabs = next_norm && H <= 8192;
    if ((rc = linear_rows<T>(d, w.wdown, H, I, s->act, M, s->r, st, down_opts, &down_done))) return rc;
    // out = h + r (language.py:153), fused with the norm that follows when there is one
    if (!next_norm) return pie_add(s->x, s->r, (size_t)M * H, c.dtype, s->x, st);
    return add_rms_norm_rows<T>(s->x, s->r, next_norm, c.rms_eps, M, H, c.dtype, s->xn, st, down_done.slabs.S > 1 ? w.bdown : nullptr, &down_done.slabs);
}

// What opens a pass whose M rows are each at their own position: h = embed_tokens(ids) into s->x and the rows' rotary (cos, sin)
static int embed_rope_cs_rows(pie_decoder *d, const int32_t *ids, int M, const int32_t *row_ctx, hipStream_t st) {
    PrefillScratch *s = d->prefill;
    if (int rc = embed_rows(d, ids, M, s->x, st)) return rc;
    hipLaunchKernelGGL(k_rope_cs_rows, dim3(M), dim3(64), 0, st, d->glob.rope_freqs, nullptr, row_ctx, d->cfg.head_dim / 2, s->rope_cs);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// The layers of a pass over M rows on pages (kv.row_ctx: every row at its own position): that opening, then per layer the head, the pass's
// own attention -- attn(li) reads s->q and the cache and writes s->attn -- and the tail.  s->xn ends up holding every row final-normed.
template <class T, class Attn>
static int paged_rows_layers(pie_decoder *d, const int32_t *ids, int M, const RowsKv &kv, hipStream_t st, Attn &&attn) {
    const pie_decoder_config &c = d->cfg;
    PrefillScratch *s = d->prefill;
    int rc = embed_rope_cs_rows(d, ids, M, kv.row_ctx, st);
    if (rc) return rc;
    for (int li = 0; li < c.n_layers; ++li) {
        const pie_layer_weights &w = d->layers[li];
        // input_layernorm: layer 0 here; for the later layers it was fused with the previous block's residual add
        if (li == 0 && (rc = pie_rms_norm(s->x, w.attn_norm, c.rms_eps, M, c.hidden, c.dtype, s->xn, st))) return rc;
        if ((rc = qkv_rope_rows<T>(d, w, li, M, kv, st)) || (rc = attn(li))) return rc;
        if ((rc = mlp_rows<T>(d, w, M, li + 1 < c.n_layers ? d->layers[li + 1].attn_norm : d->glob.final_norm, st))) return rc;
    }
    return PIE_OK;
}

// f(BF16()) or f(F16()) by a decoder's activation dtype (one of the two: pie_decoder_create refuses anything else)
template <class F>
static int for_dtype(int dtype, F &&f) {
    return dtype == PIE_BF16 ? f(BF16()) : f(F16());
}

// Quantized KV (pie_decoder_set_kv_quant): the T scratch of one layer's K and V at the cache's capacity and the table that points every layer at it.
static int kvq_scratch_reserve(pie_decoder *d) {
    const pie_decoder_config &c = d->cfg;
    if (!d->kvq_table) {
        PIE_HIP_TRY(hipMalloc((void **)&d->kvq_table, sizeof(unsigned long long) * 2 * c.n_layers));
    }
    if (d->kvq_scratch_cap == d->kv_cap && d->kvq_scratch) return PIE_OK;  // (rows are kv_cap apart: the layout follows the cache's capacity)
    if (d->kvq_scratch) (void)hipFree(d->kvq_scratch);
    d->kvq_scratch = nullptr, d->kvq_scratch_cap = 0;
    const size_t half = (size_t)c.n_kv_heads * d->kv_cap * c.head_dim;
    PIE_HIP_TRY(hipMalloc((void **)&d->kvq_scratch, 2 * half * 2));
    d->kvq_scratch_cap = d->kv_cap;
    std::vector<unsigned long long> tab(2 * (size_t)c.n_layers);
    for (int i = 0; i < c.n_layers; ++i) tab[i] = (unsigned long long)(uintptr_t)d->kvq_scratch, tab[c.n_layers + i] = tab[i] + half * 2;
    PIE_HIP_TRY(hipMemcpy(d->kvq_table, tab.data(), tab.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    return PIE_OK;
}

// The lm_head on `rows` final-normed rows: through the scratch (no 16-bit resident copy of it); keep_w4m: its int4 tiles stay (the multi-sequence
// passes), where a logits-on-every-position call keeps nothing
template <class T>
static int lm_head_rows(pie_decoder *d, const u16 *x, int rows, void *logits, hipStream_t st, bool keep_w4m = true) {
    RowsOpts o;
    o.keep = false, o.keep_w4m = keep_w4m;
    return linear_rows<T>(d, d->glob.lm_head, d->cfg.vocab, d->cfg.hidden, x, rows, (u16 *)logits, st, o);
}

// Log-probabilities of prompt tokens (pie_decoder_set_prompt_logprobs): rows [0, M) of xn -- final-normed already -- are
// rows row0 .. row0 + M - 1 of the call.  Per block of at most `block` rows: the lm_head as the logits-on-every-position branch multiplies
// it, into the caller's logits block, then the op's launches on that block.  Off: nothing is launched.
template <class T>
static int score_prompt_rows(pie_decoder *d, const u16 *xn, int row0, int M, hipStream_t st) {
    const PromptScores &pl = d->prompt;
    if (!pl.n) return PIE_OK;
    const pie_decoder_config &c = d->cfg;
    for (int b0 = 0; b0 < M; b0 += pl.block) {
        const int rows = M - b0 < pl.block ? M - b0 : pl.block;
        int rc = lm_head_rows<T>(d, xn + (size_t)b0 * c.hidden, rows, pl.ws, st, false);
        if (rc || (rc = pl.score_rows(c, pl.ws, row0 + b0, rows, st))) return rc;
    }
    return PIE_OK;
}

template <class T>
static int prefill_t(pie_decoder *d, const int32_t *ids, const void *embeds, int L, void *logits_all, hipStream_t st) {
    const pie_decoder_config &c = d->cfg;
    const int H = c.hidden, D = c.head_dim;
    const int chunk = prefill_chunk_rows() < L ? prefill_chunk_rows() : L;
    int rc = scratch_reserve(d, chunk, w16_copy_elems(c, logits_all != nullptr || d->prompt.n), d->splits);
    if (rc) return rc;
    PrefillScratch *s = d->prefill;
    // quantized KV: the pass runs on the T scratch (kv_table below), the layer's codes are expanded into it and the chunk's rows quantized back
    if (d->kv_quant && (rc = kvq_scratch_reserve(d))) return rc;
    unsigned long long *const kv_table = d->kv_quant ? d->kvq_table : d->kv_table;
    u16 *const sk = d->kvq_scratch, *const sv = d->kvq_scratch ? d->kvq_scratch + (size_t)c.n_kv_heads * d->kvq_scratch_cap * D : nullptr;
    auto kvq_rows = [&](bool expand, int li, int M) {  // the layer's codes into the scratch / the chunk's M rows quantized back; nothing without quantized KV
        if (!d->kv_quant) return (int)PIE_OK;
        const void *const *p = &d->kvq_host[(size_t)6 * li];
        const QKvLayer q = {(const u32 *)p[0], (const u16 *)p[1], (const u16 *)p[2], (const u32 *)p[3], (const u16 *)p[4], (const u16 *)p[5]};
        return kv_quant_prefill_launch(c.dtype, D, d->kvq_bits, expand, q, d->state, c.n_kv_heads, d->kv_cap, M, d->kvq_gs, sk, sv, st);
    };
    // RotatingKVCache: the chunk's K / V rows go to rows ring_rows->pos + m of the buffers (the retained window in temporal order, then the
    // update: cache/kv_cache/rotating.py), RoPE stays at the absolute position state->pos + m; the attention is windowed
    DecState *const kvs = d->ring ? d->ring_rows : d->state;
    if (d->ring) {  // every pass starts at the row the host bound (pie_decoder_set_kv_ring): the chunk loop below advances it
        PIE_REQUIRE((long long)d->ring_row0 + L <= d->kv_cap, PIE_E_SHAPE, "pie_decoder_prefill: the rotating cache's buffers do not hold the update");
        hipLaunchKernelGGL(k_set_pos, dim3(1), dim3(1), 0, st, d->ring_rows, d->ring_row0);
        PIE_LAUNCH_CHECK();
    }
    const bool mfma_attn = d->ring || pie_knob(PIE_KNOB_PREFILL_ATTN_VALU) != 1;  // 1 forces the row-per-launch-slice VALU kernel (tests compare the two)
    RowsKv kv;  // one sequence: rows at kvs->pos + m of the table's buffers, or of the pages of the decoder's one block table
    kv.state = kvs, kv.kv_table = kv_table, kv.block_tables = d->block_table, kv.n_pages = d->n_pages, kv.gemm_rope = true;
    for (int c0 = 0; c0 < L; c0 += chunk) {
        const int M = L - c0 < chunk ? L - c0 : chunk;
        // h = embed_tokens(inputs)  (language.py:176)
        if (embeds)  // h = inputs_embeds (models/intern/language.py:155-158)
            PIE_HIP_TRY(hipMemcpyAsync(s->x, (const u16 *)embeds + (size_t)c0 * H, (size_t)M * H * 2, hipMemcpyDeviceToDevice, st));
        else if ((rc = embed_rows(d, ids + c0, M, s->x, st)))
            return rc;
        hipLaunchKernelGGL(k_rope_cs_rows, dim3(M), dim3(64), 0, st, d->glob.rope_freqs, d->state, nullptr, D / 2, s->rope_cs);
        PIE_LAUNCH_CHECK();
        for (int li = 0; li < c.n_layers; ++li) {
            const pie_layer_weights &w = d->layers[li];
            // Attention.__call__ (language.py:75-108) on input_layernorm(x)
            // input_layernorm: layer 0 here; for the later layers it was fused with the previous block's residual add
            if (li == 0 && (rc = pie_rms_norm(s->x, w.attn_norm, c.rms_eps, M, H, c.dtype, s->xn, st))) return rc;
            if ((rc = kvq_rows(true, li, M)) || (rc = qkv_rope_rows<T>(d, w, li, M, kv, st)) || (rc = kvq_rows(false, li, M))) return rc;
            if (mfma_attn) {  // causal flash attention on the MFMA units (prefill_attn.hpp)
                PrefillAttnArgs pa = {};
                pa.q = s->q, pa.kv_table = kv_table, pa.layer = li, pa.n_layers = c.n_layers, pa.state = kvs, pa.window = d->ring ? d->ring_w : 0;
                pa.block_table = d->block_table, pa.n_pages = d->n_pages;
                pa.M = M, pa.Hq = c.n_heads, pa.Hkv = c.n_kv_heads, pa.scale = 1.0f / sqrtf((float)D), pa.out = s->attn;
                if ((rc = prefill_attn_launch_t<T>(pa, D, st))) return rc;
            } else {  // PIE_KNOB_PREFILL_ATTN_VALU = 1: the VALU decode kernel, one query row per blockIdx.z (cross-check for the tests)
                AttnArgs a = {};
                a.q = s->q, a.kv_table = kv_table, a.layer = li, a.n_layers = c.n_layers, a.state = d->state;
                a.block_table = d->block_table, a.n_pages = d->n_pages, a.bt_stride = 0;  // every row reads the one sequence's table
                a.Hq = c.n_heads, a.Hkv = c.n_kv_heads, a.splits = d->splits, a.rows = M, a.scale = 1.0f / sqrtf((float)D);
                a.part_acc = s->part_acc, a.part_ml = s->part_ml, a.out = s->attn;
                if ((rc = attn_decode_launch(c.dtype, D, a, true, st))) return rc;
            }
            // the last layer ends in the plain add: the final norm runs below, and only for logits on every position or for scored rows
            if ((rc = mlp_rows<T>(d, w, M, li + 1 < c.n_layers ? d->layers[li + 1].attn_norm : nullptr, st))) return rc;
        }
        if ((logits_all || d->prompt.n) && (rc = pie_rms_norm(s->x, d->glob.final_norm, c.rms_eps, M, H, c.dtype, s->xn, st))) return rc;
        // lm_head on every position, like the reference (language.py:205-209)
        if (logits_all && (rc = lm_head_rows<T>(d, s->xn, M, (u16 *)logits_all + (size_t)c0 * c.vocab, st, false))) return rc;
        if ((rc = score_prompt_rows<T>(d, s->xn, c0, M, st))) return rc;
        const bool last = c0 + M >= L;
        if (last)  // the last position continues through the decode step's lm_head + tail below
            PIE_HIP_TRY(hipMemcpyAsync(d->h, s->x + (size_t)(M - 1) * H, 2 * (size_t)H, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_add_pos, dim3(1), dim3(1), 0, st, d->state, last ? M - 1 : M);
        PIE_LAUNCH_CHECK();
        if (d->ring && !last) {
            hipLaunchKernelGGL(k_add_pos, dim3(1), dim3(1), 0, st, d->ring_rows, M);
            PIE_LAUNCH_CHECK();
        }
    }
    // logits[:, -1, :] -> logprobs -> greedy token; the tail advances the device-side offset past the last prompt token
    if ((rc = enqueue_kernel(d, PIE_K_LMHEAD, 0, nullptr, d->logits, st))) return rc;
    return enqueue_kernel(d, PIE_K_TAIL, 0, nullptr, d->logits, st);
}

// mx.fast.scaled_dot_product_attention(q, k, v, scale, mask=causal) for L > 1 (models/base.py:37-53,111-113), op level.
// The windowed form (RotatingKVCache prompts): query row r sees keys offset + r - window .. offset + r -- create_causal_mask(L, offset,
// window_size=window) in index space (models/base.py:18-34).  Key blocks wholly below a tile's first row's bound are skipped.
// Both entries' body; window 0: the plain causal mask, which `windowed` (the entry that takes a window) refuses.
static int sdpa_prefill(const std::string &who, bool windowed, const void *q, const void *k, const void *v, int Hq, int Hkv, int L, int offset, int cap, int D,
                        int window, float scale, int dtype, void *out, void *stream) {
    PIE_REQUIRE(q && k && v && out, PIE_E_ARG, who + "null pointer");
    PIE_REQUIRE(L >= 1 && offset >= 0 && offset + L <= cap && (!windowed || window >= 1), PIE_E_SHAPE,
                who + (windowed ? "need offset + L <= cap, window >= 1" : "need offset + L <= cap"));
    PIE_REQUIRE(D == 64 || D == 128, PIE_E_SHAPE, who + "head_dim must be 64 or 128");
    PIE_REQUIRE(Hkv > 0 && Hq % Hkv == 0 && Hq / Hkv <= 8, PIE_E_SHAPE, who + "n_heads / n_kv_heads must be between 1 and 8");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(k, 16) && pie_aligned(v, 16) && pie_aligned(out, 8), PIE_E_ALIGN, who + "misaligned pointer");
    PrefillAttnArgs a = {};
    a.q = (const u16 *)q, a.k = (const u16 *)k, a.v = (const u16 *)v, a.offset = offset, a.cap = cap, a.window = window;
    a.M = L, a.Hq = Hq, a.Hkv = Hkv, a.scale = scale, a.out = (u16 *)out;
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, who + "dtype must be PIE_BF16 or PIE_F16");
    return for_dtype(dtype, [&](auto t) { return prefill_attn_launch_t<decltype(t)>(a, D, (hipStream_t)stream); });
}

extern "C" int pie_sdpa_prefill_window(const void *q, const void *k, const void *v, int Hq, int Hkv, int L, int offset, int cap, int D, int window,
                                       float scale, int dtype, void *out, void *stream) {
    return sdpa_prefill("pie_sdpa_prefill_window: ", true, q, k, v, Hq, Hkv, L, offset, cap, D, window, scale, dtype, out, stream);
}

extern "C" int pie_sdpa_prefill(const void *q, const void *k, const void *v, int Hq, int Hkv, int L, int offset, int cap, int D, float scale,
                                int dtype, void *out, void *stream) {
    return sdpa_prefill("pie_sdpa_prefill: ", false, q, k, v, Hq, Hkv, L, offset, cap, D, 0, scale, dtype, out, stream);
}

// attention splits of a batch of B decode rows over block tables of max_blocks pages
static int batch_attn_splits(const pie_decoder *d, int B, int max_blocks) {
    const pie_decoder_config &c = d->cfg;
    // attention splits: enough workgroups for two per CU across the batch, never more than pages per sequence
    int splits = ((d->kv_i8 ? 1024 : 512) + B * c.n_kv_heads - 1) / (B * c.n_kv_heads);  // (the int8-page kernel runs 4-wave workgroups: twice as many)
    splits = splits > ATTN_MAX_SPLITS ? ATTN_MAX_SPLITS : (splits > max_blocks ? max_blocks : splits);
    splits = splits < 1 ? 1 : splits;
    // short sequences (tables of at most 8 pages) in a batch of 64+ (sequence, kv-head) workgroups: one split, and no combine launch
    // (threshold 128 -> 64, i.e. from 8 sequences of the 8B model: 8 / 12 sequences 2.46 / 2.57 -> 2.40 / 2.46 ms at ~170 positions,
    // 2.59 / 2.78 -> 2.57 / 2.61 at ~420; at 48 the 6-sequence step lost 1 % at ~420 positions)
    if (max_blocks <= 8 && B * c.n_kv_heads >= (d->kv_i8 ? 512 : 64)) splits = 1;  // (the int8-page kernel's workgroups are half as wide)
    // a handful of short sequences: one split as well -- the split kernel + its combine launch cost 10.6 us per layer against 5.5 for the
    // batch-1 step's attention, and a few hundred positions are a handful of row blocks per wave
    if (B <= GEMV_ROWS_MAX && max_blocks <= 4 && !d->kv_i8) splits = 1;
    return splits;
}

// The attention of decode-state rows: rows [0, rows) of s->q, each its own sequence (kv.row_ctx[r] positions, block-table row r) over its
// pages of layer li -- which hold the row just appended -- into s->attn
static int paged_decode_attn(pie_decoder *d, int li, int rows, int splits, const RowsKv &kv, hipStream_t st) {
    const pie_decoder_config &c = d->cfg;
    PrefillScratch *s = d->prefill;
    AttnArgs a = {};
    a.q = s->q, a.slab = (const u16 *)kv.slabs[li], a.block_table = kv.block_tables, a.ctx_len = kv.row_ctx, a.bt_stride = kv.bt_stride, a.n_pages = kv.n_pages;
    a.rows = rows, a.Hq = c.n_heads, a.Hkv = c.n_kv_heads, a.splits = splits, a.scale = 1.0f / sqrtf((float)c.head_dim);
    a.nt_kv = (size_t)rows * kv.bt_stride * 64 >= 2048;
    a.part_acc = s->part_acc, a.part_ml = s->part_ml, a.out = s->attn;
    return kv.i8 ? paged_attn_i8_launch(c.dtype, c.head_dim, a, st) : attn_decode_launch(c.dtype, c.head_dim, a, true, st);
}

// ---------------------------------------------------------------- the multi-sequence passes' tail
// What follows the lm_head of `rows` output rows.  No table set: the greedy tail, as ever.  A table (pie_decoder_set_batch_tail):
// every row's own penalty over its own window first (ids / ctx / out_rows: the pass's input ids, context lengths and, where output row s
// is not source row s, its source rows), then the same log-softmax + argmax, then every row's own sampler over the fp32 log-probabilities.
// Per-row edits (pie_decoder_set_batch_logits_edits), with or without a table: every row's own bias behind its penalty, in the
// penalty's launch, and every row's own token mask inside the partials pass of the log-softmax.
// The rows' top-n log-probability records (pie_decoder_set_batch_top_logprobs), once next_tokens are final.  Off: nothing is launched.
static int batch_top_logprobs_launch(pie_decoder *d, int rows, const float *logprobs, const int32_t *next_tokens, hipStream_t st) {
    const RowsTail::Top &t = d->rows.top;
    if (!t.n) return PIE_OK;
    return top_logprobs_launch(logprobs, rows, d->cfg.vocab, t.n, next_tokens, t.count, t.ids, t.vals, t.ws, st);
}

static int batch_tail_launch(pie_decoder *d, const int32_t *ids, const int32_t *ctx, const int32_t *out_rows, int n_src, int rows, u16 *logits,
                             float *logprobs, int32_t *next_tokens, hipStream_t st) {
    const pie_decoder_config &c = d->cfg;
    PrefillScratch *s = d->prefill;
    const RowsTail &r = d->rows;
    int rc;
    // The six stages of configured_tail (decoder.hip), per row; with nothing configured only the partials and the finish run.
    // token automata: the armed rows' masks and mask_on entries come first, written into the edits' mask part (check_rows: set)
    if (r.dfa.records && (rc = token_dfa_mask_launch(r.dfa.records, r.dfa.states, r.dfa.tables, r.dfa.tables_len, rows, c.vocab, const_cast<unsigned *>(r.edits.masks),
                                                     r.edits.mask_words, const_cast<int *>(r.edits.mask_on), st))) return rc;
    if (r.sampler.table || r.edits.bias_cap) {  // edit: the rows' biases ride the penalty's launch (k_logits_edit_rows: no penalties without a table)
        PenRowsArgs p = {};
        p.logits = logits, p.V = c.vocab, p.n_src = n_src, p.table = r.sampler.table, p.recent = r.sampler.recent, p.ids = ids, p.ctx = ctx, p.out_rows = out_rows;
        const BiasRowsArgs b = {r.edits.bias_ids, r.edits.bias_vals, r.edits.bias_n, r.edits.bias_cap, r.sampler.table ? 1 : 0};
        if ((rc = r.edits.bias_cap ? logits_edit_rows_launch(c.dtype, p, b, rows, st) : logits_penalty_rows_launch(c.dtype, p, rows, st))) return rc;
    }
    if (r.counts.records) {  // count penalty: behind the row's penalty and its bias
        CountPenArgs k = {};
        k.logits = logits, k.V = c.vocab, k.n_src = n_src, k.records = r.counts.records, k.counts = r.counts.counts, k.ids = ids, k.ctx = ctx, k.out_rows = out_rows;
        if ((rc = logits_count_penalty_rows_launch(c.dtype, k, rows, st))) return rc;
    }
    if (r.dry.records) {  // DRY: behind the count penalty, over the rows' own rings
        DryRowsArgs k = {};
        k.r.logits = logits, k.r.V = c.vocab, k.r.n_src = n_src, k.r.recent = r.dry.recent, k.r.ids = ids, k.r.ctx = ctx, k.r.out_rows = out_rows;
        k.records = r.dry.records, k.breakers = r.dry.breakers;
        if ((rc = logits_dry_rows_launch(c.dtype, k, rows, st))) return rc;
    }
    // partials and finish: the rows' masks ride the partials pass -- physically last, so a masked id is -inf whatever else is configured
    if ((rc = logits_tail_rows_launch(c.dtype, logits, c.vocab, rows, s->tail_stats, logprobs, next_tokens, st, r.edits.masks, r.edits.mask_words, r.edits.mask_on))) return rc;
    // sampler and top-n
    if (r.sampler.table && (rc = sample_rows_launch(logprobs, rows, c.vocab, r.sampler.table, r.sampler.ws, next_tokens, nullptr, nullptr, st,
                                                     SampleXtc{r.xtc.records, nullptr}))) return rc;
    if ((rc = batch_top_logprobs_launch(d, rows, logprobs, next_tokens, st))) return rc;
    if (!r.dfa.records) return PIE_OK;
    // last: every armed row's state moves by the token it drew
    return token_dfa_advance_launch(r.dfa.records, r.dfa.states, r.dfa.tables, r.dfa.tables_len, rows, c.vocab, next_tokens, st);
}

// ---------------------------------------------------------------- one decode step for B sequences (continuous batching)
// The weights stream once for all B rows (linear_rows: up to 5 rows the streaming GEMV where the format has one, beyond that int4 matrices
// on their W4M tiles and the others on the W16M copy + k_w16l_gemm); each row is its own sequence: RoPE at its own position, K/V appended
// to its own page, attention over its own block table (k_attn_decode PAGED, one sequence per blockIdx.z), lm_head + tail on every row.
// What the reference's Scheduler / BatchDetails / PagedAttention skeleton (src/pie_core/include/engine/batch_details.hpp:10-88,
// scheduler.hpp) describes for decode-state sequences.
template <class T>
static int decode_batch_t(pie_decoder *d, const int32_t *tokens, const int32_t *ctx_len, const void *const *slabs, int n_pages,
                          const int32_t *block_tables, int max_blocks, int B, u16 *logits, float *logprobs, int32_t *next_tokens, hipStream_t st) {
    const pie_decoder_config &c = d->cfg;
    const int H = c.hidden, D = c.head_dim, QD = c.n_heads * D, KVD = c.n_kv_heads * D, NQKV = QD + 2 * KVD, I = c.inter;
    const int splits = batch_attn_splits(d, B, max_blocks);
    int rc = scratch_reserve(d, B, w16_copy_elems(c, true), splits > d->splits ? splits : d->splits);
    if (rc) return rc;
    PrefillScratch *s = d->prefill;
    const int lm_waves = w4s_gemv_waves(c.vocab, H);  // the fused few-sequence form: one log-softmax partial per GEMV wave and row
    const size_t stats_per_row = (size_t)(lm_waves > TAIL_STAT_TILES ? lm_waves : TAIL_STAT_TILES);
    if ((rc = tail_stats_reserve(s, stats_per_row * (size_t)B))) return rc;
    RowsKv kv;  // every row its own sequence: its own position, page (T or int8: the append quantises) and block-table row
    kv.row_ctx = ctx_len, kv.slabs = slabs, kv.block_tables = block_tables, kv.bt_stride = max_blocks, kv.n_pages = n_pages, kv.i8 = d->kv_i8;
    kv.gemm_rope = true, kv.split_any_rows = true;
    // Up to 5 sequences on an int4 checkpoint: the batch-1 launch sequence, once, with every GEMV multiplying all rows per weight
    // unit (k_w4s_gemv_rows: RMSNorm prologues; RoPE + page append, residual, SwiGLU and logits epilogues, per row) -- 6 launches per
    // layer instead of 9-10, each row in MLX's row-by-row fp32 regime.  Biases, int8 pages and hidden sizes beyond 8192 take the
    // general path below.
    bool fused_rows = B <= GEMV_ROWS_MAX && d->uniform_int4() && !d->kv_i8 && H <= 8192 && lm_waves <= TAIL_MAX_STATS;
    for (const pie_layer_weights &w : d->layers)
        if (w.bqkv || w.bo || w.bgateup || w.bdown) fused_rows = false;
    if (fused_rows) {
        if ((rc = embed_rope_cs_rows(d, tokens, B, ctx_len, st))) return rc;
        for (int li = 0; li < c.n_layers; ++li) {
            const pie_layer_weights &w = d->layers[li];
            GemvRowsArgs g = {};
            g.w = (const char *)w.wqkv, g.K = H, g.N = NQKV, g.M = B, g.x = s->x, g.norm_w = (const u16 *)w.attn_norm, g.eps = c.rms_eps;
            g.rope_cs = s->rope_cs, g.ctx_len = ctx_len, g.block_table = block_tables, g.slab = (u16 *)slabs[li], g.q_out = s->q;
            g.bt_stride = max_blocks, g.n_pages = n_pages, g.n_heads = c.n_heads, g.n_kv_heads = c.n_kv_heads, g.head_dim = D, g.rope_traditional = c.rope_traditional;
            if ((rc = w4s_gemv_rows_fused_launch(c.dtype, PRO_RMSNORM, EPI_ROPE_KV, g, st))) return rc;
            if ((rc = paged_decode_attn(d, li, B, splits, kv, st))) return rc;
            g = GemvRowsArgs();
            g.w = (const char *)w.wo, g.K = QD, g.N = H, g.M = B, g.x = s->attn, g.resid = s->x;
            if ((rc = w4s_gemv_rows_fused_launch(c.dtype, PRO_NONE, EPI_RESIDUAL, g, st))) return rc;
            g = GemvRowsArgs();
            g.w = (const char *)w.wgateup, g.K = H, g.N = 2 * I, g.M = B, g.x = s->x, g.norm_w = (const u16 *)w.mlp_norm, g.eps = c.rms_eps, g.y = s->act;
            if ((rc = w4s_gemv_rows_fused_launch(c.dtype, PRO_RMSNORM, EPI_SWIGLU, g, st))) return rc;
            g = GemvRowsArgs();
            g.w = (const char *)w.wdown, g.K = I, g.N = H, g.M = B, g.x = s->act, g.resid = s->x;
            if ((rc = w4s_gemv_rows_fused_launch(c.dtype, PRO_NONE, EPI_RESIDUAL, g, st))) return rc;
        }
        GemvRowsArgs g = {};
        g.w = (const char *)d->glob.lm_head, g.K = H, g.N = c.vocab, g.M = B, g.x = s->x, g.norm_w = (const u16 *)d->glob.final_norm, g.eps = c.rms_eps;
        g.y = logits, g.stats = s->tail_stats;
        if ((rc = w4s_gemv_rows_fused_launch(c.dtype, PRO_RMSNORM, EPI_LOGITS, g, st))) return rc;
        if (d->rows.edits_logits()) return batch_tail_launch(d, tokens, ctx_len, nullptr, B, B, logits, logprobs, next_tokens, st);  // (the epilogue's partials are stale after a penalty or an edit)
        if ((rc = logits_finish_launch(c.dtype, logits, c.vocab, B, s->tail_stats, lm_waves, logprobs, next_tokens, nullptr, nullptr, 0, nullptr, st))) return rc;
        return batch_top_logprobs_launch(d, B, logprobs, next_tokens, st);
    }
    if ((rc = paged_rows_layers<T>(d, tokens, B, kv, st, [&](int li) { return paged_decode_attn(d, li, B, splits, kv, st); }))) return rc;
    if ((rc = lm_head_rows<T>(d, s->xn, B, logits, st))) return rc;
    return batch_tail_launch(d, tokens, ctx_len, nullptr, B, B, logits, logprobs, next_tokens, st);
}

// ---------------------------------------------------------------- several fresh prompts in one pass
__global__ void k_gather_rows(const uint4 *x, const int *rows, int H8, uint4 *y) {  // y[s] = x[rows[s]], H8 = hidden / 8
    const uint4 *src = x + (size_t)rows[blockIdx.x] * H8;
    for (int i = threadIdx.x; i < H8; i += blockDim.x) y[(size_t)blockIdx.x * H8 + i] = src[i];
}

// The rows of S prompts concatenated ([N] ids): one pass of GEMMs over all N rows, RoPE at each row's own position, K / V into
// each prompt's own pages AND a contiguous copy the attention of this pass reads (causal inside each prompt = the segment
// kernel with seg_hi[r] = r + 1), lm_head + tail on every prompt's last row.  Fresh prompts only (nothing cached before them).
// n_decode > 0 (a mixed batch, batch_details.hpp:10-88's prefill- and decode-state sequences in one BatchDetails): rows
// [0, n_decode) are decode-state sequences -- row r is sequence r (row_seq[r] == r, block-table row r) at position
// row_ctx[r] - 1 with a trivial segment [r, r + 1) -- whose attention then runs over their pages (the multi-sequence step's
// paged kernel) and replaces the segment kernel's rows; the prompt rows follow.  One pass over the weights for both kinds.
template <class T>
static int prefill_varlen_t(pie_decoder *d, const int32_t *ids, const int32_t *row_ctx, const int32_t *row_seq, const int32_t *seg_lo,
                            const int32_t *seg_hi, const int32_t *last_rows, int N, int S, int n_decode, const void *const *slabs, int n_pages,
                            const int32_t *block_tables, int max_blocks, u16 *logits, float *logprobs, int32_t *next_tokens, hipStream_t st,
                            int n_chunks = 0, const int32_t *chunks = nullptr) {
    const pie_decoder_config &c = d->cfg;
    const int H = c.hidden, D = c.head_dim, QD = c.n_heads * D;
    const int dsplits = n_decode > 0 ? batch_attn_splits(d, n_decode, max_blocks) : 1;
    int rc = scratch_reserve(d, N > S ? N : S, w16_copy_elems(c, true), dsplits > d->splits ? dsplits : d->splits);
    if (rc) return rc;
    PrefillScratch *s = d->prefill;
    if ((rc = tail_stats_reserve(s, (size_t)TAIL_STAT_TILES * (size_t)S))) return rc;
    RowsKv kv;  // rows of a sequence share its block-table row; K / V also go to the contiguous copies this pass's own attention reads
    kv.row_ctx = row_ctx, kv.slabs = slabs, kv.block_tables = block_tables, kv.bt_stride = max_blocks, kv.n_pages = n_pages, kv.i8 = d->kv_i8;
    kv.row_seq = row_seq, kv.kc = s->kc, kv.vc = s->vc;
    rc = paged_rows_layers<T>(d, ids, N, kv, st, [&](int li) {
        PrefillAttnArgs pa = {};
        pa.q = s->q, pa.k = s->kc, pa.v = s->vc, pa.offset = 0, pa.cap = N, pa.seg_lo = seg_lo, pa.seg_hi = seg_hi;
        pa.M = N, pa.Hq = c.n_heads, pa.Hkv = c.n_kv_heads, pa.scale = 1.0f / sqrtf((float)D), pa.out = s->attn;
        int rc = segment_attn_gqa_launch_t<T>(pa, D, st);
        // the decode-state rows attend to their pages (which hold the row just appended)
        if (!rc && n_decode > 0) rc = paged_decode_attn(d, li, n_decode, dsplits, kv, st);
        for (int ci = 0; ci < n_chunks && !rc; ++ci) {  // prompts continuing a cached prefix: causal attention over their pages from the cached length
            const int32_t *ch = chunks + 4 * ci;
            PrefillAttnArgs ca = {};
            ca.q = s->q + (size_t)ch[0] * QD, ca.out = s->attn + (size_t)ch[0] * QD;
            ca.k = (const u16 *)slabs[li], ca.v = (const u16 *)slabs[li] + (size_t)c.n_kv_heads * PIE_PAGE_TOKENS * D;
            ca.offset = ch[2], ca.cap = PIE_PAGE_TOKENS, ca.block_table = block_tables + (size_t)ch[3] * max_blocks, ca.n_pages = n_pages;
            ca.M = ch[1], ca.Hq = c.n_heads, ca.Hkv = c.n_kv_heads, ca.scale = pa.scale;
            rc = prefill_attn_launch_t<T>(ca, D, st);
        }
        return rc;
    });
    if (rc) return rc;
    // the normalised last row of every prompt -> lm_head -> tail
    hipLaunchKernelGGL(k_gather_rows, dim3(S), dim3(256), 0, st, (const uint4 *)s->xn, last_rows, H / 8, (uint4 *)s->r);
    PIE_LAUNCH_CHECK();
    if ((rc = lm_head_rows<T>(d, s->r, S, logits, st))) return rc;
    if ((rc = batch_tail_launch(d, ids, row_ctx, last_rows, N, S, logits, logprobs, next_tokens, st))) return rc;
    // the prompt rows' own records (pie_decoder_set_prompt_logprobs): s->xn still holds every row final-normed; the decode rows are not scored
    return score_prompt_rows<T>(d, s->xn + (size_t)n_decode * H, n_decode, N - n_decode, st);
}

// ---------------------------------------------------------------- what the page-pool entries refuse alike
// bytes one page of the active format takes in a layer's slab: K block + V block of T rows, or the int8 page with its scales
static size_t active_page_bytes(const pie_decoder *d) {
    const pie_decoder_config &c = d->cfg;
    return d->kv_i8 ? pie_page_i8_bytes(c.n_kv_heads, c.head_dim) : (size_t)2 * PIE_PAGE_TOKENS * c.n_kv_heads * c.head_dim * 2;
}

static const char *const SLABS_BELOW_ACTIVE_FORMAT =
    "the slabs are smaller than n_pages pages of the active page format (an int8 pool needs PIE_OPT_KV_I8, a T pool must not have it)";

// The six refusals that pie_decoder_step_batch, pie_decoder_prefill_batch / _step_mixed and pie_decoder_spec_step_batch share, each written once.  An entry
// fills the record and runs them as check(first, last) in the order it always made them, its own checks between them where they always stood: a call
// that breaks two rules still reports the same one.
enum PoolCheck { POOL_GLOBALS, POOL_LAYERS, POOL_SHAPE, POOL_SLAB_BYTES, POOL_HEAD_RATIO, POOL_SLABS };
struct PoolRefusals {
    const pie_decoder *d;
    std::string who;                   // the entry's prefix ("...: ")
    const void *const *slabs;          // the caller's pool: one slab of slab_bytes per layer holding n_pages pages, block tables of max_blocks entries
    size_t n_pages, slab_bytes;
    int max_blocks;
    bool rows_ok;                      // the entry's row limits: refused together with the pool's size, as shape_msg
    const char *shape_msg, *slab_msg;  // ... and the entry's wording of the slab_bytes refusal
    int check(int first, int last) const {
        for (int k = first; k <= last; ++k) {
            if (k == POOL_GLOBALS) PIE_REQUIRE(d->glob_set, PIE_E_STATE, who + "set_globals must be called first");
            if (k == POOL_LAYERS)
                for (char s : d->layer_set) PIE_REQUIRE(s, PIE_E_STATE, who + "a layer has no weights (pie_decoder_set_layer)");
            if (k == POOL_SHAPE) PIE_REQUIRE(rows_ok && max_blocks > 0 && n_pages > 0 && n_pages < 0x7FFFFFFFu, PIE_E_SHAPE, who + shape_msg);
            if (k == POOL_SLAB_BYTES) PIE_REQUIRE(slab_bytes >= n_pages * active_page_bytes(d), PIE_E_SHAPE, who + slab_msg);
            if (k == POOL_HEAD_RATIO) {
                const int rep = d->cfg.n_heads / d->cfg.n_kv_heads;
                PIE_REQUIRE(rep >= 1 && rep <= 8, PIE_E_SHAPE, who + "n_heads / n_kv_heads must be between 1 and 8");
            }
            if (k == POOL_SLABS)
                for (int i = 0; i < d->cfg.n_layers; ++i) PIE_REQUIRE(slabs[i] && pie_aligned(slabs[i], 16), PIE_E_ALIGN, who + "null or misaligned slab");
        }
        return PIE_OK;
    }
};

static int varlen_batch(pie_decoder *d, const int32_t *ids, const int32_t *row_context_lens, const int32_t *row_seq, const int32_t *seg_lo,
                        const int32_t *seg_hi, const int32_t *last_rows, int N, int S, int n_decode, const void *const *slabs, size_t n_pages, size_t slab_bytes,
                        const int32_t *block_tables, int max_blocks, void *logits, float *logprobs, int32_t *next_tokens, void *stream, int n_chunks = 0,
                        const int32_t *chunks = nullptr) {
    PIE_REQUIRE(d && ids && row_context_lens && row_seq && seg_lo && seg_hi && last_rows && slabs && block_tables && logits && logprobs && next_tokens,
                PIE_E_ARG, "pie_decoder_prefill_batch / _step_mixed: null pointer");
    PIE_REQUIRE(n_chunks >= 0 && (n_chunks == 0 || chunks), PIE_E_ARG, "pie_decoder_step_mixed: chunks without their descriptor array");
    PIE_REQUIRE(n_chunks == 0 || !d->kv_i8, PIE_E_STATE, "pie_decoder_step_mixed: a prompt continuing a cached prefix reads T pages (int8 pages: fresh prompts and decode rows only)");
    for (int ci = 0; ci < n_chunks; ++ci) {
        const int32_t *ch = chunks + 4 * ci;
        PIE_REQUIRE(ch[0] >= n_decode && ch[1] >= 1 && ch[0] + ch[1] <= N && ch[2] >= 1 && ch[3] >= 0 && ch[3] < S &&
                        (ch[2] + ch[1] + PIE_PAGE_TOKENS - 1) / PIE_PAGE_TOKENS <= max_blocks,
                    PIE_E_SHAPE, "pie_decoder_step_mixed: a chunk is {first row >= n_decode, rows >= 1, cached positions >= 1, sequence < S} inside the batch and its block table");
    }
    const PoolRefusals shared = {d, "pie_decoder_prefill_batch / _step_mixed: ", slabs, n_pages, slab_bytes, max_blocks, S >= 1 && N >= S && N <= 65535,
                                 "bad batch shape", SLABS_BELOW_ACTIVE_FORMAT};
    if (int rc = shared.check(POOL_GLOBALS, POOL_LAYERS)) return rc;
    if (int rc = d->rows.check_rows(S, "pie_decoder_prefill_batch / _step_mixed")) return rc;
    PIE_REQUIRE(!d->prompt.n || N <= d->prompt.rows_cap, PIE_E_SHAPE, shared.who + "more rows than the prompt log-probabilities' rows_cap");
    PIE_REQUIRE(!d->rows.top.n || pie_aligned(logprobs, 4), PIE_E_ALIGN, shared.who + "logprobs need 4-byte alignment");
    if (int rc = shared.check(POOL_SHAPE, POOL_SLAB_BYTES)) return rc;
    PIE_REQUIRE(d->cfg.hidden % 8 == 0 && d->cfg.hidden <= 8192, PIE_E_SHAPE, shared.who + "hidden must be a multiple of 8, at most 8192");
    if (int rc = shared.check(POOL_HEAD_RATIO, POOL_SLABS)) return rc;
    return for_dtype(d->cfg.dtype, [&](auto t) {
        return prefill_varlen_t<decltype(t)>(d, ids, row_context_lens, row_seq, seg_lo, seg_hi, last_rows, N, S, n_decode, slabs, (int)n_pages, block_tables,
                                             max_blocks, (u16 *)logits, logprobs, next_tokens, (hipStream_t)stream, n_chunks, chunks);
    });
}

extern "C" int pie_decoder_prefill_batch(pie_decoder *d, const int32_t *ids, const int32_t *row_context_lens, const int32_t *row_seq,
                                         const int32_t *seg_lo, const int32_t *seg_hi, const int32_t *last_rows, int N, int S,
                                         const void *const *slabs, size_t n_pages, size_t slab_bytes, const int32_t *block_tables, int max_blocks, void *logits,
                                         float *logprobs, int32_t *next_tokens, void *stream) {
    return varlen_batch(d, ids, row_context_lens, row_seq, seg_lo, seg_hi, last_rows, N, S, 0, slabs, n_pages, slab_bytes, block_tables,
                        max_blocks, logits, logprobs, next_tokens, stream);
}

extern "C" int pie_decoder_step_mixed(pie_decoder *d, const int32_t *ids, const int32_t *row_context_lens, const int32_t *row_seq,
                                      const int32_t *seg_lo, const int32_t *seg_hi, const int32_t *out_rows, int N, int S, int n_decode,
                                      const void *const *slabs, size_t n_pages, size_t slab_bytes, const int32_t *block_tables, int max_blocks, void *logits,
                                      float *logprobs, int32_t *next_tokens, int n_chunks, const int32_t *chunks_host, void *stream) {
    PIE_REQUIRE(n_decode >= 0 && n_decode <= S, PIE_E_SHAPE, "pie_decoder_step_mixed: n_decode must be between 0 and the number of output rows");
    return varlen_batch(d, ids, row_context_lens, row_seq, seg_lo, seg_hi, out_rows, N, S, n_decode, slabs, n_pages, slab_bytes, block_tables,
                        max_blocks, logits, logprobs, next_tokens, stream, n_chunks, chunks_host);
}

// ---------------------------------------------------------------- one speculative pass for B decode-state sequences
// Sequence s presents 1 + m_s consecutive rows (segment s of seg_first): its fed token, then its drafts.  The pass is the several-prompts
// pass's body on those N rows -- embed, linear_rows / mlp_rows, RoPE + append into each sequence's own pages -- with ONE attention launch
// per layer for all segments (paged_attn_verify.hip) where that pass runs a segment kernel and a launch per chunk, the lm_head on ALL N
// rows (s->xn holds them final-normed, in row order: nothing to gather) and the segmented verify behind it.
template <class T>
static int spec_batch_t(pie_decoder *d, const int32_t *fed, const int32_t *row_ctx, const int32_t *row_seq, const int32_t *seg_first, int N, int B,
                        const void *const *slabs, int n_pages, const int32_t *block_tables, int max_blocks, u16 *logits, hipStream_t st) {
    const pie_decoder_config &c = d->cfg;
    const int D = c.head_dim;
    const int splits = paged_attn_verify_splits(B, c.n_kv_heads, max_blocks);
    int rc = scratch_reserve(d, N, w16_copy_elems(c, true), splits > d->splits ? splits : d->splits);
    if (rc) return rc;
    PrefillScratch *s = d->prefill;
    RowsKv kv;  // rows of a sequence share its block-table row; T pages only (the entry refuses int8 pages)
    kv.row_ctx = row_ctx, kv.slabs = slabs, kv.block_tables = block_tables, kv.bt_stride = max_blocks, kv.n_pages = n_pages, kv.row_seq = row_seq;
    rc = paged_rows_layers<T>(d, fed, N, kv, st, [&](int li) {
        VerifyAttnArgs a = {};  // every row attends its sequence's pages, which now hold the pass's own rows
        a.q = s->q, a.slab = (const u16 *)slabs[li], a.block_table = block_tables, a.row_seq = row_seq, a.row_ctx = row_ctx, a.seg_first = seg_first;
        a.N = N, a.B = B, a.Hq = c.n_heads, a.Hkv = c.n_kv_heads, a.bt_stride = max_blocks, a.n_pages = n_pages, a.splits = splits;
        a.scale = 1.0f / sqrtf((float)D), a.part_acc = s->part_acc, a.part_ml = s->part_ml, a.out = s->attn;
        return paged_attn_verify_launch(c.dtype, D, a, st);
    });
    if (rc) return rc;
    return lm_head_rows<T>(d, s->xn, N, logits, st);
}

// What pie_decoder_spec_step_batch and pie_decoder_spec_step_batch_tail share: the entry's refusals -- with_tail: which parts of the batch
// tail the pass admits is RowsTail's answer (decoder.hpp) --, the pool's, shape and alignment checks, the workspace's carve-up (the logits
// block at its head, then *fed, then *verify_ws), the gather of the input rows and the pass itself, raw logits on every row.
static int spec_batch_body(const std::string &who, bool with_tail, pie_decoder *d, const int32_t *tokens, const int32_t *draft_ids, int draft_stride,
                           const int32_t *row_context_lens, const int32_t *row_seq, const int32_t *seg_first, int N, int B, const void *const *slabs, size_t n_pages,
                           size_t slab_bytes, const int32_t *block_tables, int max_blocks, int32_t *out_tokens, int32_t *out_n, float *logprobs, int32_t *seq_ids,
                           int32_t *seq_len, int seq_cap, void *workspace, hipStream_t st, int **fed_out, void **verify_ws) {
    PIE_REQUIRE(d && tokens && draft_ids && row_context_lens && row_seq && seg_first && slabs && block_tables && out_tokens && out_n && (logprobs || !with_tail) && workspace,
                PIE_E_ARG, who + "null pointer");
    PIE_REQUIRE((seq_ids == nullptr) == (seq_len == nullptr) && (seq_ids ? seq_cap >= 1 : seq_cap == 0), PIE_E_ARG,
                who + "seq_ids [B, seq_cap >= 1] and seq_len come together or not at all");
    PIE_REQUIRE(!d->tp(), PIE_E_STATE, who + "not available on a tensor-parallel shard");
    PIE_REQUIRE(!d->kv_i8, PIE_E_STATE, who + "not available on int8 KV pages");
    const char *part = with_tail ? d->rows.spec_tail_refused() : d->rows.spec_refused();
    PIE_REQUIRE(!part, PIE_E_STATE, who + "not available with " + part);
    PIE_REQUIRE(!d->prompt.n, PIE_E_STATE, who + "not available with prompt scoring");
    PIE_REQUIRE(!with_tail || d->rows.sampler.table, PIE_E_STATE, who + "no batch tail is set (the greedy and raw pass is pie_decoder_spec_step_batch)");
    const PoolRefusals shared = {d, who, slabs, n_pages, slab_bytes, max_blocks, B >= 1 && N >= B && N <= SPEC_BATCH_ROWS && N <= SPEC_SEG_ROWS * B && draft_stride >= 1,
                                 "need 1 <= B <= N <= min(256, 8 B) rows, draft_stride >= 1 and a page pool", "the slabs are smaller than n_pages T pages"};
    if (int rc = shared.check(POOL_GLOBALS, POOL_SLAB_BYTES)) return rc;
    if (with_tail)  // record, ring, bias entries and XTC record s belong to sequence s: every configured part holds B of them
        if (int rc = d->rows.check_rows(B, "pie_decoder_spec_step_batch_tail")) return rc;
    PIE_REQUIRE(d->cfg.hidden % 8 == 0 && d->cfg.hidden <= 8192, PIE_E_SHAPE, who + "hidden must be a multiple of 8, at most 8192");
    PIE_REQUIRE(d->cfg.head_dim == 64 || d->cfg.head_dim == 128, PIE_E_SHAPE, who + "head_dim must be 64 or 128");
    // this entry's ratio must also be whole: refused in the words of the shared check right behind it
    PIE_REQUIRE(d->cfg.n_heads % d->cfg.n_kv_heads == 0, PIE_E_SHAPE, who + "n_heads / n_kv_heads must be between 1 and 8");
    if (int rc = shared.check(POOL_HEAD_RATIO, POOL_HEAD_RATIO)) return rc;
    PIE_REQUIRE(pie_aligned(tokens, 4) && pie_aligned(draft_ids, 4) && pie_aligned(row_context_lens, 4) && pie_aligned(row_seq, 4) && pie_aligned(seg_first, 4) &&
                    pie_aligned(block_tables, 4) && pie_aligned(out_tokens, 4) && pie_aligned(out_n, 4) && pie_aligned(logprobs, 4) && pie_aligned(seq_ids, 4) &&
                    pie_aligned(seq_len, 4),
                PIE_E_ALIGN, who + "4-byte alignment required");
    PIE_REQUIRE(pie_aligned(workspace, 16), PIE_E_ALIGN, who + "workspace needs 16-byte alignment");
    PIE_REQUIRE(!with_tail || pie_sample_workspace_bytes(SPEC_BATCH_ROWS, d->cfg.vocab) != 0, PIE_E_SHAPE, who + "the vocabulary is larger than the sampler takes (524288)");
    if (int rc = shared.check(POOL_SLABS, POOL_SLABS)) return rc;
    const int V = d->cfg.vocab;
    u16 *logits = (u16 *)workspace;
    const SpecPassLayout lay(SPEC_BATCH_ROWS, SPEC_BATCH_ROWS, V);
    int *fed = (int *)((char *)workspace + lay.fed);
    *fed_out = fed, *verify_ws = (char *)workspace + lay.verify;
    // a row no segment covers is fed id 0 (seg_first is device memory: nothing here can check it)
    PIE_HIP_TRY(hipMemsetAsync(fed, 0, sizeof(int) * (size_t)N, st));
    if (int rc = spec_gather_rows_launch(tokens, draft_ids, draft_stride, seg_first, B, N, d->embed_vocab(), fed, st)) return rc;
    return for_dtype(d->cfg.dtype, [&](auto t) {
        return spec_batch_t<decltype(t)>(d, fed, row_context_lens, row_seq, seg_first, N, B, slabs, (int)n_pages, block_tables, max_blocks, logits, st);
    });
}

// workspace (SpecPassLayout): the logits block [256, vocab] T | the pass's input ids [256] | pie_spec_verify_rows' workspace for 256 rows
extern "C" size_t pie_decoder_spec_batch_workspace_bytes(const pie_decoder *d) {
    return d ? SpecPassLayout(SPEC_BATCH_ROWS, SPEC_BATCH_ROWS, d->cfg.vocab).bytes(pie_spec_verify_rows_workspace_bytes(SPEC_BATCH_ROWS)) : 0;
}

extern "C" int pie_decoder_spec_step_batch(pie_decoder *d, const int32_t *tokens, const int32_t *draft_ids, int draft_stride, const int32_t *row_context_lens,
                                           const int32_t *row_seq, const int32_t *seg_first, int N, int B, const void *const *slabs, size_t n_pages,
                                           size_t slab_bytes, const int32_t *block_tables, int max_blocks, int32_t *out_tokens, int32_t *out_n, int32_t *seq_ids,
                                           int32_t *seq_len, int seq_cap, void *workspace, void *stream) {
    int *fed;
    void *verify_ws;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = spec_batch_body("pie_decoder_spec_step_batch: ", false, d, tokens, draft_ids, draft_stride, row_context_lens, row_seq, seg_first, N, B, slabs, n_pages,
                                 slab_bytes, block_tables, max_blocks, out_tokens, out_n, nullptr, seq_ids, seq_len, seq_cap, workspace, st, &fed, &verify_ws))
        return rc;
    return spec_verify_rows_launch((const u16 *)workspace, N, d->cfg.vocab, d->cfg.dtype, seg_first, B, draft_ids, draft_stride, out_tokens, out_n, seq_ids, seq_len, seq_cap,
                                   verify_ws, st);
}

// workspace (SpecPassLayout): the logits block [256, vocab] T | the pass's input ids [256] | pie_spec_verify_rows_sampled's workspace for 256 rows (zeroed once)
extern "C" size_t pie_decoder_spec_batch_tail_workspace_bytes(const pie_decoder *d) {
    return d ? SpecPassLayout(SPEC_BATCH_ROWS, SPEC_BATCH_ROWS, d->cfg.vocab).bytes(pie_spec_verify_rows_sampled_workspace_bytes(SPEC_BATCH_ROWS, d->cfg.vocab)) : 0;
}

// The pass under the seats' own tails: the same body, then the batch tail's records and rings, the batch edits' bias part
// and the batch XTC records applied to every segment's rows, and moved by what the pass accepted (speculative.hip).
extern "C" int pie_decoder_spec_step_batch_tail(pie_decoder *d, const int32_t *tokens, const int32_t *draft_ids, int draft_stride, const int32_t *row_context_lens,
                                                const int32_t *row_seq, const int32_t *seg_first, int N, int B, const void *const *slabs, size_t n_pages,
                                                size_t slab_bytes, const int32_t *block_tables, int max_blocks, int32_t *out_tokens, int32_t *out_n, float *logprobs,
                                                int32_t *seq_ids, int32_t *seq_len, int seq_cap, void *workspace, void *stream) {
    int *fed;
    void *verify_ws;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = spec_batch_body("pie_decoder_spec_step_batch_tail: ", true, d, tokens, draft_ids, draft_stride, row_context_lens, row_seq, seg_first, N, B, slabs, n_pages,
                                 slab_bytes, block_tables, max_blocks, out_tokens, out_n, logprobs, seq_ids, seq_len, seq_cap, workspace, st, &fed, &verify_ws))
        return rc;
    const RowsTail &t = d->rows;
    SpecSeats q;
    q.table = t.sampler.table, q.recent = t.sampler.recent, q.row_ctx = row_context_lens, q.xtc = t.xtc.records;
    if (t.edits.rows_cap && t.edits.bias_cap) q.bias_ids = t.edits.bias_ids, q.bias_vals = t.edits.bias_vals, q.bias_n = t.edits.bias_n, q.bias_cap = t.edits.bias_cap;
    return spec_verify_rows_sampled_launch(q, (u16 *)workspace, N, d->cfg.vocab, d->cfg.dtype, seg_first, B, fed, draft_ids, draft_stride, out_tokens, out_n, logprobs,
                                           seq_ids, seq_len, seq_cap, verify_ws, st);
}

extern "C" int pie_decoder_step_batch(pie_decoder *d, const int32_t *tokens, const int32_t *context_lens, const void *const *slabs, size_t n_pages, size_t slab_bytes,
                                      const int32_t *block_tables, int max_blocks, int B, void *logits, float *logprobs, int32_t *next_tokens,
                                      int flags, void *stream) {
    const std::string who = "pie_decoder_step_batch: ";
    PIE_REQUIRE(d && tokens && context_lens && slabs && block_tables && logits && logprobs && next_tokens, PIE_E_ARG, who + "null pointer");
    const PoolRefusals shared = {d, who, slabs, n_pages, slab_bytes, max_blocks, B >= 1 && B <= 4096, "bad batch shape", SLABS_BELOW_ACTIVE_FORMAT};
    if (int rc = shared.check(POOL_GLOBALS, POOL_GLOBALS)) return rc;
    PIE_REQUIRE(!d->tp(), PIE_E_STATE, who + "not available on a tensor-parallel shard");
    if (int rc = shared.check(POOL_LAYERS, POOL_SHAPE)) return rc;
    if (int rc = d->rows.check_rows(B, "pie_decoder_step_batch")) return rc;
    PIE_REQUIRE(!d->rows.top.n || pie_aligned(logprobs, 4), PIE_E_ALIGN, who + "logprobs need 4-byte alignment");
    if (int rc = shared.check(POOL_SLAB_BYTES, POOL_SLABS)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const auto decode_batch = [&](hipStream_t on) {  // the step's launches on a stream: the caller's, or the capturing one
        return for_dtype(d->cfg.dtype, [&](auto t) {
            return decode_batch_t<decltype(t)>(d, tokens, context_lens, slabs, (int)n_pages, block_tables, max_blocks, B, (u16 *)logits, logprobs, next_tokens, on);
        });
    };
    if (!(flags & PIE_STEP_GRAPH)) return decode_batch(st);
    // Graph replay.  The launches bake in the caller's buffers and this library's scratch / resident weight copies, so a graph is
    // captured only for a call that repeats the previous call's buffers after that call allocated nothing, and is dropped when
    // either changes.  (First call with new buffers: eager, it may allocate; second: capture; from the third: replay.)
    std::vector<uintptr_t> key = {(uintptr_t)tokens, (uintptr_t)context_lens, (uintptr_t)block_tables, (uintptr_t)logits, (uintptr_t)logprobs,
                                  (uintptr_t)next_tokens, (uintptr_t)n_pages, (uintptr_t)max_blocks, (uintptr_t)B, (uintptr_t)d->kv_i8 /* the page format is baked into the launches too */};
    for (int i = 0; i < d->cfg.n_layers; ++i) key.push_back((uintptr_t)slabs[i]);
    d->rows.key(key);  // the tail's launches bake the per-row state in too
    if (!d->prefill) d->prefill = new PrefillScratch();
    PrefillScratch *s = d->prefill;
    if (s->batch_graph && s->batch_key == key && s->batch_gen == s->alloc_gen) {
        PIE_HIP_TRY(hipGraphLaunch(s->batch_graph, st));
        ++d->batch_replays;
        return PIE_OK;
    }
    if (s->warm_key == key && s->warm_gen == s->alloc_gen) {
        if (s->batch_graph) (void)hipGraphExecDestroy(s->batch_graph), s->batch_graph = nullptr;
        const unsigned gen = s->alloc_gen;
        hipGraph_t g = nullptr;
        hipError_t e = hipSuccess;
        int rc = PIE_OK;
        const int crc = capture_graph(decode_batch, &rc, &g, &e);
        if (crc) return crc;
        if (rc || e != hipSuccess || d->prefill->alloc_gen != gen) {  // something allocated or failed under capture: run this call eagerly instead
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            d->prefill->warm_key.clear();
            return decode_batch(st);
        }
        s = d->prefill;
        e = hipGraphInstantiate(&s->batch_graph, g, nullptr, nullptr, 0);
        d->batch_graph_kernels = graph_kernel_nodes(g);  // what the graph really holds (pie_decoder_batch_graph_launches), not a formula
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) return pie::fail(PIE_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        s->batch_key = key, s->batch_gen = s->alloc_gen;
        PIE_HIP_TRY(hipGraphLaunch(s->batch_graph, st));
        return PIE_OK;
    }
    const int rc = decode_batch(st);
    d->prefill->warm_key = key, d->prefill->warm_gen = d->prefill->alloc_gen;
    return rc;
}

int prefill_batched(pie_decoder *d, const int32_t *ids, const void *embeds, int L, void *logits_all, hipStream_t st) {
    const int rep = d->cfg.n_heads / d->cfg.n_kv_heads;
    PIE_REQUIRE(rep >= 1 && rep <= 8, PIE_E_SHAPE, "prefill: n_heads / n_kv_heads must be between 1 and 8");
    return for_dtype(d->cfg.dtype, [&](auto t) { return prefill_t<decltype(t)>(d, ids, embeds, L, logits_all, st); });
}
