// ops.hip -- op-level entry points that are not the W4S GEMV: attention (decode), RMSNorm, RoPE,
// SiLU*mul, residual add, and the log-softmax / argmax tail.  One C-ABI function per MLX op the reference
// calls on the decode path (see include/pie_hip.h for the call sites).
#include <cmath>

#include "attention.hpp"
#include "tail.hpp"
#include "token_dfa.hpp"

// ---------------------------------------------------------------- attention launch
template <class T, int D, bool PAGED, bool NT, bool SHORT = false, bool RING = false>
static int attn_launch_rep(int rep, const AttnArgs &a, bool combine, hipStream_t st) {
    const int rows = a.rows > 0 ? a.rows : 1;
    const dim3 grid(a.Hkv, a.splits + a.pf_rows, rows);
#define ATTN_GO(R)                                                                                                                      \
    {                                                                                                                                   \
        constexpr int W_ = SHORT ? attn_short_waves(R) : ATTN_WAVES;                                                                    \
        hipLaunchKernelGGL((k_attn_decode<T, D, R, PAGED, NT, W_, RING>), grid, dim3(W_ * 64), 0, st, a);                                      \
    }                                                                                                                                   \
    break
    switch (rep) {  // q-heads per kv-head: Llama-3-8B/70B 4/8, Llama-3.2-3B 3, Qwen2.5-7B 7, MHA 1
        case 1: ATTN_GO(1);
        case 2: ATTN_GO(2);
        case 3: ATTN_GO(3);
        case 4: ATTN_GO(4);
        case 5: ATTN_GO(5);
        case 6: ATTN_GO(6);
        case 7: ATTN_GO(7);
        case 8: ATTN_GO(8);
        default: return pie::fail(PIE_E_SHAPE, "sdpa_decode: n_heads / n_kv_heads must be between 1 and 8");
    }
#undef ATTN_GO
    PIE_LAUNCH_CHECK();
    if (combine && !(PAGED && a.splits == 1 && a.ctx_len)) {  // (one split per sequence of a paged batch: the kernel wrote `out` itself)
        hipLaunchKernelGGL(k_attn_combine<T>, dim3(a.Hq, rows), dim3(256), 0, st, a, D);
        PIE_LAUNCH_CHECK();
    }
    return PIE_OK;
}

template <class T, int D>
static int attn_launch_d(int rep, const AttnArgs &a, bool combine, hipStream_t st) {
    if (a.ring_stage) {  // RotatingKVCache (decoder step, contiguous buffers): the same three plans, rows found by the ring rule
        if (a.block_table) return pie::fail(PIE_E_STATE, "sdpa_decode: a rotating cache is contiguous");
        if (a.nt_kv) return attn_launch_rep<T, D, false, true, false, true>(rep, a, combine, st);
        if (!combine) return attn_launch_rep<T, D, false, false, true, true>(rep, a, combine, st);
        return attn_launch_rep<T, D, false, false, false, true>(rep, a, combine, st);
    }
    if (a.nt_kv) return a.block_table ? attn_launch_rep<T, D, true, true>(rep, a, combine, st) : attn_launch_rep<T, D, false, true>(rep, a, combine, st);
    if (!combine)  // the merged-split plan of short caches (capacity <= 1024): 4-wave workgroups
        return a.block_table ? attn_launch_rep<T, D, true, false, true>(rep, a, combine, st)
                             : attn_launch_rep<T, D, false, false, true>(rep, a, combine, st);
    return a.block_table ? attn_launch_rep<T, D, true, false>(rep, a, combine, st) : attn_launch_rep<T, D, false, false>(rep, a, combine, st);
}

int attn_decode_launch(int dtype, int D, AttnArgs &a, bool combine, hipStream_t stream) {
    PIE_REQUIRE(a.Hkv > 0 && a.Hq % a.Hkv == 0, PIE_E_SHAPE, "sdpa_decode: Hq must be a multiple of Hkv");
    PIE_REQUIRE(a.splits >= 1 && a.splits <= ATTN_MAX_SPLITS, PIE_E_ARG, "sdpa_decode: bad split count");
    const int rep = a.Hq / a.Hkv;
    if (dtype == PIE_BF16 && D == 128) return attn_launch_d<BF16, 128>(rep, a, combine, stream);
    if (dtype == PIE_BF16 && D == 64) return attn_launch_d<BF16, 64>(rep, a, combine, stream);
    if (dtype == PIE_F16 && D == 128) return attn_launch_d<F16, 128>(rep, a, combine, stream);
    if (dtype == PIE_F16 && D == 64) return attn_launch_d<F16, 64>(rep, a, combine, stream);
    return pie::fail(PIE_E_SHAPE, "sdpa_decode: head_dim must be 64 or 128 and dtype bf16/f16");
}

// ---------------------------------------------------------------- mx.fast.rms_norm: one workgroup per row
template <class T>
__global__ void __launch_bounds__(256) k_rms_norm(const u16 *x, const u16 *w, float eps, int H, u16 *y) {
    __shared__ float red[4];
    const u16 *xr = x + (size_t)blockIdx.x * H;
    u16 *yr = y + (size_t)blockIdx.x * H;
    float ssq = 0.0f;
    for (int i = threadIdx.x * 8; i < H; i += 256 * 8) {
        uint4 v = *reinterpret_cast<const uint4 *>(xr + i);
        const u32 vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float lo = lo_f32<T>(vv[j]), hi = hi_f32<T>(vv[j]);
            ssq = fmaf(lo, lo, ssq);
            ssq = fmaf(hi, hi, ssq);
        }
    }
    ssq = wave_sum(ssq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ssq;
    __syncthreads();
    const float inv = 1.0f / sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)H + eps);
    for (int i = threadIdx.x * 8; i < H; i += 256 * 8) {
        uint4 v = *reinterpret_cast<const uint4 *>(xr + i);
        uint4 g = *reinterpret_cast<const uint4 *>(w + i);
        const u32 vv[4] = {v.x, v.y, v.z, v.w}, gg[4] = {g.x, g.y, g.z, g.w};
        u32 o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = pack2<T>(round_T<T>(lo_f32<T>(vv[j]) * inv) * lo_f32<T>(gg[j]), round_T<T>(hi_f32<T>(vv[j]) * inv) * hi_f32<T>(gg[j]));
        *reinterpret_cast<uint4 *>(yr + i) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// ---------------------------------------------------------------- mx.fast.rope (rotate-half), one thread per pair
template <class T>
__global__ void k_rope(const u16 *x, int heads, int L, int D, const float *freqs, int offset, int traditional, u16 *y) {
    const int half = D >> 1;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)heads * L * half) return;
    const int i = (int)(idx % half);
    const size_t row = idx / half;  // h*L + l
    const int l = (int)(row % L);
    const float theta = (float)(offset + l) * (1.0f / freqs[i]);
    float sn, cs;
    sincosf(theta, &sn, &cs);
    const int i0 = traditional ? 2 * i : i, i1 = traditional ? 2 * i + 1 : i + half;
    const float a = T::to_f32(x[row * D + i0]), b = T::to_f32(x[row * D + i1]);
    y[row * D + i0] = T::from_f32(__fsub_rn(__fmul_rn(a, cs), __fmul_rn(b, sn)));
    y[row * D + i1] = T::from_f32(__fadd_rn(__fmul_rn(a, sn), __fmul_rn(b, cs)));
}

// ---------------------------------------------------------------- nn.silu(a) * b and a + b, 8 elements per thread
template <class T, int OP>
__global__ void k_binary(const u16 *a, const u16 *b, size_t n, u16 *y) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (i >= n) return;
    if (i + 8 <= n) {
        uint4 av = *reinterpret_cast<const uint4 *>(a + i), bv = *reinterpret_cast<const uint4 *>(b + i);
        const u32 aa[4] = {av.x, av.y, av.z, av.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
        u32 o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float al = lo_f32<T>(aa[j]), ah = hi_f32<T>(aa[j]), bl = lo_f32<T>(bb[j]), bh = hi_f32<T>(bb[j]);
            if (OP == 0) {
                al = round_T<T>(al / (1.0f + expf(-al))) * bl;
                ah = round_T<T>(ah / (1.0f + expf(-ah))) * bh;
            } else {
                al += bl, ah += bh;
            }
            o[j] = pack2<T>(al, ah);
        }
        *reinterpret_cast<uint4 *>(y + i) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        for (size_t k = i; k < n; ++k) {
            float av = T::to_f32(a[k]), bv = T::to_f32(b[k]);
            y[k] = T::from_f32(OP == 0 ? round_T<T>(av / (1.0f + expf(-av))) * bv : av + bv);
        }
    }
}

// ---------------------------------------------------------------- C ABI
template <class F16K, class BF16K>
static int by_dtype(int dtype, F16K f16k, BF16K bf16k, const char *who) {
    if (dtype == PIE_BF16) bf16k();
    else if (dtype == PIE_F16) f16k();
    else return pie::fail(PIE_E_ARG, std::string(who) + ": dtype must be PIE_BF16 or PIE_F16");
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

extern "C" {

size_t pie_sdpa_decode_workspace_bytes(int Hq, int D) {
    if (Hq <= 0 || D <= 0) return 0;
    return (size_t)Hq * ATTN_MAX_SPLITS * (D + 2) * sizeof(float);
}

int pie_sdpa_decode(const void *q, const void *k, const void *v, int Hq, int Hkv, int T, int cap, int D, float scale,
                    int dtype, void *out, void *workspace, void *stream) {
    PIE_REQUIRE(q && k && v && out && workspace, PIE_E_ARG, "pie_sdpa_decode: null pointer");
    PIE_REQUIRE(T >= 1 && T <= cap, PIE_E_SHAPE, "pie_sdpa_decode: need 1 <= T <= cap");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(k, 16) && pie_aligned(v, 16), PIE_E_ALIGN, "pie_sdpa_decode: 16-byte alignment required");
    AttnArgs a = {};
    a.q = (const u16 *)q, a.k = (const u16 *)k, a.v = (const u16 *)v;
    a.T = T, a.cap = cap, a.Hq = Hq, a.Hkv = Hkv, a.scale = scale;
    a.splits = T >= 2048 ? ATTN_MAX_SPLITS : (T >= 512 ? 16 : (T >= 128 ? 4 : 1));
    a.nt_kv = T >= 2048;
    a.part_acc = (float *)workspace;
    a.part_ml = a.part_acc + (size_t)Hq * ATTN_MAX_SPLITS * D;
    a.out = (u16 *)out;
    return attn_decode_launch(dtype, D, a, true, (hipStream_t)stream);
}

// The decoder's rotating-cache step attention (RING) at op level: the new K / V rows wait in `stage` ([2, Hkv, 64, D], row pos % 64) as the
// q|k|v epilogue leaves them; the launch moves them into ring row slot(pos) of k / v [Hkv, cap, D] and attends min(pos + 1, window) rows.
// The ring state (DecState) goes into the workspace behind the split partials.
int pie_sdpa_decode_ring(const void *q, void *k, void *v, const void *stage, int Hq, int Hkv, int cap, int D, int pos, int window, int keep,
                         int rot0, float scale, int dtype, void *out, void *workspace, void *stream) {
    PIE_REQUIRE(q && k && v && stage && out && workspace, PIE_E_ARG, "pie_sdpa_decode_ring: null pointer");
    PIE_REQUIRE(window >= 1 && keep >= 0 && keep < window && pos >= 0 && rot0 >= 0, PIE_E_ARG, "pie_sdpa_decode_ring: need 0 <= keep < window, pos >= 0");
    DecState s = {};
    s.pos = pos, s.cap = cap, s.window = window, s.keep = keep, s.rot0 = rot0;
    const int T = ring_len(s), slot = ring_slot(s, pos);
    PIE_REQUIRE(Hkv > 0 && cap >= 1 && T <= cap && slot < cap, PIE_E_SHAPE, "pie_sdpa_decode_ring: the ring's rows and the new row's slot must lie in the buffers");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(k, 16) && pie_aligned(v, 16) && pie_aligned(stage, 16) && pie_aligned(workspace, 16), PIE_E_ALIGN,
                "pie_sdpa_decode_ring: 16-byte alignment required");
    hipStream_t st = (hipStream_t)stream;
    DecState *ds = reinterpret_cast<DecState *>((char *)workspace + pie_sdpa_decode_workspace_bytes(Hq, D));
    PIE_HIP_TRY(hipMemcpyAsync(ds, &s, sizeof(s), hipMemcpyHostToDevice, st));  // (pageable source: staged before the call returns)
    AttnArgs a = {};
    a.q = (const u16 *)q, a.k = (const u16 *)k, a.v = (const u16 *)v, a.state = ds, a.ring_stage = (const u16 *)stage;
    a.Hq = Hq, a.Hkv = Hkv, a.scale = scale;
    a.splits = T >= 2048 ? ATTN_MAX_SPLITS : (T >= 512 ? 16 : (T >= 128 ? 4 : 1));
    a.nt_kv = T >= 2048;
    a.part_acc = (float *)workspace;
    a.part_ml = a.part_acc + (size_t)Hq * ATTN_MAX_SPLITS * D;
    a.out = (u16 *)out;
    return attn_decode_launch(dtype, D, a, true, st);
}

// ---------------------------------------------------------------- paged KV
// One thread per 16-byte piece of the new K and V rows: row (sequence s, kv-head g) goes to page
// block_table[s][positions[s] / 64], slot positions[s] % 64.  positions[s] < 0 = idle slot.
__global__ void __launch_bounds__(256) k_paged_kv_append(const uint4 *k, const uint4 *v, u16 *slab, const int *block_table, int bt_stride,
                                                          const int *positions, int B, int Hkv, int D, int n_pages) {
    const int ppr = D >> 3, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * Hkv * ppr) return;
    const int s = i / (Hkv * ppr), g = (i / ppr) % Hkv, pc = i % ppr;
    const int pos = positions[s];
    if (pos < 0 || (pos >> 6) >= bt_stride) return;
    const unsigned pg = min((unsigned)block_table[(size_t)s * bt_stride + (pos >> 6)], (unsigned)n_pages - 1u);
    u16 *kd = slab + (size_t)pg * 2 * 64 * Hkv * D + ((size_t)g * 64 + (pos & 63)) * D + pc * 8;
    *reinterpret_cast<uint4 *>(kd) = k[i];
    *reinterpret_cast<uint4 *>(kd + (size_t)Hkv * 64 * D) = v[i];
}

size_t pie_paged_attn_workspace_bytes(int B, int Hq, int D) {
    if (B <= 0 || Hq <= 0 || D <= 0) return 0;
    return (size_t)B * Hq * ATTN_MAX_SPLITS * (D + 2) * sizeof(float);
}

int pie_paged_kv_append(const void *k, const void *v, void *slab, size_t n_pages, const int32_t *block_table, int max_blocks,
                        const int32_t *positions, int B, int Hkv, int D, int dtype, void *stream) {
    PIE_REQUIRE(k && v && slab && block_table && positions, PIE_E_ARG, "pie_paged_kv_append: null pointer");
    PIE_REQUIRE(B > 0 && Hkv > 0 && max_blocks > 0 && n_pages > 0 && n_pages < 0x7FFFFFFFu, PIE_E_SHAPE, "pie_paged_kv_append: bad shape");
    PIE_REQUIRE(D == 64 || D == 128, PIE_E_SHAPE, "pie_paged_kv_append: head_dim must be 64 or 128");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_paged_kv_append: dtype must be PIE_BF16 or PIE_F16");
    PIE_REQUIRE(pie_aligned(k, 16) && pie_aligned(v, 16) && pie_aligned(slab, 16), PIE_E_ALIGN, "pie_paged_kv_append: 16-byte alignment required");
    const int n = B * Hkv * (D >> 3);
    hipLaunchKernelGGL(k_paged_kv_append, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const uint4 *)k, (const uint4 *)v, (u16 *)slab,
                       block_table, max_blocks, positions, B, Hkv, D, (int)n_pages);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

int pie_paged_attn_decode(const void *q, const void *slab, size_t n_pages, const int32_t *block_table, int max_blocks,
                          const int32_t *context_lens, int B, int Hq, int Hkv, int D, float scale, int dtype, void *out, void *workspace,
                          void *stream) {
    PIE_REQUIRE(q && slab && block_table && context_lens && out && workspace, PIE_E_ARG, "pie_paged_attn_decode: null pointer");
    PIE_REQUIRE(B > 0 && B <= 65535 && max_blocks > 0 && n_pages > 0 && n_pages < 0x7FFFFFFFu, PIE_E_SHAPE, "pie_paged_attn_decode: bad shape");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(slab, 16) && pie_aligned(out, 16), PIE_E_ALIGN, "pie_paged_attn_decode: 16-byte alignment required");
    AttnArgs a = {};
    a.q = (const u16 *)q, a.slab = (const u16 *)slab, a.block_table = block_table, a.ctx_len = context_lens;
    a.bt_stride = max_blocks, a.n_pages = (int)n_pages, a.rows = B;
    a.nt_kv = (size_t)B * max_blocks * 64 >= 2048;  // more rows than stay cached between steps
    a.Hq = Hq, a.Hkv = Hkv, a.scale = scale;
    // enough workgroups for two per CU across the batch, never more splits than pages per sequence
    int splits = Hkv > 0 ? (512 + B * Hkv - 1) / (B * Hkv) : 1;
    splits = splits > ATTN_MAX_SPLITS ? ATTN_MAX_SPLITS : splits;
    splits = splits > max_blocks ? max_blocks : splits;
    a.splits = splits < 1 ? 1 : splits;
    a.part_acc = (float *)workspace;
    a.part_ml = a.part_acc + (size_t)B * Hq * a.splits * D;
    a.out = (u16 *)out;
    return attn_decode_launch(dtype, D, a, true, (hipStream_t)stream);
}

int pie_rms_norm(const void *x, const void *w, float eps, int rows, int H, int dtype, void *y, void *stream) {
    PIE_REQUIRE(x && w && y, PIE_E_ARG, "pie_rms_norm: null pointer");
    PIE_REQUIRE(rows > 0 && H > 0 && H % 8 == 0, PIE_E_SHAPE, "pie_rms_norm: H must be a multiple of 8");
    PIE_REQUIRE(pie_aligned(x, 16) && pie_aligned(w, 16) && pie_aligned(y, 16), PIE_E_ALIGN, "pie_rms_norm: 16-byte alignment required");
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(
        dtype, [&] { hipLaunchKernelGGL(k_rms_norm<F16>, dim3(rows), dim3(256), 0, st, (const u16 *)x, (const u16 *)w, eps, H, (u16 *)y); },
        [&] { hipLaunchKernelGGL(k_rms_norm<BF16>, dim3(rows), dim3(256), 0, st, (const u16 *)x, (const u16 *)w, eps, H, (u16 *)y); },
        "pie_rms_norm");
}

int pie_rope(const void *x, int heads, int L, int D, const float *freqs, int offset, int dtype, void *y, void *stream) {
    return pie_rope_ex(x, heads, L, D, freqs, offset, 0, dtype, y, stream);
}

int pie_rope_ex(const void *x, int heads, int L, int D, const float *freqs, int offset, int traditional, int dtype, void *y,
                void *stream) {
    PIE_REQUIRE(x && freqs && y, PIE_E_ARG, "pie_rope: null pointer");
    PIE_REQUIRE(heads > 0 && L > 0 && D > 0 && D % 2 == 0 && offset >= 0, PIE_E_SHAPE, "pie_rope: bad shape");
    const size_t n = (size_t)heads * L * (D / 2);
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(
        dtype, [&] { hipLaunchKernelGGL(k_rope<F16>, grid, block, 0, st, (const u16 *)x, heads, L, D, freqs, offset, traditional, (u16 *)y); },
        [&] { hipLaunchKernelGGL(k_rope<BF16>, grid, block, 0, st, (const u16 *)x, heads, L, D, freqs, offset, traditional, (u16 *)y); }, "pie_rope");
}

static int binary(int op, const void *a, const void *b, size_t n, int dtype, void *y, void *stream, const char *who) {
    PIE_REQUIRE(a && b && y, PIE_E_ARG, std::string(who) + ": null pointer");
    PIE_REQUIRE(n > 0, PIE_E_SHAPE, std::string(who) + ": empty input");
    PIE_REQUIRE(pie_aligned(a, 16) && pie_aligned(b, 16) && pie_aligned(y, 16), PIE_E_ALIGN, std::string(who) + ": 16-byte alignment required");
    dim3 grid((unsigned)((n + 2047) / 2048)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (op == 0)
        return by_dtype(
            dtype, [&] { hipLaunchKernelGGL((k_binary<F16, 0>), grid, block, 0, st, (const u16 *)a, (const u16 *)b, n, (u16 *)y); },
            [&] { hipLaunchKernelGGL((k_binary<BF16, 0>), grid, block, 0, st, (const u16 *)a, (const u16 *)b, n, (u16 *)y); }, who);
    return by_dtype(
        dtype, [&] { hipLaunchKernelGGL((k_binary<F16, 1>), grid, block, 0, st, (const u16 *)a, (const u16 *)b, n, (u16 *)y); },
        [&] { hipLaunchKernelGGL((k_binary<BF16, 1>), grid, block, 0, st, (const u16 *)a, (const u16 *)b, n, (u16 *)y); }, who);
}

int pie_silu_mul(const void *a, const void *b, size_t n, int dtype, void *y, void *stream) {
    return binary(0, a, b, n, dtype, y, stream, "pie_silu_mul");
}
int pie_add(const void *a, const void *b, size_t n, int dtype, void *y, void *stream) {
    return binary(1, a, b, n, dtype, y, stream, "pie_add");
}

// The yardstick of bench.py's roofline.stream_peak: what this chip gives a BARE streaming read shaped like the weight GEMV's -- one 8-wave
// workgroup per CU, every wave instruction a contiguous KB of non-temporal 16-byte loads, four in flight per lane, nothing computed.
typedef __attribute__((ext_vector_type(4))) unsigned stream_u32x4;
__global__ void __launch_bounds__(512) k_stream_read(const stream_u32x4 *p, size_t n16, unsigned *sink) {
    const size_t stride = (size_t)gridDim.x * 512;
    size_t i = (size_t)blockIdx.x * 512 + threadIdx.x;
    unsigned acc = 0;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const stream_u32x4 a = __builtin_nontemporal_load(p + i), b = __builtin_nontemporal_load(p + i + stride), c = __builtin_nontemporal_load(p + i + 2 * stride),
                           d = __builtin_nontemporal_load(p + i + 3 * stride);
        acc ^= a.x ^ b.y ^ c.z ^ d.w;
    }
    for (; i < n16; i += stride) acc ^= __builtin_nontemporal_load(p + i).x;
    if (acc == 0x9e3779b9u && sink) *sink = acc;  // keeps the loads alive; practically never taken
}
int pie_stream_read(const void *p, size_t bytes, void *stream) {
    PIE_REQUIRE(p && bytes >= 16 && pie_aligned(p, 16), PIE_E_ARG, "pie_stream_read: need a 16-byte aligned buffer");
    int dev = 0, n_cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cus = prop.multiProcessorCount;
    hipLaunchKernelGGL(k_stream_read, dim3(n_cus), dim3(512), 0, (hipStream_t)stream, (const stream_u32x4 *)p, bytes / 16, (unsigned *)nullptr);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

int pie_logprobs_argmax(const void *logits, int V, int dtype, float *logprobs, int32_t *token, void *stream) {
    PIE_REQUIRE(logits && logprobs && token, PIE_E_ARG, "pie_logprobs_argmax: null pointer");
    PIE_REQUIRE(V > 0, PIE_E_SHAPE, "pie_logprobs_argmax: empty vocabulary");
    return logits_tail_launch(dtype, (const u16 *)logits, V, nullptr, 0, logprobs, token, nullptr, nullptr, 0, (hipStream_t)stream);
}

int pie_logits_penalty(void *logits, int V, int dtype, const int32_t *ids, int n, double penalty, void *stream) {
    PIE_REQUIRE(logits && ids, PIE_E_ARG, "pie_logits_penalty: null pointer");
    PIE_REQUIRE(penalty >= 0.0 && std::isfinite(penalty), PIE_E_ARG, "pie_logits_penalty: the penalty must be finite and non-negative");
    PIE_REQUIRE(n >= 1 && n <= PEN_MAX_IDS, PIE_E_ARG, "pie_logits_penalty: 1 <= n <= 1024 ids");
    PIE_REQUIRE(V >= 1, PIE_E_SHAPE, "pie_logits_penalty: empty vocabulary");
    PenArgs a = {};
    a.logits = (u16 *)logits, a.V = V, a.penalty = (float)penalty, a.ids = ids, a.n = n;
    return logits_penalty_launch(dtype, a, (hipStream_t)stream);
}

int pie_logprobs_argmax_masked(void *logits, int V, int dtype, const uint32_t *mask, int mask_words, float *logprobs, int32_t *token, void *stream) {
    PIE_REQUIRE(logits && mask && logprobs && token, PIE_E_ARG, "pie_logprobs_argmax_masked: null pointer");
    PIE_REQUIRE(V > 0, PIE_E_SHAPE, "pie_logprobs_argmax_masked: empty vocabulary");
    PIE_REQUIRE(mask_words >= (V + 31) / 32, PIE_E_SHAPE, "pie_logprobs_argmax_masked: the mask needs ceil(V / 32) words");
    PIE_REQUIRE(pie_aligned(mask, 4), PIE_E_ALIGN, "pie_logprobs_argmax_masked: the mask needs 4-byte alignment");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_logprobs_argmax_masked: dtype must be PIE_BF16 or PIE_F16");
    hipStream_t st = (hipStream_t)stream;
    LogitStat *stats = nullptr;  // stream-ordered scratch, like pie_logprobs_argmax's
    if (hipMallocAsync((void **)&stats, sizeof(LogitStat) * TAIL_STAT_TILES, st) != hipSuccess) return pie::fail(PIE_E_HIP, "pie_logprobs_argmax_masked: hipMallocAsync failed");
    int rc = logits_stats_launch(dtype, (u16 *)logits, V, stats, st, mask);
    if (!rc) rc = logits_tail_launch(dtype, (const u16 *)logits, V, stats, TAIL_STAT_TILES, logprobs, token, nullptr, nullptr, 0, st);
    (void)hipFreeAsync(stats, st);
    return rc;
}

int pie_logits_bias(void *logits, int V, int dtype, const int32_t *ids, const float *bias, int n, void *stream) {
    PIE_REQUIRE(logits && ids && bias, PIE_E_ARG, "pie_logits_bias: null pointer");
    PIE_REQUIRE(n >= 1 && n <= PEN_MAX_IDS, PIE_E_ARG, "pie_logits_bias: 1 <= n <= 1024 entries");
    PIE_REQUIRE(V >= 1, PIE_E_SHAPE, "pie_logits_bias: empty vocabulary");
    PIE_REQUIRE(pie_aligned(ids, 4) && pie_aligned(bias, 4), PIE_E_ALIGN, "pie_logits_bias: ids and bias need 4-byte alignment");
    PenArgs a = {};
    a.logits = (u16 *)logits, a.V = V, a.penalty = 1.0f;
    const BiasArgs b = {ids, bias, n, 0};  // the penalty phase off
    return logits_edit_launch(dtype, a, b, (hipStream_t)stream);
}

int pie_logits_penalty_rows(void *logits, int rows, int V, int dtype, const pie_row_tail *table, int32_t *recent_ids, const int32_t *ids,
                            const int32_t *ctx, const int32_t *out_rows, int n_src, void *stream) {
    PIE_REQUIRE(logits && table && recent_ids && ids && ctx, PIE_E_ARG, "pie_logits_penalty_rows: null pointer");
    PIE_REQUIRE(rows >= 1 && rows <= 65535 && n_src >= 1 && V >= 1, PIE_E_SHAPE, "pie_logits_penalty_rows: 1 <= rows <= 65535, n_src >= 1, V >= 1");
    PIE_REQUIRE(out_rows || n_src >= rows, PIE_E_SHAPE, "pie_logits_penalty_rows: without out_rows every output row needs its source row");
    PIE_REQUIRE(pie_aligned(table, 8) && pie_aligned(recent_ids, 4), PIE_E_ALIGN, "pie_logits_penalty_rows: misaligned table or ring");
    PenRowsArgs a = {};
    a.logits = (u16 *)logits, a.V = V, a.n_src = n_src, a.table = table, a.recent = recent_ids, a.ids = ids, a.ctx = ctx, a.out_rows = out_rows;
    return logits_penalty_rows_launch(dtype, a, rows, (hipStream_t)stream);
}

int pie_logprobs_argmax_rows_masked(void *logits, int rows, int V, int dtype, const uint32_t *masks, int mask_words, const int32_t *mask_on,
                                    float *logprobs, int32_t *tokens, void *stream) {
    PIE_REQUIRE(logits && masks && mask_on && logprobs && tokens, PIE_E_ARG, "pie_logprobs_argmax_rows_masked: null pointer");
    PIE_REQUIRE(rows >= 1, PIE_E_ARG, "pie_logprobs_argmax_rows_masked: rows >= 1");
    PIE_REQUIRE(rows <= 65535 && V > 0, PIE_E_SHAPE, "pie_logprobs_argmax_rows_masked: rows <= 65535 and a non-empty vocabulary");
    PIE_REQUIRE(mask_words >= (V + 31) / 32, PIE_E_SHAPE, "pie_logprobs_argmax_rows_masked: every row's mask needs ceil(V / 32) words");
    PIE_REQUIRE(pie_aligned(masks, 4) && pie_aligned(mask_on, 4), PIE_E_ALIGN, "pie_logprobs_argmax_rows_masked: masks and mask_on need 4-byte alignment");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_logprobs_argmax_rows_masked: dtype must be PIE_BF16 or PIE_F16");
    hipStream_t st = (hipStream_t)stream;
    LogitStat *stats = nullptr;  // stream-ordered scratch, like pie_logprobs_argmax's
    if (hipMallocAsync((void **)&stats, sizeof(LogitStat) * TAIL_STAT_TILES * (size_t)rows, st) != hipSuccess)
        return pie::fail(PIE_E_HIP, "pie_logprobs_argmax_rows_masked: hipMallocAsync failed");
    const int rc = logits_tail_rows_launch(dtype, (u16 *)logits, V, rows, stats, logprobs, tokens, st, masks, mask_words, mask_on);
    (void)hipFreeAsync(stats, st);
    return rc;
}

int pie_logits_bias_rows(void *logits, int rows, int V, int dtype, const int32_t *ids, const float *bias, const int32_t *n, int cap, void *stream) {
    PIE_REQUIRE(logits && ids && bias && n, PIE_E_ARG, "pie_logits_bias_rows: null pointer");
    PIE_REQUIRE(rows >= 1 && cap >= 1 && cap <= PEN_MAX_IDS, PIE_E_ARG, "pie_logits_bias_rows: rows >= 1 and 1 <= cap <= 1024 entries per row");
    PIE_REQUIRE(V >= 1, PIE_E_SHAPE, "pie_logits_bias_rows: empty vocabulary");
    PIE_REQUIRE(pie_aligned(ids, 4) && pie_aligned(bias, 4) && pie_aligned(n, 4), PIE_E_ALIGN, "pie_logits_bias_rows: ids, bias and n need 4-byte alignment");
    PenRowsArgs a = {};
    a.logits = (u16 *)logits, a.V = V;  // no ctx: every row is live, and the penalty phase is off
    const BiasRowsArgs b = {ids, bias, n, cap, 0};
    return logits_edit_rows_launch(dtype, a, b, rows, (hipStream_t)stream);
}

int pie_token_dfa_mask(const pie_row_dfa *records, const int32_t *states, const int32_t *tables, int tables_len, int rows, int V, uint32_t *masks,
                       int mask_words, int32_t *mask_on, void *stream) {
    PIE_REQUIRE(masks, PIE_E_ARG, "pie_token_dfa_mask: null pointer");
    if (int rc = token_dfa_check("pie_token_dfa_mask", records, states, tables, tables_len, rows, V)) return rc;
    PIE_REQUIRE(mask_words >= (V + 31) / 32, PIE_E_SHAPE, "pie_token_dfa_mask: every row's mask needs ceil(V / 32) words");
    PIE_REQUIRE(pie_aligned(masks, 4) && pie_aligned(mask_on, 4), PIE_E_ALIGN, "pie_token_dfa_mask: masks and mask_on need 4-byte alignment");
    return token_dfa_mask_launch(records, states, tables, tables_len, rows, V, masks, mask_words, mask_on, (hipStream_t)stream);
}

int pie_token_dfa_advance(const pie_row_dfa *records, int32_t *states, const int32_t *tables, int tables_len, int rows, int V, const int32_t *tokens,
                          void *stream) {
    PIE_REQUIRE(tokens, PIE_E_ARG, "pie_token_dfa_advance: null pointer");
    if (int rc = token_dfa_check("pie_token_dfa_advance", records, states, tables, tables_len, rows, V)) return rc;
    PIE_REQUIRE(pie_aligned(tokens, 4), PIE_E_ALIGN, "pie_token_dfa_advance: tokens need 4-byte alignment");
    return token_dfa_advance_launch(records, states, tables, tables_len, rows, V, tokens, (hipStream_t)stream);
}

int pie_token_dfa_walk(const pie_row_dfa *record, const int32_t *state, const int32_t *tables, int tables_len, int V, const int32_t *tokens, int n,
                       int32_t *out_states, void *stream) {
    PIE_REQUIRE(tokens && out_states, PIE_E_ARG, "pie_token_dfa_walk: null pointer");
    if (int rc = token_dfa_check("pie_token_dfa_walk", record, state, tables, tables_len, 1, V)) return rc;
    PIE_REQUIRE(n >= 1 && n <= DFA_MAX_DRAFT, PIE_E_SHAPE, "pie_token_dfa_walk: n must be 1..31");
    PIE_REQUIRE(pie_aligned(tokens, 4) && pie_aligned(out_states, 4), PIE_E_ALIGN, "pie_token_dfa_walk: tokens and out_states need 4-byte alignment");
    return token_dfa_walk_launch(record, state, tables, tables_len, V, tokens, n, out_states, nullptr, nullptr, (hipStream_t)stream);
}

int pie_token_dfa_draft(const pie_row_dfa *record, const int32_t *state, const int32_t *tables, int tables_len, const int32_t *forced, int forced_states, int V,
                        const int32_t *cand, const int32_t *cand_count, int k, int32_t *out_ids, int32_t *out_count, void *stream) {
    PIE_REQUIRE(forced && cand && cand_count && out_ids && out_count, PIE_E_ARG, "pie_token_dfa_draft: null pointer");
    if (int rc = token_dfa_check("pie_token_dfa_draft", record, state, tables, tables_len, 1, V)) return rc;
    PIE_REQUIRE(k >= 1 && k <= DFA_MAX_DRAFT && forced_states >= 1, PIE_E_SHAPE, "pie_token_dfa_draft: k must be 1..31 and the forced table hold at least one state");
    PIE_REQUIRE(pie_aligned(forced, 8) && pie_aligned(cand, 4) && pie_aligned(cand_count, 4) && pie_aligned(out_ids, 4) && pie_aligned(out_count, 4), PIE_E_ALIGN,
                "pie_token_dfa_draft: the forced table needs 8-byte, the candidate and the outputs 4-byte alignment");
    return token_dfa_draft_launch(record, state, tables, tables_len, forced, forced_states, V, cand, cand_count, k, out_ids, out_count, (hipStream_t)stream);
}

size_t pie_count_penalty_bytes(void) { return sizeof(pie_count_penalty); }

int pie_count_penalty_pack(double freq, double pres, int start, int counted_pos, pie_count_penalty *out) {
    PIE_REQUIRE(out, PIE_E_ARG, "pie_count_penalty_pack: null pointer");
    PIE_REQUIRE(std::isfinite(freq) && std::isfinite(pres) && std::isfinite((float)freq) && std::isfinite((float)pres), PIE_E_ARG,
                "pie_count_penalty_pack: the frequency and presence penalties must be finite");
    PIE_REQUIRE(start >= 0 && counted_pos >= -1, PIE_E_ARG, "pie_count_penalty_pack: start >= 0 and counted_pos >= -1");
    pie_count_penalty r = {};
    r.freq = (float)freq, r.pres = (float)pres, r.start = start, r.counted_pos = counted_pos;
    *out = r;
    return PIE_OK;
}

int pie_logits_count_penalty_rows(void *logits, int rows, int V, int dtype, pie_count_penalty *records, int32_t *counts, const int32_t *ids,
                                  const int32_t *ctx, const int32_t *out_rows, int n_src, void *stream) {
    PIE_REQUIRE(logits && records && counts, PIE_E_ARG, "pie_logits_count_penalty_rows: null pointer");
    PIE_REQUIRE(rows >= 1, PIE_E_ARG, "pie_logits_count_penalty_rows: rows >= 1");
    PIE_REQUIRE(!ctx || ids, PIE_E_ARG, "pie_logits_count_penalty_rows: context lengths without input ids");
    PIE_REQUIRE(rows <= 65535 && V >= 1, PIE_E_SHAPE, "pie_logits_count_penalty_rows: rows <= 65535 and a non-empty vocabulary");
    PIE_REQUIRE(!ctx || (n_src >= 1 && (out_rows || n_src >= rows)), PIE_E_SHAPE,
                "pie_logits_count_penalty_rows: n_src >= 1, and without out_rows every output row needs its source row");
    PIE_REQUIRE(pie_aligned(records, 4) && pie_aligned(counts, 4) && pie_aligned(logits, 2), PIE_E_ALIGN,
                "pie_logits_count_penalty_rows: records and counts need 4-byte alignment, logits 2-byte");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_logits_count_penalty_rows: dtype must be PIE_BF16 or PIE_F16");
    CountPenArgs a = {};
    a.logits = (u16 *)logits, a.V = V, a.n_src = n_src, a.records = records, a.counts = counts;
    if (ctx) a.ids = ids, a.ctx = ctx, a.out_rows = out_rows;
    return logits_count_penalty_rows_launch(dtype, a, rows, (hipStream_t)stream);
}

size_t pie_dry_penalty_bytes(void) { return sizeof(pie_dry_penalty); }

int pie_dry_penalty_pack(double multiplier, double base, int allowed_length, int range, int n_breakers, pie_dry_penalty *out) {
    PIE_REQUIRE(out, PIE_E_ARG, "pie_dry_penalty_pack: null pointer");
    PIE_REQUIRE(std::isfinite(multiplier) && std::isfinite((float)multiplier) && multiplier >= 0.0, PIE_E_ARG,
                "pie_dry_penalty_pack: the multiplier must be finite and non-negative");
    PIE_REQUIRE(std::isfinite(base) && std::isfinite((float)base) && (float)base > 0.0f, PIE_E_ARG, "pie_dry_penalty_pack: the base must be finite and positive");
    PIE_REQUIRE(allowed_length >= 1 && allowed_length <= PIE_DRY_MAX_MATCH, PIE_E_ARG, "pie_dry_penalty_pack: 1 <= allowed_length <= 64");
    PIE_REQUIRE(range >= 1 && range <= PEN_MAX_IDS, PIE_E_ARG, "pie_dry_penalty_pack: 1 <= range <= 1024 window positions");
    PIE_REQUIRE(n_breakers >= 0 && n_breakers <= PIE_DRY_BREAKERS_MAX, PIE_E_ARG, "pie_dry_penalty_pack: 0 <= n_breakers <= 64");
    pie_dry_penalty r = {};
    r.multiplier = (float)multiplier, r.base = (float)base, r.allowed_length = allowed_length, r.range = range, r.n_breakers = n_breakers;
    *out = r;
    return PIE_OK;
}

int pie_logits_dry_penalty(void *logits, int V, int dtype, const int32_t *ids, int n, double multiplier, double base, int allowed_length,
                           const int32_t *breakers, int n_breakers, void *stream) {
    PIE_REQUIRE(logits && ids && (breakers || n_breakers == 0), PIE_E_ARG, "pie_logits_dry_penalty: null pointer");
    PIE_REQUIRE(n >= 1 && n <= PEN_MAX_IDS, PIE_E_ARG, "pie_logits_dry_penalty: 1 <= n <= 1024 ids");
    DryArgs a = {};
    if (pie_dry_penalty_pack(multiplier, base, allowed_length, n, n_breakers, &a.value)) return PIE_E_ARG;  // (the message names the rule)
    PIE_REQUIRE(V >= 1, PIE_E_SHAPE, "pie_logits_dry_penalty: empty vocabulary");
    PIE_REQUIRE(pie_aligned(ids, 4) && pie_aligned(breakers, 4) && pie_aligned(logits, 2), PIE_E_ALIGN,
                "pie_logits_dry_penalty: ids and breakers need 4-byte alignment, logits 2-byte");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_logits_dry_penalty: dtype must be PIE_BF16 or PIE_F16");
    a.w.logits = (u16 *)logits, a.w.V = V, a.w.ids = ids, a.w.n = n, a.breakers = breakers;
    return logits_dry_launch(dtype, a, (hipStream_t)stream);
}

int pie_logits_dry_penalty_rows(void *logits, int rows, int V, int dtype, const pie_dry_penalty *records, const int32_t *breakers,
                                int32_t *recent_ids, const int32_t *ids, const int32_t *ctx, const int32_t *out_rows, int n_src, void *stream) {
    PIE_REQUIRE(logits && records && breakers && recent_ids && ids && ctx, PIE_E_ARG, "pie_logits_dry_penalty_rows: null pointer");
    PIE_REQUIRE(rows >= 1, PIE_E_ARG, "pie_logits_dry_penalty_rows: rows >= 1");
    PIE_REQUIRE(rows <= 65535 && n_src >= 1 && V >= 1, PIE_E_SHAPE, "pie_logits_dry_penalty_rows: rows <= 65535, n_src >= 1, V >= 1");
    PIE_REQUIRE(out_rows || n_src >= rows, PIE_E_SHAPE, "pie_logits_dry_penalty_rows: without out_rows every output row needs its source row");
    PIE_REQUIRE(pie_aligned(records, 4) && pie_aligned(breakers, 4) && pie_aligned(recent_ids, 4) && pie_aligned(ids, 4) && pie_aligned(ctx, 4) &&
                    pie_aligned(out_rows, 4) && pie_aligned(logits, 2),
                PIE_E_ALIGN, "pie_logits_dry_penalty_rows: the records and the int32 arrays need 4-byte alignment, logits 2-byte");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_logits_dry_penalty_rows: dtype must be PIE_BF16 or PIE_F16");
    DryRowsArgs a = {};
    a.r.logits = (u16 *)logits, a.r.V = V, a.r.n_src = n_src, a.r.recent = recent_ids, a.r.ids = ids, a.r.ctx = ctx, a.r.out_rows = out_rows;
    a.records = records, a.breakers = breakers;
    return logits_dry_rows_launch(dtype, a, rows, (hipStream_t)stream);
}

}  // extern "C"
