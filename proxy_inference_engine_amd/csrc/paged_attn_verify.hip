// paged_attn_verify.hip -- attention of a batched speculative pass over T pages.
//
// Segment s of the pass is sequence s's 1..8 consecutive query rows (the fed token, then its drafts); row r attends positions
// 0 .. row_ctx[r] - 1 of its own sequence's pages, which already hold this pass's own rows (the RoPE + append launch runs in front).
// k_paged_attn_verify, grid (kv-heads, splits, segments), 4 waves:
//   * the positions of the segment's LONGEST row are cut by attn_split (attention.hpp): fixed grid, data-dependent activity; an idle
//     split leaves the neutral partial, an idle slot (an empty segment) leaves at once;
//   * a split walks its pages: the K and V rows of (page, kv-head) -- 64 x D, contiguous in the page -- go to LDS once, fetched into
//     registers one page ahead of their use, and every (row, q-head) pair of the kv-group is scored against them there: the cache is
//     read once per (kv-head, split) for all rows and all heads.  Positions at or beyond the longest context are stored as zeros,
//     so nothing behind a context is ever multiplied; a row's shorter context is a mask on the scores;
//   * a wave owns two rows x REP heads (at most 16 online-softmax streams in registers, attn_decode_body's inner loop with LDS as its
//     source: dot2 scores, DPP reduction inside a token's lanes, one running max per token group); a segment of 1-2 / 3-4 rows has
//     4 / 2 waves per row pair, which then take the page's token blocks in turn;
//   * the token groups of a wave are merged by shuffles, the waves of a row pair through LDS (the tile's storage, behind a barrier);
//     fp32 throughout, one rounding at the end: with one split the result itself, else one partial (m, l, acc[D]) per (row, head, split).
// k_verify_attn_merge, grid (q-heads, rows): the splits' partials in split order, neutral ones at weight 0.
#include "paged_attn_verify.hpp"

namespace {

constexpr int VA_WAVES = 4, VA_NT = VA_WAVES * 64, VA_RPW = 2;  // waves, threads, rows per wave

__device__ __forceinline__ int va_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <class T, int D, int REP>
__global__ void __launch_bounds__(VA_NT) k_paged_attn_verify(const VerifyAttnArgs a) {
    constexpr int LPT = D / 8;            // lanes per token row (16 B each)
    constexpr int TPW = 64 / LPT;         // token rows per wave-load
    constexpr int NBLK = 64 / TPW;        // token blocks per page
    constexpr int NP = VA_RPW * REP;      // (row, head) pairs per wave
    constexpr int PCS = 64 * LPT / VA_NT;  // 16-byte pieces of a page's K (and V) rows per thread
    constexpr int TILE = 64 * LPT;        // pieces of one kv-head's K (or V) rows of a page
    __shared__ uint4 s_tile[2 * TILE];    // K rows, then V rows: [slot][piece]
    __shared__ float s_m[VA_WAVES][NP], s_l[VA_WAVES][NP];
    float *s_acc = reinterpret_cast<float *>(s_tile);  // [VA_WAVES][NP][D] once the scoring is over: 4 * NP * D * 4 <= 256 * D bytes, the tile's size
    static_assert(sizeof(float) * VA_WAVES * NP * D <= sizeof(uint4) * 2 * TILE, "the waves' streams must fit the tile's storage");

    const int g = blockIdx.x, split = blockIdx.y, seg = blockIdx.z, q0 = g * REP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ts = lane / LPT, dc = lane % LPT;
    // every index that comes from device memory is clamped before it addresses anything
    const int r0 = va_clamp(a.seg_first[seg], 0, a.N);
    const int n = va_clamp(a.seg_first[seg + 1], r0, min(a.N, r0 + VERIFY_MAX_SEG_ROWS)) - r0;
    if (n <= 0) return;  // idle slot
    const int cap_pos = a.bt_stride * 64;
    int Tmax = 0;
    for (int i = 0; i < n; ++i) Tmax = max(Tmax, va_clamp(a.row_ctx[r0 + i], 0, cap_pos));
    const AttnSplit sp = attn_split(Tmax, a.splits);
    if (split >= sp.active) {  // uniform for the workgroup: the neutral partial (one split and no position at all: zeros)
        for (int o = threadIdx.x; o < n * REP * (D / 2); o += VA_NT) {
            const int i = o / (REP * (D / 2)), h = (o / (D / 2)) % REP, d = (o % (D / 2)) * 2;
            const size_t hq = (size_t)(r0 + i) * a.Hq + q0 + h;
            if (a.splits == 1) {
                *reinterpret_cast<u32 *>(a.out + hq * D + d) = 0u;
                continue;
            }
            *reinterpret_cast<float2 *>(a.part_acc + (hq * a.splits + split) * D + d) = make_float2(0.0f, 0.0f);
            if (d == 0) a.part_ml[(hq * a.splits + split) * 2 + 0] = ATTN_NEG, a.part_ml[(hq * a.splits + split) * 2 + 1] = 0.0f;
        }
        return;
    }
    const int t_begin = split * sp.chunk, t_end = min(Tmax, t_begin + sp.chunk);  // t_begin < t_end <= cap_pos
    const int p_first = t_begin >> 6, p_last = (t_end - 1) >> 6;                  // pages of the split: below bt_stride
    const int *bt = a.block_table + (size_t)va_clamp(a.row_seq[r0], 0, a.B - 1) * a.bt_stride;
    const size_t page_elems = (size_t)2 * 64 * a.Hkv * D;
    const unsigned last_page = (unsigned)a.n_pages - 1u;

    // wave roles: NG row pairs, TS waves per pair taking the token blocks in turn; 3 row pairs leave the fourth wave to the staging alone
    const int NG = (n + 1) >> 1, TS = VA_WAVES / NG, rg = wave % NG, slice = wave / NG;
    const bool scoring = slice < TS;
    int ctx[VA_RPW];
    u32 qr[NP][4];
#pragma unroll
    for (int r = 0; r < VA_RPW; ++r) {
        const int i = 2 * rg + r;
        ctx[r] = i < n ? va_clamp(a.row_ctx[r0 + i], 0, cap_pos) : 0;  // a row pair's missing second row attends nothing and is not written
        const u16 *qrow = a.q + ((size_t)(r0 + min(i, n - 1)) * a.Hq + q0) * D + dc * 8;
#pragma unroll
        for (int h = 0; h < REP; ++h) {
            const uint4 qv = *reinterpret_cast<const uint4 *>(qrow + (size_t)h * D);
            qr[r * REP + h][0] = qv.x, qr[r * REP + h][1] = qv.y, qr[r * REP + h][2] = qv.z, qr[r * REP + h][3] = qv.w;
        }
    }
    float m[NP], l[NP], acc[NP][8];
#pragma unroll
    for (int pr = 0; pr < NP; ++pr) {
        m[pr] = ATTN_NEG, l[pr] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[pr][j] = 0.0f;
    }

    uint4 kreg[PCS], vreg[PCS];
    auto fetch = [&](int p) {  // page p's rows of this kv-head: 64 x D of K, contiguous, and the same of V
        const unsigned pg = min((unsigned)bt[p], last_page);  // a corrupt table must not become a wild address
        const uint4 *kp = reinterpret_cast<const uint4 *>(a.slab + (size_t)pg * page_elems + (size_t)g * 64 * D);
        const uint4 *vp = kp + (size_t)a.Hkv * TILE;
#pragma unroll
        for (int j = 0; j < PCS; ++j) kreg[j] = kp[threadIdx.x + j * VA_NT], vreg[j] = vp[threadIdx.x + j * VA_NT];
    };
    const float sl2 = a.scale * ATTN_LOG2E;
    fetch(p_first);
    for (int p = p_first; p <= p_last; ++p) {
        __syncthreads();  // the page before is scored
#pragma unroll
        for (int j = 0; j < PCS; ++j) {
            const int idx = threadIdx.x + j * VA_NT;
            const bool live = p * 64 + idx / LPT < Tmax;  // behind the longest context: zeros, whatever the page holds
            s_tile[idx] = live ? kreg[j] : make_uint4(0u, 0u, 0u, 0u);
            s_tile[TILE + idx] = live ? vreg[j] : make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        if (p < p_last) fetch(p + 1);  // in flight under the scoring
        if (!scoring) continue;
        for (int b = slice; b < NBLK; b += TS) {
            const int tb = p * 64 + b * TPW;
            if (tb >= t_end || tb + TPW <= t_begin) continue;  // wave-uniform: a block outside the split
            const int t = tb + ts;
            const bool in = t >= t_begin && t < t_end;
            const uint4 kq = s_tile[(b * TPW + ts) * LPT + dc], vq = s_tile[TILE + (b * TPW + ts) * LPT + dc];
            const u32 kw[4] = {kq.x, kq.y, kq.z, kq.w};
            float vf[8];
            vf[0] = lo_f32<T>(vq.x), vf[1] = hi_f32<T>(vq.x), vf[2] = lo_f32<T>(vq.y), vf[3] = hi_f32<T>(vq.y);
            vf[4] = lo_f32<T>(vq.z), vf[5] = hi_f32<T>(vq.z), vf[6] = lo_f32<T>(vq.w), vf[7] = hi_f32<T>(vq.w);
            float sc[NP];
#pragma unroll
            for (int pr = 0; pr < NP; ++pr) {
                sc[pr] = 0.0f;
#pragma unroll
                for (int j = 0; j < 4; ++j) sc[pr] = T::dot2(qr[pr][j], kw[j], sc[pr]);
            }
            // the reduction inside a token's lanes, written pair-interleaved (attn_decode_body's)
#pragma unroll
            for (int pr = 0; pr < NP; ++pr) sc[pr] += __builtin_amdgcn_update_dpp(0.0f, sc[pr], 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
#pragma unroll
            for (int pr = 0; pr < NP; ++pr) sc[pr] += __builtin_amdgcn_update_dpp(0.0f, sc[pr], 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
#pragma unroll
            for (int pr = 0; pr < NP; ++pr) sc[pr] += __builtin_amdgcn_update_dpp(0.0f, sc[pr], 0x141, 0xF, 0xF, true);  // row_half_mirror
            if (LPT == 16) {
#pragma unroll
                for (int pr = 0; pr < NP; ++pr) sc[pr] += __builtin_amdgcn_update_dpp(0.0f, sc[pr], 0x140, 0xF, 0xF, true);  // row_mirror
            }
            bool valid[VA_RPW];
#pragma unroll
            for (int r = 0; r < VA_RPW; ++r) valid[r] = in && t < ctx[r];  // causal inside the segment: a row never sees its successors
            bool grow = false;
#pragma unroll
            for (int pr = 0; pr < NP; ++pr) {
                sc[pr] = valid[pr / REP] ? sc[pr] * sl2 : ATTN_NEG;
                grow |= sc[pr] > m[pr];
            }
            if (grow) {
#pragma unroll
                for (int pr = 0; pr < NP; ++pr) {
                    const float m_new = sc[pr] > m[pr] ? sc[pr] : m[pr];
                    const float alpha = attn_exp2(m[pr] - m_new);
                    l[pr] *= alpha;
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[pr][j] *= alpha;
                    m[pr] = m_new;
                }
            }
#pragma unroll
            for (int pr = 0; pr < NP; ++pr) {
                const float pw = valid[pr / REP] ? attn_exp2(sc[pr] - m[pr]) : 0.0f;
                l[pr] += pw;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[pr][j] = fmaf(pw, vf[j], acc[pr][j]);
            }
        }
    }

    // the token groups of the wave (lanes with equal dc): common max, rescale, plain sums
#pragma unroll
    for (int pr = 0; pr < NP; ++pr) {
        float mw = m[pr];
        if (LPT == 8) mw = fmaxf(mw, ror8(mw));
        mw = xor32_max(xor16_max(mw));
        const float wg = attn_exp2(m[pr] - mw);  // 0 for a group that saw no valid position; 1 when none did (l = 0 then)
        m[pr] = mw;
        l[pr] *= wg;
        if (LPT == 8) l[pr] += ror8(l[pr]);
        l[pr] = xor32_sum(xor16_sum(l[pr]));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc[pr][j] *= wg;
            if (LPT == 8) acc[pr][j] += ror8(acc[pr][j]);
            acc[pr][j] = xor32_sum(xor16_sum(acc[pr][j]));
        }
    }
    __syncthreads();  // every wave is done with the tile: its storage takes the waves' streams
    if (scoring && ts == 0) {
#pragma unroll
        for (int pr = 0; pr < NP; ++pr) {
            if (dc == 0) s_m[wave][pr] = m[pr], s_l[wave][pr] = l[pr];
            float *dst = s_acc + ((size_t)wave * NP + pr) * D + dc * 8;
            *reinterpret_cast<float4 *>(dst) = make_float4(acc[pr][0], acc[pr][1], acc[pr][2], acc[pr][3]);
            *reinterpret_cast<float4 *>(dst + 4) = make_float4(acc[pr][4], acc[pr][5], acc[pr][6], acc[pr][7]);
        }
    }
    __syncthreads();
    // one (row, head, dim pair) per thread and iteration: the row pair's waves in wave order
    for (int o = threadIdx.x; o < n * REP * (D / 2); o += VA_NT) {
        const int i = o / (REP * (D / 2)), h = (o / (D / 2)) % REP, d = (o % (D / 2)) * 2;
        const int pr = (i & 1) * REP + h, w0 = i >> 1;
        float M = ATTN_NEG;
        for (int k = 0; k < TS; ++k) M = fmaxf(M, s_m[w0 + k * NG][pr]);
        float Lsum = 0.0f, A0 = 0.0f, A1 = 0.0f;
        for (int k = 0; k < TS; ++k) {
            const int w = w0 + k * NG;
            const float wt = attn_exp2(s_m[w][pr] - M);
            const float2 av = *reinterpret_cast<const float2 *>(s_acc + ((size_t)w * NP + pr) * D + d);
            Lsum = fmaf(wt, s_l[w][pr], Lsum);
            A0 = fmaf(wt, av.x, A0), A1 = fmaf(wt, av.y, A1);
        }
        const size_t hq = (size_t)(r0 + i) * a.Hq + q0 + h;
        if (a.splits == 1) {  // the partial IS the result: no merge launch (a row that attends nothing: zeros)
            *reinterpret_cast<u32 *>(a.out + hq * D + d) = Lsum > 0.0f ? pack2<T>(A0 / Lsum, A1 / Lsum) : 0u;
            continue;
        }
        *reinterpret_cast<float2 *>(a.part_acc + (hq * a.splits + split) * D + d) = make_float2(A0, A1);
        if (d == 0) a.part_ml[(hq * a.splits + split) * 2 + 0] = M, a.part_ml[(hq * a.splits + split) * 2 + 1] = Lsum;
    }
}

// out[row, head] from the splits' partials: every slot is read (an idle split's is neutral: weight exp2(ATTN_NEG - M) = 0), in split order
template <class T>
__global__ void __launch_bounds__(64) k_verify_attn_merge(const VerifyAttnArgs a, int D) {
    const int d = threadIdx.x * 2;
    if (d >= D) return;
    const size_t hq = (size_t)blockIdx.y * a.Hq + blockIdx.x;
    const float *ml = a.part_ml + hq * a.splits * 2, *pa = a.part_acc + hq * a.splits * D + d;
    float M = ATTN_NEG;
    for (int j = 0; j < a.splits; ++j) M = fmaxf(M, ml[2 * j]);
    float Lsum = 0.0f, A0 = 0.0f, A1 = 0.0f;
    for (int j = 0; j < a.splits; ++j) {
        const float w = attn_exp2(ml[2 * j] - M);
        const float2 av = *reinterpret_cast<const float2 *>(pa + (size_t)j * D);
        Lsum = fmaf(w, ml[2 * j + 1], Lsum);
        A0 = fmaf(w, av.x, A0), A1 = fmaf(w, av.y, A1);
    }
    *reinterpret_cast<u32 *>(a.out + hq * D + d) = Lsum > 0.0f ? pack2<T>(A0 / Lsum, A1 / Lsum) : 0u;
}

template <class T, int D>
int verify_attn_launch_rep(const VerifyAttnArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)a.Hkv, (unsigned)a.splits, (unsigned)a.B);
#define VA_GO(R)                                                                                   \
    hipLaunchKernelGGL((k_paged_attn_verify<T, D, R>), grid, dim3(VA_NT), 0, st, a);               \
    break
    switch (a.Hq / a.Hkv) {
        case 1: VA_GO(1);
        case 2: VA_GO(2);
        case 3: VA_GO(3);
        case 4: VA_GO(4);
        case 5: VA_GO(5);
        case 6: VA_GO(6);
        case 7: VA_GO(7);
        case 8: VA_GO(8);
        default: return pie::fail(PIE_E_SHAPE, "paged_attn_verify: n_heads / n_kv_heads must be between 1 and 8");
    }
#undef VA_GO
    PIE_LAUNCH_CHECK();
    if (a.splits > 1) {
        hipLaunchKernelGGL(k_verify_attn_merge<T>, dim3((unsigned)a.Hq, (unsigned)a.N), dim3(64), 0, st, a, D);
        PIE_LAUNCH_CHECK();
    }
    return PIE_OK;
}

}  // namespace

int paged_attn_verify_splits(int B, int Hkv, int max_blocks) {
    if (B < 1 || Hkv < 1 || max_blocks < 1) return 1;
    int splits = (512 + B * Hkv - 1) / (B * Hkv);
    splits = splits > ATTN_MAX_SPLITS ? ATTN_MAX_SPLITS : splits;
    splits = splits > max_blocks ? max_blocks : splits;
    return splits < 1 ? 1 : splits;
}

int paged_attn_verify_launch(int dtype, int D, const VerifyAttnArgs &a, hipStream_t st) {
    if (dtype == PIE_BF16 && D == 128) return verify_attn_launch_rep<BF16, 128>(a, st);
    if (dtype == PIE_BF16 && D == 64) return verify_attn_launch_rep<BF16, 64>(a, st);
    if (dtype == PIE_F16 && D == 128) return verify_attn_launch_rep<F16, 128>(a, st);
    if (dtype == PIE_F16 && D == 64) return verify_attn_launch_rep<F16, 64>(a, st);
    return pie::fail(PIE_E_SHAPE, "paged_attn_verify: head_dim must be 64 or 128 and dtype bf16 / f16");
}

extern "C" {

int pie_paged_attn_verify_splits(int B, int Hkv, int max_blocks) { return paged_attn_verify_splits(B, Hkv, max_blocks); }

size_t pie_paged_attn_verify_workspace_bytes(int N, int Hq, int D, int splits) {
    if (N <= 0 || Hq <= 0 || D <= 0 || splits < 1 || splits > ATTN_MAX_SPLITS) return 0;
    return (size_t)N * Hq * splits * (D + 2) * sizeof(float);
}

int pie_paged_attn_verify(const void *q, const void *slab, size_t n_pages, const int32_t *block_tables, int max_blocks, const int32_t *row_seq,
                          const int32_t *row_context_lens, const int32_t *seg_first, int N, int B, int Hq, int Hkv, int D, float scale, int dtype,
                          int splits, void *out, void *workspace, void *stream) {
    PIE_REQUIRE(q && slab && block_tables && row_seq && row_context_lens && seg_first && out && workspace, PIE_E_ARG, "pie_paged_attn_verify: null pointer");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_paged_attn_verify: dtype must be PIE_BF16 or PIE_F16");
    PIE_REQUIRE(splits >= 0 && splits <= ATTN_MAX_SPLITS, PIE_E_ARG, "pie_paged_attn_verify: splits must be 0 (chosen here) or 1..32");
    PIE_REQUIRE(N >= 1 && N <= 65535 && B >= 1 && B <= 65535 && max_blocks > 0 && max_blocks <= (1 << 24) && n_pages > 0 && n_pages < 0x7FFFFFFFu, PIE_E_SHAPE,
                "pie_paged_attn_verify: bad batch shape");
    PIE_REQUIRE(D == 64 || D == 128, PIE_E_SHAPE, "pie_paged_attn_verify: head_dim must be 64 or 128");
    PIE_REQUIRE(Hkv > 0 && Hq > 0 && Hq % Hkv == 0 && Hq / Hkv <= 8, PIE_E_SHAPE, "pie_paged_attn_verify: n_heads must be 1..8 times n_kv_heads");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(slab, 16) && pie_aligned(out, 16) && pie_aligned(workspace, 16), PIE_E_ALIGN,
                "pie_paged_attn_verify: q, slab, out and workspace need 16-byte alignment");
    PIE_REQUIRE(pie_aligned(block_tables, 4) && pie_aligned(row_seq, 4) && pie_aligned(row_context_lens, 4) && pie_aligned(seg_first, 4), PIE_E_ALIGN,
                "pie_paged_attn_verify: the index arrays need 4-byte alignment");
    VerifyAttnArgs a = {};
    a.q = (const u16 *)q, a.slab = (const u16 *)slab, a.block_table = block_tables, a.row_seq = row_seq, a.row_ctx = row_context_lens, a.seg_first = seg_first;
    a.N = N, a.B = B, a.Hq = Hq, a.Hkv = Hkv, a.bt_stride = max_blocks, a.n_pages = (int)n_pages, a.scale = scale;
    a.splits = splits ? splits : paged_attn_verify_splits(B, Hkv, max_blocks);
    a.part_acc = (float *)workspace;
    a.part_ml = a.part_acc + (size_t)N * Hq * a.splits * D;
    a.out = (u16 *)out;
    return paged_attn_verify_launch(dtype, D, a, (hipStream_t)stream);
}

}  // extern "C"
