// paged_attn_verify_i8.hip -- attention of a batched speculative pass over int8 pages, on the MFMA units.
//
// The same rows as paged_attn_verify.hip: segment s is sequence s's 1..8 consecutive query rows, row r attends positions 0 .. row_ctx[r] - 1
// of its own sequence's pages, which already hold this pass's own rows as codes (the RoPE + append launch quantises in front).  Pages and
// arithmetic are paged_i8.hip's: x' = fp32(q8) * fp32(s) with the page's per-head fp16 scale, fp32 afterwards, one rounding to T at the end.
// k_paged_attn_verify_i8, grid (kv-heads, splits, segments), 4 waves:
//   * columns: the segment's (row, q-head) pairs of the kv-group, c = row * REP + head, C = rows * REP <= 64, are the N side of every
//     product -- one or two 32-column tiles.  A lane keeps its column's Q fragments in VGPRs (the B operand of K . Q^T) for the whole
//     kernel; padding columns attend nothing (context 0) and are never stored;
//   * the positions of the segment's LONGEST row are cut by attn_split; a split walks its pages.  The 64 x D codes of (page, kv-head) --
//     contiguous, 16-byte loads, fetched into registers one page ahead of their use, half the registers of the T kernel -- are converted
//     to T ONCE on the way into LDS (integers up to 127 are exact in bf16 and f16) and stored as two 32-key images in prefill_attn.hpp's
//     dual-use swizzle; codes at or behind the longest context are stored as zeros.  Every column then uses them from there;
//   * per 32-key image, in prefill_attn.hpp's orientation: S^T[key, col] = K . Q^T (v_mfma_f32_32x32x16, A = K rows by ds_read_b128), the
//     score = acc * (scale * log2e * k_scale[page, g]) in fp32, masked per column by ITS row's context (a row never sees its successors'
//     codes); online softmax over registers; the value operand p * v_scale[page, g] in fp32, split into hi + lo halves of T, is directly
//     the B operand of O^T[dim, col] += V^T . P^T, whose A = V^T comes through the hardware-transposing read (ds_read_b64_tr_b16) of the
//     row-major V image -- conflict-free under that swizzle, where a transposed store would be 2-byte scatters;
//   * a page in LDS is two 32-key images, so wave w takes image w >> 1.  Two column tiles: wave w owns tile w & 1.  One tile: the pair of
//     waves of an image scores it alike and wave w accumulates the output dims' half w & 1 (both waves busy instead of one idle; the
//     scores are a third of the image's MFMAs);
//   * every wave keeps its own online-softmax stream; the streams of image 1 go to LDS (the tile's storage, behind a barrier) and the
//     waves of image 0 merge them behind their own: fixed order.  With one split the result itself, else one partial (m, l, acc[D]) per
//     (row, head, split) for k_verify_attn_merge (paged_attn_verify.hip).
#include "paged_attn_verify.hpp"
#include "prefill_attn.hpp"

namespace {

constexpr int VI_WAVES = 4, VI_NT = VI_WAVES * 64;

__device__ __forceinline__ int vi_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float vi_f16(u32 bits) { return (float)__builtin_bit_cast(_Float16, (u16)bits); }
// codes j and j + 1 of a word as a T pair: exact
template <class T>
__device__ __forceinline__ u32 vi_codes2(u32 w, int j) {
    return pack2<T>((float)(int)(signed char)(w >> (8 * j)), (float)(int)(signed char)(w >> (8 * j + 8)));
}

template <class T, int D, int REP>
__global__ void __launch_bounds__(VI_NT) k_paged_attn_verify_i8(const VerifyAttnArgs a, const size_t page_bytes) {
    constexpr int KS = D / 16, DT = D / 32;  // k-steps of K . Q^T, 32-dim output tiles
    constexpr int PPR = D / 16;              // 16-code pieces of a row
    constexpr int PCS = 64 * PPR / VI_NT;    // pieces of a page's K (and V) codes per thread
    constexpr int IMG = 32 * 2 * D;          // bytes of one 32-key image of T rows
    constexpr bool CAN_TWO = REP * VERIFY_MAX_SEG_ROWS > 32;
    static_assert(PCS >= 1 && DT >= 2, "head_dim 64 or 128");
    __shared__ __attribute__((aligned(16))) char s_kv[4 * IMG];  // K images 0, 1, then V images 0, 1
    __shared__ float s_ml[2][64][2];
    char *const k_lds = s_kv, *const v_lds = s_kv + 2 * IMG;
    float *const s_acc = reinterpret_cast<float *>(s_kv);  // [2 waves][DT * 16 registers][64 lanes] once the scoring is over: 256 D bytes, the images' size

    const int g = blockIdx.x, split = blockIdx.y, seg = blockIdx.z, q0 = g * REP;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    // every index that comes from device memory is clamped before it addresses anything
    const int r0 = vi_clamp(a.seg_first[seg], 0, a.N);
    const int n = vi_clamp(a.seg_first[seg + 1], r0, min(a.N, r0 + VERIFY_MAX_SEG_ROWS)) - r0;
    if (n <= 0) return;  // idle slot
    const int cap_pos = a.bt_stride * 64;
    int Tmax = 0;
    for (int i = 0; i < n; ++i) Tmax = max(Tmax, vi_clamp(a.row_ctx[r0 + i], 0, cap_pos));
    const AttnSplit sp = attn_split(Tmax, a.splits);
    if (split >= sp.active) {  // uniform for the workgroup: the neutral partial (one split and no position at all: zeros)
        for (int o = threadIdx.x; o < n * REP * (D / 2); o += VI_NT) {
            const int i = o / (REP * (D / 2)), hd = (o / (D / 2)) % REP, d = (o % (D / 2)) * 2;
            const size_t hq = (size_t)(r0 + i) * a.Hq + q0 + hd;
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
    const int *bt = a.block_table + (size_t)vi_clamp(a.row_seq[r0], 0, a.B - 1) * a.bt_stride;
    const char *slab = reinterpret_cast<const char *>(a.slab);
    const size_t blk = (size_t)a.Hkv * 64 * D;  // bytes of a page's K (and V) block
    const unsigned last_page = (unsigned)a.n_pages - 1u;

    // wave roles
    const int C = n * REP;
    const bool two = CAN_TWO && C > 32;
    const int kb = wave >> 1, sub = wave & 1;
    const int dt0 = two ? 0 : sub * (DT / 2), ndt = two ? DT : DT / 2;  // the output tiles this wave accumulates: oacc[j] = tile dt0 + j
    const int cc = (two ? 32 * sub : 0) + c;                            // this lane's column
    const bool col_on = cc < C;
    const int cq = col_on ? cc : C - 1, ci = cq / REP, chd = cq % REP;
    const int ctx_c = col_on ? vi_clamp(a.row_ctx[r0 + ci], 0, cap_pos) : 0;  // a padding column attends nothing
    const size_t hq = (size_t)(r0 + ci) * a.Hq + q0 + chd;
    uint4 qf[KS];  // B operand of K . Q^T: lane (column c, half h), k-step s holds Q[column][16 s + 8 h .. + 8]
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const uint4 *>(a.q + hq * D + 16 * s + 8 * h);

    f32x16_t oacc[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[j][i] = 0.0f;
    float m_run = ATTN_NEG, l_run = 0.0f;

    uint4 kreg[PCS], vreg[PCS];
    u32 sc_next = 0, sc_cur = 0;  // K scale | V scale << 16 of (page, kv-head): fp16 bits
    auto fetch = [&](int p) {     // page p's codes of this kv-head: 64 x D bytes of K, contiguous, and the same of V; and the two scales
        const unsigned pg = min((unsigned)bt[p], last_page);  // a corrupt table must not become a wild address
        const char *page = slab + (size_t)pg * page_bytes;
        const uint4 *kp = reinterpret_cast<const uint4 *>(page + (size_t)g * 64 * D);
        const uint4 *vp = reinterpret_cast<const uint4 *>(page + blk + (size_t)g * 64 * D);
#pragma unroll
        for (int j = 0; j < PCS; ++j) kreg[j] = kp[threadIdx.x + j * VI_NT], vreg[j] = vp[threadIdx.x + j * VI_NT];
        const u16 *scp = reinterpret_cast<const u16 *>(page + 2 * blk);
        sc_next = (u32)scp[g] | ((u32)scp[a.Hkv + g] << 16);
    };
    auto publish = [&](char *img, const uint4 &q8, int row, int pc, bool live) {  // 16 codes -> two 16-byte chunks of T
        uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
        if (live) {
            lo = make_uint4(vi_codes2<T>(q8.x, 0), vi_codes2<T>(q8.x, 2), vi_codes2<T>(q8.y, 0), vi_codes2<T>(q8.y, 2));
            hi = make_uint4(vi_codes2<T>(q8.z, 0), vi_codes2<T>(q8.z, 2), vi_codes2<T>(q8.w, 0), vi_codes2<T>(q8.w, 2));
        }
        char *base = img + (row >> 5) * IMG;
        *reinterpret_cast<uint4 *>(base + pa_off<D>(row & 31, 2 * pc)) = lo;
        *reinterpret_cast<uint4 *>(base + pa_off<D>(row & 31, 2 * pc + 1)) = hi;
    };
    const float sl2 = a.scale * ATTN_LOG2E;
    // transposed-read addressing (prefill_attn.hpp): lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p + 3
    const int grp = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;

    fetch(p_first);
    for (int p = p_first; p <= p_last; ++p) {
        __syncthreads();  // the page before is scored
#pragma unroll
        for (int j = 0; j < PCS; ++j) {
            const int x = threadIdx.x + j * VI_NT, row = x / PPR, pc = x % PPR;
            const bool live = p * 64 + row < Tmax;  // behind the longest context: zero codes, whatever the page holds
            publish(k_lds, kreg[j], row, pc, live);
            publish(v_lds, vreg[j], row, pc, live);
        }
        sc_cur = sc_next;
        __syncthreads();
        if (p < p_last) fetch(p + 1);  // in flight under the scoring
        const int tb = p * 64 + kb * 32;
        if (tb >= t_end || tb + 32 <= t_begin) continue;  // wave-uniform: an image outside the split
        const char *kimg = k_lds + kb * IMG, *vimg = v_lds + kb * IMG;
        const float ksl = sl2 * vi_f16(sc_cur & 0xFFFFu), vs = vi_f16(sc_cur >> 16);

        // S^T = K . Q^T : rows = keys (registers), cols = the segment's (row, head) pairs (lanes)
        f32x16_t sacc;
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint4 kf = *reinterpret_cast<const uint4 *>(kimg + pa_off<D>(c, 2 * s + h));
            sacc = MfmaT<T>::run(kf, qf[s], sacc);
        }
        // online softmax over keys: register i <-> key tb + (i & 3) + 8 (i >> 2) + 4 h
        const int t_hi = min(ctx_c, t_end);  // the column's own context, inside the split
        float sc[16], mloc = ATTN_NEG;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int t = tb + (i & 3) + 8 * (i >> 2) + 4 * h;
            sc[i] = (t >= t_begin && t < t_hi) ? sacc[i] * ksl : ATTN_NEG;
            mloc = fmaxf(mloc, sc[i]);
        }
        mloc = xor32_max(mloc);  // the other 16 keys of the image live in the partner lane
        const float m_new = fmaxf(m_run, mloc);
        if (m_new > m_run) {
            const float alpha = attn_exp2(m_run - m_new);
            l_run *= alpha;
#pragma unroll
            for (int j = 0; j < DT; ++j)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[j][i] *= alpha;
            m_run = m_new;
        }
        u32 phi[8], plo[8];
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
            const int ta = tb + (i & 3) + 8 * (i >> 2) + 4 * h;
            const float pa = (ta >= t_begin && ta < t_hi) ? attn_exp2(sc[i] - m_run) : 0.0f;
            const float pb = (ta + 1 >= t_begin && ta + 1 < t_hi) ? attn_exp2(sc[i + 1] - m_run) : 0.0f;
            l_run += pa + pb;
            const float va = pa * vs, vb = pb * vs;  // the value operand carries the page's V scale
            const float ha = round_T<T>(va), hb = round_T<T>(vb);
            phi[i >> 1] = pack2<T>(ha, hb);
            plo[i >> 1] = pack2<T>(va - ha, vb - hb);
        }
        // O^T += V^T . P^T : k-step s covers keys 16 s .. 16 s + 15 in the operand order 16 s + 8 (j >> 2) + 4 h + (j & 3)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint4 bh = make_uint4(phi[4 * s], phi[4 * s + 1], phi[4 * s + 2], phi[4 * s + 3]);
            const uint4 bl = make_uint4(plo[4 * s], plo[4 * s + 1], plo[4 * s + 2], plo[4 * s + 3]);
#pragma unroll
            for (int j = 0; j < DT; ++j) {
                if (j < ndt) {  // wave-uniform
                    const int ch = 4 * (dt0 + j) + 2 * (grp & 1) + (tp >> 1);
                    const v4i16_t lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) v4i16_t *)(vimg + pa_off<D>(16 * s + 4 * h + tq, ch) + 8 * (tp & 1)));
                    const v4i16_t hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) v4i16_t *)(vimg + pa_off<D>(16 * s + 8 + 4 * h + tq, ch) + 8 * (tp & 1)));
                    const uint2 a0 = __builtin_bit_cast(uint2, lo4), a1 = __builtin_bit_cast(uint2, hi4);
                    const uint4 vf = make_uint4(a0.x, a0.y, a1.x, a1.y);
                    oacc[j] = MfmaT<T>::run(vf, bh, oacc[j]);
                    oacc[j] = MfmaT<T>::run(vf, bl, oacc[j]);
                }
            }
        }
    }

    // the streams of image 1 go through LDS to the waves of image 0 (same sub: same columns and output tiles)
    __syncthreads();  // every wave is done with the images: their storage takes the streams
    if (kb == 1) {
#pragma unroll
        for (int j = 0; j < DT; ++j)
            if (j < ndt)
#pragma unroll
                for (int i = 0; i < 16; ++i) s_acc[((sub * DT + j) * 16 + i) * 64 + lane] = oacc[j][i];
        s_ml[sub][lane][0] = m_run, s_ml[sub][lane][1] = l_run;
    }
    __syncthreads();
    if (kb == 1) return;
    const float m1 = s_ml[sub][lane][0], l1 = s_ml[sub][lane][1];
    const float M = fmaxf(m_run, m1);  // (the lane pair of a column holds the same maxima)
    const float w0 = attn_exp2(m_run - M), w1 = attn_exp2(m1 - M);  // a stream that saw no position: weight 0, or 1 when neither did (l = 0 then)
    const float Lsum = xor32_sum(fmaf(w1, l1, w0 * l_run));          // the pair holds the two halves of the column's sum
#pragma unroll
    for (int j = 0; j < DT; ++j)
        if (j < ndt)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[j][i] = fmaf(w1, s_acc[((sub * DT + j) * 16 + i) * 64 + lane], w0 * oacc[j][i]);
    if (!col_on) return;  // padding columns are never stored
#pragma unroll
    for (int j = 0; j < DT; ++j) {
        if (j < ndt) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // registers 4k .. 4k + 3 <-> dims 32 (dt0 + j) + 8 k + 4 h + {0..3}
                const int d = 32 * (dt0 + j) + 8 * k + 4 * h;
                const float o0 = oacc[j][4 * k], o1 = oacc[j][4 * k + 1], o2 = oacc[j][4 * k + 2], o3 = oacc[j][4 * k + 3];
                if (a.splits == 1) {  // the partial IS the result: no merge launch (a row that attends nothing: zeros)
                    *reinterpret_cast<uint2 *>(a.out + hq * D + d) =
                        Lsum > 0.0f ? make_uint2(pack2<T>(o0 / Lsum, o1 / Lsum), pack2<T>(o2 / Lsum, o3 / Lsum)) : make_uint2(0u, 0u);
                } else {
                    *reinterpret_cast<float4 *>(a.part_acc + (hq * a.splits + split) * D + d) = make_float4(o0, o1, o2, o3);
                }
            }
        }
    }
    if (a.splits > 1 && h == 0 && (two || sub == 0)) a.part_ml[(hq * a.splits + split) * 2 + 0] = M, a.part_ml[(hq * a.splits + split) * 2 + 1] = Lsum;
}

template <class T, int D>
int verify_attn_i8_launch_rep(const VerifyAttnArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)a.Hkv, (unsigned)a.splits, (unsigned)a.B);
    const size_t pb = pie_page_i8_bytes(a.Hkv, D);
#define VI_GO(R)                                                                                       \
    hipLaunchKernelGGL((k_paged_attn_verify_i8<T, D, R>), grid, dim3(VI_NT), 0, st, a, pb);            \
    break
    switch (a.Hq / a.Hkv) {
        case 1: VI_GO(1);
        case 2: VI_GO(2);
        case 3: VI_GO(3);
        case 4: VI_GO(4);
        case 5: VI_GO(5);
        case 6: VI_GO(6);
        case 7: VI_GO(7);
        case 8: VI_GO(8);
        default: return pie::fail(PIE_E_SHAPE, "paged_attn_verify_i8: n_heads / n_kv_heads must be between 1 and 8");
    }
#undef VI_GO
    PIE_LAUNCH_CHECK();
    return a.splits > 1 ? verify_attn_merge_launch(std::is_same<T, BF16>::value ? PIE_BF16 : PIE_F16, D, a, st) : PIE_OK;
}

}  // namespace

// A workgroup per CU: a position is half the T pages' bytes and a 32-key image is two dozen MFMAs per wave, so a split has to hold
// twice the positions of the T kernel's to weigh as much against the workgroup's fixed part (the Q fragments, the closing merge)
int paged_attn_verify_i8_splits(int B, int Hkv, int max_blocks) {
    if (B < 1 || Hkv < 1 || max_blocks < 1) return 1;
    int splits = (256 + B * Hkv - 1) / (B * Hkv);
    splits = splits > ATTN_MAX_SPLITS ? ATTN_MAX_SPLITS : splits;
    splits = splits > max_blocks ? max_blocks : splits;
    return splits < 1 ? 1 : splits;
}

int paged_attn_verify_i8_launch(int dtype, int D, const VerifyAttnArgs &a, hipStream_t st) {
    if (dtype == PIE_BF16 && D == 128) return verify_attn_i8_launch_rep<BF16, 128>(a, st);
    if (dtype == PIE_BF16 && D == 64) return verify_attn_i8_launch_rep<BF16, 64>(a, st);
    if (dtype == PIE_F16 && D == 128) return verify_attn_i8_launch_rep<F16, 128>(a, st);
    if (dtype == PIE_F16 && D == 64) return verify_attn_i8_launch_rep<F16, 64>(a, st);
    return pie::fail(PIE_E_SHAPE, "paged_attn_verify_i8: head_dim must be 64 or 128 and dtype bf16 / f16");
}

extern "C" {

int pie_paged_attn_verify_i8_splits(int B, int Hkv, int max_blocks) { return paged_attn_verify_i8_splits(B, Hkv, max_blocks); }

size_t pie_paged_attn_verify_i8_workspace_bytes(int N, int Hq, int D, int splits) {
    if (N <= 0 || Hq <= 0 || D <= 0 || splits < 1 || splits > ATTN_MAX_SPLITS) return 0;
    return (size_t)N * Hq * splits * (D + 2) * sizeof(float);
}

int pie_paged_attn_verify_i8(const void *q, const void *slab, size_t n_pages, size_t slab_bytes, const int32_t *block_tables, int max_blocks,
                             const int32_t *row_seq, const int32_t *row_context_lens, const int32_t *seg_first, int N, int B, int Hq, int Hkv, int D,
                             float scale, int dtype, int splits, void *out, void *workspace, void *stream) {
    PIE_REQUIRE(q && slab && block_tables && row_seq && row_context_lens && seg_first && out && workspace, PIE_E_ARG, "pie_paged_attn_verify_i8: null pointer");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_paged_attn_verify_i8: dtype must be PIE_BF16 or PIE_F16");
    PIE_REQUIRE(splits >= 0 && splits <= ATTN_MAX_SPLITS, PIE_E_ARG, "pie_paged_attn_verify_i8: splits must be 0 (chosen here) or 1..32");
    PIE_REQUIRE(N >= 1 && N <= 65535 && B >= 1 && B <= 65535 && max_blocks > 0 && max_blocks <= (1 << 24) && n_pages > 0 && n_pages < 0x7FFFFFFFu, PIE_E_SHAPE,
                "pie_paged_attn_verify_i8: bad batch shape");
    PIE_REQUIRE(D == 64 || D == 128, PIE_E_SHAPE, "pie_paged_attn_verify_i8: head_dim must be 64 or 128");
    PIE_REQUIRE(Hkv > 0 && Hq > 0 && Hq % Hkv == 0 && Hq / Hkv <= 8, PIE_E_SHAPE, "pie_paged_attn_verify_i8: n_heads must be 1..8 times n_kv_heads");
    PIE_REQUIRE(slab_bytes / pie_page_i8_bytes(Hkv, D) >= n_pages, PIE_E_SHAPE, "pie_paged_attn_verify_i8: the slab is smaller than n_pages int8 pages");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(slab, 16) && pie_aligned(out, 16) && pie_aligned(workspace, 16), PIE_E_ALIGN,
                "pie_paged_attn_verify_i8: q, slab, out and workspace need 16-byte alignment");
    PIE_REQUIRE(pie_aligned(block_tables, 4) && pie_aligned(row_seq, 4) && pie_aligned(row_context_lens, 4) && pie_aligned(seg_first, 4), PIE_E_ALIGN,
                "pie_paged_attn_verify_i8: the index arrays need 4-byte alignment");
    VerifyAttnArgs a = {};
    a.q = (const u16 *)q, a.slab = (const u16 *)slab, a.block_table = block_tables, a.row_seq = row_seq, a.row_ctx = row_context_lens, a.seg_first = seg_first;
    a.N = N, a.B = B, a.Hq = Hq, a.Hkv = Hkv, a.bt_stride = max_blocks, a.n_pages = (int)n_pages, a.scale = scale;
    a.splits = splits ? splits : paged_attn_verify_i8_splits(B, Hkv, max_blocks);
    a.part_acc = (float *)workspace;
    a.part_ml = a.part_acc + (size_t)N * Hq * a.splits * D;
    a.out = (u16 *)out;
    return paged_attn_verify_i8_launch(dtype, D, a, (hipStream_t)stream);
}

}  // extern "C"
