// paged_attn_verify_mfma.hip -- attention of a batched speculative pass over T pages, on the MFMA units.
//
// The contract of paged_attn_verify.hip through the same VerifyAttnArgs: segment s is sequence s's 1..8 consecutive query rows, row r attends
// positions 0 .. row_ctx[r] - 1 of its own sequence's T pages, which already hold this pass's own rows.  The structure is
// paged_attn_verify_i8.hip's with the conversion and the scales taken out.  k_paged_attn_verify_mfma, grid (kv-heads, splits, segments), 4 waves:
//   * columns: the segment's (row, q-head) pairs of the kv-group, c = row * REP + head, C = rows * REP <= 64, are the N side of every
//     product -- one or two 32-column tiles.  A lane keeps its column's Q fragments in VGPRs (the B operand of K . Q^T) for the whole
//     kernel; padding columns attend nothing (context 0) and are never stored;
//   * the positions of the segment's LONGEST row are cut by attn_split; a split walks its pages.  The 64 x D elements of (page, kv-head) --
//     contiguous, 16-byte loads, fetched into registers one page ahead of their use -- go unconverted into LDS as two 32-key images per
//     operand in prefill_attn.hpp's dual-use swizzle; positions at or behind the longest context are stored as zeros, whatever the page
//     holds (0 * NaN is NaN on the matrix units).  Every column then uses them from there;
//   * per 32-key image, in prefill_attn.hpp's orientation: S^T[key, col] = K . Q^T (v_mfma_f32_32x32x16, A = K rows by ds_read_b128), the
//     score = acc * scale * log2e in fp32, masked per column by ITS row's context (a row never sees its successors); base-2 online
//     softmax over registers; p in fp32, split into hi + lo halves of T, is directly the B operand of O^T[dim, col] += V^T . P^T, whose
//     A = V^T comes through the hardware-transposing read (ds_read_b64_tr_b16) of the row-major V image: k_prefill_attn's operand;
//   * a page in LDS is two 32-key images, so wave w takes image w >> 1.  Two column tiles: wave w owns tile w & 1.  One tile: the pair of
//     waves of an image scores it alike and wave w accumulates the output dims' half w & 1;
//   * every wave keeps its own online-softmax stream; the streams of image 1 go to LDS (the images' storage, behind a barrier) and the
//     waves of image 0 merge them behind their own: fixed order.  With one split the result itself, else one partial (m, l, acc[D]) per
//     (row, head, split) for k_verify_attn_merge (paged_attn_verify.hip).
#include "paged_attn_verify.hpp"
#include "prefill_attn.hpp"

namespace {

constexpr int VM_WAVES = 4, VM_NT = VM_WAVES * 64;

__device__ __forceinline__ int vm_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <class T, int D, int REP>
__global__ void __launch_bounds__(VM_NT) k_paged_attn_verify_mfma(const VerifyAttnArgs a) {
    constexpr int KS = D / 16, DT = D / 32;  // k-steps of K . Q^T, 32-dim output tiles
    constexpr int CH = D / 8;                // 16-byte chunks of a row
    constexpr int PCS = 64 * CH / VM_NT;     // chunks of a page's K (and V) rows per thread
    constexpr int IMG = 32 * 2 * D;          // bytes of one 32-key image of T rows
    constexpr bool CAN_TWO = REP * VERIFY_MAX_SEG_ROWS > 32;
    static_assert(PCS >= 2 && DT >= 2, "head_dim 64 or 128");
    __shared__ __attribute__((aligned(16))) char s_kv[4 * IMG];  // K images 0, 1, then V images 0, 1
    __shared__ float s_ml[2][64][2];
    char *const k_lds = s_kv, *const v_lds = s_kv + 2 * IMG;
    float *const s_acc = reinterpret_cast<float *>(s_kv);  // [2 waves][DT * 16 registers][64 lanes] once the scoring is over: 256 D bytes, the images' size

    const int g = blockIdx.x, split = blockIdx.y, seg = blockIdx.z, q0 = g * REP;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    // every index that comes from device memory is clamped before it addresses anything
    const int r0 = vm_clamp(a.seg_first[seg], 0, a.N);
    const int n = vm_clamp(a.seg_first[seg + 1], r0, min(a.N, r0 + VERIFY_MAX_SEG_ROWS)) - r0;
    if (n <= 0) return;  // idle slot
    const int cap_pos = a.bt_stride * 64;
    int Tmax = 0;
    for (int i = 0; i < n; ++i) Tmax = max(Tmax, vm_clamp(a.row_ctx[r0 + i], 0, cap_pos));
    const AttnSplit sp = attn_split(Tmax, a.splits);
    if (split >= sp.active) {  // uniform for the workgroup: the neutral partial (one split and no position at all: zeros)
        for (int o = threadIdx.x; o < n * REP * (D / 2); o += VM_NT) {
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
    const int *bt = a.block_table + (size_t)vm_clamp(a.row_seq[r0], 0, a.B - 1) * a.bt_stride;
    const size_t page_elems = (size_t)2 * 64 * a.Hkv * D;
    const unsigned last_page = (unsigned)a.n_pages - 1u;

    // wave roles
    const int C = n * REP;
    const bool two = CAN_TWO && C > 32;
    const int kb = wave >> 1, sub = wave & 1;
    const int dt0 = two ? 0 : sub * (DT / 2), ndt = two ? DT : DT / 2;  // the output tiles this wave accumulates: oacc[j] = tile dt0 + j
    const int cc = (two ? 32 * sub : 0) + c;                            // this lane's column
    const bool col_on = cc < C;
    const int cq = col_on ? cc : C - 1, ci = cq / REP, chd = cq % REP;
    const int ctx_c = col_on ? vm_clamp(a.row_ctx[r0 + ci], 0, cap_pos) : 0;  // a padding column attends nothing
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
    auto fetch = [&](int p) {  // page p's rows of this kv-head: 64 x D of K, contiguous, and the same of V
        const unsigned pg = min((unsigned)bt[p], last_page);  // a corrupt table must not become a wild address
        const uint4 *kp = reinterpret_cast<const uint4 *>(a.slab + (size_t)pg * page_elems + (size_t)g * 64 * D);
        const uint4 *vp = kp + (size_t)a.Hkv * 64 * CH;
#pragma unroll
        for (int j = 0; j < PCS; ++j) kreg[j] = kp[threadIdx.x + j * VM_NT], vreg[j] = vp[threadIdx.x + j * VM_NT];
    };
    const float sl2 = a.scale * ATTN_LOG2E;
    // transposed-read addressing (prefill_attn.hpp): lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p + 3
    const int grp = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;

    fetch(p_first);
    for (int p = p_first; p <= p_last; ++p) {
        __syncthreads();  // the page before is scored
#pragma unroll
        for (int j = 0; j < PCS; ++j) {
            const int x = threadIdx.x + j * VM_NT, row = x / CH, ch = x % CH;
            const bool live = p * 64 + row < Tmax;  // behind the longest context: zeros, whatever the page holds
            const int off = (row >> 5) * IMG + pa_off<D>(row & 31, ch);
            *reinterpret_cast<uint4 *>(k_lds + off) = live ? kreg[j] : make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint4 *>(v_lds + off) = live ? vreg[j] : make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        if (p < p_last) fetch(p + 1);  // in flight under the scoring
        const int tb = p * 64 + kb * 32;
        if (tb >= t_end || tb + 32 <= t_begin) continue;  // wave-uniform: an image outside the split
        const char *kimg = k_lds + kb * IMG, *vimg = v_lds + kb * IMG;

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
            sc[i] = (t >= t_begin && t < t_hi) ? sacc[i] * sl2 : ATTN_NEG;
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
            const float ha = round_T<T>(pa), hb = round_T<T>(pb);
            phi[i >> 1] = pack2<T>(ha, hb);
            plo[i >> 1] = pack2<T>(pa - ha, pb - hb);
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
int verify_attn_mfma_launch_rep(const VerifyAttnArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)a.Hkv, (unsigned)a.splits, (unsigned)a.B);
#define VM_GO(R)                                                                                   \
    hipLaunchKernelGGL((k_paged_attn_verify_mfma<T, D, R>), grid, dim3(VM_NT), 0, st, a);          \
    break
    switch (a.Hq / a.Hkv) {
        case 1: VM_GO(1);
        case 2: VM_GO(2);
        case 3: VM_GO(3);
        case 4: VM_GO(4);
        case 5: VM_GO(5);
        case 6: VM_GO(6);
        case 7: VM_GO(7);
        case 8: VM_GO(8);
        default: return pie::fail(PIE_E_SHAPE, "paged_attn_verify_mfma: n_heads / n_kv_heads must be between 1 and 8");
    }
#undef VM_GO
    PIE_LAUNCH_CHECK();
    return a.splits > 1 ? verify_attn_merge_launch(std::is_same<T, BF16>::value ? PIE_BF16 : PIE_F16, D, a, st) : PIE_OK;
}

}  // namespace

// The T kernel's target, two workgroups per CU: a position here carries twice the int8 kernel's bytes under the same MFMAs, so a split
// half as long weighs as much against the workgroup's fixed part (DESIGN.md 28 has the measurement against 256)
int paged_attn_verify_mfma_splits(int B, int Hkv, int max_blocks) {
    if (B < 1 || Hkv < 1 || max_blocks < 1) return 1;
    int splits = (512 + B * Hkv - 1) / (B * Hkv);
    splits = splits > ATTN_MAX_SPLITS ? ATTN_MAX_SPLITS : splits;
    splits = splits > max_blocks ? max_blocks : splits;
    return splits < 1 ? 1 : splits;
}

int paged_attn_verify_mfma_launch(int dtype, int D, const VerifyAttnArgs &a, hipStream_t st) {
    if (dtype == PIE_BF16 && D == 128) return verify_attn_mfma_launch_rep<BF16, 128>(a, st);
    if (dtype == PIE_BF16 && D == 64) return verify_attn_mfma_launch_rep<BF16, 64>(a, st);
    if (dtype == PIE_F16 && D == 128) return verify_attn_mfma_launch_rep<F16, 128>(a, st);
    if (dtype == PIE_F16 && D == 64) return verify_attn_mfma_launch_rep<F16, 64>(a, st);
    return pie::fail(PIE_E_SHAPE, "paged_attn_verify_mfma: head_dim must be 64 or 128 and dtype bf16 / f16");
}

extern "C" {

int pie_paged_attn_verify_mfma_splits(int B, int Hkv, int max_blocks) { return paged_attn_verify_mfma_splits(B, Hkv, max_blocks); }

int pie_paged_attn_verify_mfma(const void *q, const void *slab, size_t n_pages, const int32_t *block_tables, int max_blocks, const int32_t *row_seq,
                               const int32_t *row_context_lens, const int32_t *seg_first, int N, int B, int Hq, int Hkv, int D, float scale, int dtype,
                               int splits, void *out, void *workspace, void *stream) {
    PIE_REQUIRE(q && slab && block_tables && row_seq && row_context_lens && seg_first && out && workspace, PIE_E_ARG, "pie_paged_attn_verify_mfma: null pointer");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_paged_attn_verify_mfma: dtype must be PIE_BF16 or PIE_F16");
    PIE_REQUIRE(splits >= 0 && splits <= ATTN_MAX_SPLITS, PIE_E_ARG, "pie_paged_attn_verify_mfma: splits must be 0 (chosen here) or 1..32");
    PIE_REQUIRE(N >= 1 && N <= 65535 && B >= 1 && B <= 65535 && max_blocks > 0 && max_blocks <= (1 << 24) && n_pages > 0 && n_pages < 0x7FFFFFFFu, PIE_E_SHAPE,
                "pie_paged_attn_verify_mfma: bad batch shape");
    PIE_REQUIRE(D == 64 || D == 128, PIE_E_SHAPE, "pie_paged_attn_verify_mfma: head_dim must be 64 or 128");
    PIE_REQUIRE(Hkv > 0 && Hq > 0 && Hq % Hkv == 0 && Hq / Hkv <= 8, PIE_E_SHAPE, "pie_paged_attn_verify_mfma: n_heads must be 1..8 times n_kv_heads");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(slab, 16) && pie_aligned(out, 16) && pie_aligned(workspace, 16), PIE_E_ALIGN,
                "pie_paged_attn_verify_mfma: q, slab, out and workspace need 16-byte alignment");
    PIE_REQUIRE(pie_aligned(block_tables, 4) && pie_aligned(row_seq, 4) && pie_aligned(row_context_lens, 4) && pie_aligned(seg_first, 4), PIE_E_ALIGN,
                "pie_paged_attn_verify_mfma: the index arrays need 4-byte alignment");
    VerifyAttnArgs a = {};
    a.q = (const u16 *)q, a.slab = (const u16 *)slab, a.block_table = block_tables, a.row_seq = row_seq, a.row_ctx = row_context_lens, a.seg_first = seg_first;
    a.N = N, a.B = B, a.Hq = Hq, a.Hkv = Hkv, a.bt_stride = max_blocks, a.n_pages = (int)n_pages, a.scale = scale;
    a.splits = splits ? splits : paged_attn_verify_mfma_splits(B, Hkv, max_blocks);
    a.part_acc = (float *)workspace;
    a.part_ml = a.part_acc + (size_t)N * Hq * a.splits * D;
    a.out = (u16 *)out;
    return paged_attn_verify_mfma_launch(dtype, D, a, (hipStream_t)stream);
}

}  // extern "C"
