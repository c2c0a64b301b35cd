// prefill_attn_i8.hip -- causal attention of prompt chunks that continue a cached prefix, over int8 pages, on the MFMA units.
//
// A chunk is {first row, rows M, cached positions P >= 1, block-table row}: query row r of the chunk sits at absolute position P + r and
// attends keys 0 .. P + r of its sequence's pages, which already hold the chunk's own rows as codes (the RoPE + append launch quantises in
// front).  Pages and arithmetic are paged_i8.hip's: x' = fp32(q8) * fp32(s) with the page's per-head fp16 scale, fp32 afterwards, base-2
// online softmax, one rounding to T at the end.  k_prefill_attn_i8, grid (tiles x kv-heads, chunks), REP * QT waves:
//   * ONE launch per layer for up to 32 chunks: their descriptors ride in the kernel arguments by value (512 bytes: no device copy, no
//     host sync); blockIdx.y is the chunk, and a workgroup beyond its chunk's own tile count exits at once;
//   * a workgroup owns a 32 QT-row query tile of one chunk and one kv-head group (the group is the fastest index of the block id, tiles
//     longest first); wave w owns tile w / REP and q-head g REP + w % REP -- k_prefill_attn's split -- and keeps its Q fragments in VGPRs;
//   * the 64 x D codes of (page, kv-head) -- contiguous, 16-byte loads, fetched into registers one page ahead of their use, the page's two
//     scales with them -- are converted to T ONCE per workgroup on the way into LDS (integers up to 127 are exact in bf16 and f16) and
//     stored as two 32-key K images and two V images in prefill_attn.hpp's dual-use swizzle: a WHOLE page per barrier pair (32 KB at
//     D = 128), every wave walks both images, half of k_prefill_attn's barriers per key.  Codes behind the chunk's last position are
//     stored as zeros; a page behind every row of the tile is never addressed and its scales are never read; a table entry is clamped to
//     n_pages - 1 before it addresses anything;
//   * per 32-key image: S^T[key, row] = K . Q^T (v_mfma_f32_32x32x16, A = K rows by ds_read_b128, B = the Q fragments), the score =
//     acc * (scale * log2e * k_scale[page, g]) in fp32; only an image that crosses the wave's diagonal pays the per-element causal mask
//     (a wave-uniform branch around sixteen selects), an image behind the wave's last row is skipped; the reduction runs over registers; the value
//     operand p * v_scale[page, g] (over the first page's, see below) in fp32, split into hi + lo halves of T, is directly the B operand of O^T[dim, row] += V^T . P^T,
//     whose A = V^T comes through ds_read_b64_tr_b16 of the row-major V image; l accumulates the unscaled p;
//   * no KV split and nothing to merge: a wave owns its rows' whole key range.
#include "prefill_attn_i8.hpp"
#include "prefill_attn.hpp"

namespace {

struct PrefillI8Chunks {
    PrefillI8Chunk ch[PREFILL_I8_MAX_CHUNKS];
};

__device__ __forceinline__ float pi_f16(u32 bits) { return (float)__builtin_bit_cast(_Float16, (u16)bits); }
// codes j and j + 1 of a word as a T pair: exact (paged_attn_verify_i8.hip's converter, restated: that file's code stays as measured)
template <class T>
__device__ __forceinline__ u32 pi_codes2(u32 w, int j) {
    return pack2<T>((float)(int)(signed char)(w >> (8 * j)), (float)(int)(signed char)(w >> (8 * j + 8)));
}

template <class T, int D, int REP, int QT>
__global__ void __launch_bounds__(REP * QT * 64) k_prefill_attn_i8(const PrefillI8Args a, const PrefillI8Chunks cs, const size_t page_bytes) {
    constexpr int NT = REP * QT * 64, BM = 32 * QT;
    constexpr int KS = D / 16, DT = D / 32;     // k-steps of K . Q^T, 32-dim output tiles
    constexpr int PPR = D / 16;                 // 16-code pieces of a row
    constexpr int PIECES = 64 * PPR;            // ... of a page's K (and V) block
    constexpr int PCS = (PIECES + NT - 1) / NT; // ... per thread
    constexpr int IMG = 32 * 2 * D;             // bytes of one 32-key image of T rows
    static_assert(DT >= 2 && PCS >= 1 && PCS <= 8, "head_dim 64 or 128");
    __shared__ __attribute__((aligned(16))) char s_kv[4 * IMG];  // K images 0, 1, then V images 0, 1
    char *const k_lds = s_kv, *const v_lds = s_kv + 2 * IMG;

    const PrefillI8Chunk ck = cs.ch[blockIdx.y];
    const int M = ck.rows, P = ck.cached;
    const int g = (int)blockIdx.x % a.Hkv, tile = (int)blockIdx.x / a.Hkv;
    const int tiles = (M + BM - 1) / BM;
    if (tile >= tiles) return;  // a shorter chunk of the launch
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int wg_r0 = (tiles - 1 - tile) * BM;                             // longest first
    const int r0 = wg_r0 + 32 * (wave / REP), hq = g * REP + wave % REP;  // this wave's 32-row tile and q-head
    const int t_end = P + M;                                               // positions the chunk's pages hold
    const int p_last = min((P + min(wg_r0 + BM, M) - 1) >> 6, a.bt_stride - 1);  // the page of the tile's last row: below bt_stride
    const bool wave_on = r0 < M;                                           // (QT = 2: the second tile of a chunk's last workgroup may be empty)
    const int t_w0 = P + r0, t_wlast = P + min(r0 + 32, M) - 1;           // positions of the wave's first and last row
    const int *bt = a.block_tables + (size_t)ck.seq * a.bt_stride;
    const char *slab = reinterpret_cast<const char *>(a.slab);
    const size_t blk = (size_t)a.Hkv * 64 * D;  // bytes of a page's K (and V) block
    const unsigned last_page = (unsigned)a.n_pages - 1u;

    // Q fragments (B operand of K . Q^T): lane (row c, half h), k-step s holds Q[r0 + c][hq][16 s + 8 h .. + 8]; rows past M are padding, never stored
    const int qrow = ck.first + min(r0 + c, M - 1);
    uint4 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const uint4 *>(a.q + ((size_t)qrow * a.Hq + hq) * D + 16 * s + 8 * h);
    const int t_row = P + r0 + c;  // the last key this lane's row attends

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
        for (int j = 0; j < PCS; ++j) {
            const int x = threadIdx.x + j * NT;
            if (PIECES % NT == 0 || x < PIECES) kreg[j] = kp[x], vreg[j] = vp[x];
        }
        const u16 *scp = reinterpret_cast<const u16 *>(page + 2 * blk);
        sc_next = (u32)scp[g] | ((u32)scp[a.Hkv + g] << 16);
    };
    auto publish = [&](char *img, const uint4 &q8, int row, int pc, bool live) {  // 16 codes -> two 16-byte chunks of T
        uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
        if (live) {
            lo = make_uint4(pi_codes2<T>(q8.x, 0), pi_codes2<T>(q8.x, 2), pi_codes2<T>(q8.y, 0), pi_codes2<T>(q8.y, 2));
            hi = make_uint4(pi_codes2<T>(q8.z, 0), pi_codes2<T>(q8.z, 2), pi_codes2<T>(q8.w, 0), pi_codes2<T>(q8.w, 2));
        }
        char *base = img + (row >> 5) * IMG;
        *reinterpret_cast<uint4 *>(base + pa_off<D>(row & 31, 2 * pc)) = lo;
        *reinterpret_cast<uint4 *>(base + pa_off<D>(row & 31, 2 * pc + 1)) = hi;
    };
    const float sl2 = a.scale * ATTN_LOG2E;
    // transposed-read addressing (prefill_attn.hpp): lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p + 3
    const int grp = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;

    // one 32-key image against the wave's 32 rows; crosses (wave-uniform): the image reaches beyond the wave's first row, so some key is masked
    auto image = [&](bool crosses, const char *kimg, const char *vimg, int tb, float ksl, float vs) {
        // S^T = K . Q^T : rows = keys (registers), cols = query rows (lanes)
        f32x16_t sacc;
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint4 kf = *reinterpret_cast<const uint4 *>(kimg + pa_off<D>(c, 2 * s + h));
            sacc = MfmaT<T>::run(kf, qf[s], sacc);
        }
        // online softmax over keys: register i <-> key tb + (i & 3) + 8 (i >> 2) + 4 h
        float sc[16], mloc = ATTN_NEG;
#pragma unroll
        for (int i = 0; i < 16; ++i) sc[i] = sacc[i] * ksl;
        if (crosses) {  // only these images pay the per-element causal mask
#pragma unroll
            for (int i = 0; i < 16; ++i) sc[i] = tb + (i & 3) + 8 * (i >> 2) + 4 * h <= t_row ? sc[i] : ATTN_NEG;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) mloc = fmaxf(mloc, sc[i]);
        mloc = xor32_max(mloc);  // the other 16 keys of the image live in the partner lane
        const float m_new = fmaxf(m_run, mloc);
        if (m_new > m_run) {  // rare after the first images
            const float alpha = attn_exp2(m_run - m_new);
            l_run *= alpha;
#pragma unroll
            for (int j = 0; j < DT; ++j)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[j][i] *= alpha;
            m_run = m_new;
        }
        // (m_run is finite from the first image on -- key 0 is below every row, P >= 1 -- so a masked score's exp2(ATTN_NEG - m_run) is 0 exactly)
        u32 phi[8], plo[8];
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
            const float pa = attn_exp2(sc[i] - m_run), pb = attn_exp2(sc[i + 1] - m_run);
            l_run += pa + pb;
            const float va = pa * vs, vb = pb * vs;  // the value operand carries the page's V scale (over v_ref)
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
                const int ch = 4 * j + 2 * (grp & 1) + (tp >> 1);
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
    };

    fetch(0);
    // The value operand is p * (v_scale[page, g] / v_ref) with v_ref = the V scale of the sequence's first page, restored in the closing
    // division: where the scales of a head are one number for all pages (scales per layer and head) the operand is p itself, as in
    // k_prefill_attn, and pages that differ keep their ratio.  p * v_scale itself -- scales of 1/128 and less -- sinks the lo half, and at
    // long contexts the hi half, into f16's subnormals: measured, 7.8 % of a row's f16 elements then miss the float64 result.
    const float v_ref0 = pi_f16(sc_next >> 16), v_ref = v_ref0 > 0.0f ? v_ref0 : 1.0f, inv_vref = 1.0f / v_ref;
    for (int p = 0; p <= p_last; ++p) {
        __syncthreads();  // the page before is scored
#pragma unroll
        for (int j = 0; j < PCS; ++j) {
            const int x = threadIdx.x + j * NT, row = x / PPR, pc = x % PPR;
            if (PIECES % NT == 0 || x < PIECES) {
                const bool live = p * 64 + row < t_end;  // behind the chunk's last position: zero codes, whatever the page holds
                publish(k_lds, kreg[j], row, pc, live);
                publish(v_lds, vreg[j], row, pc, live);
            }
        }
        sc_cur = sc_next;
        __syncthreads();
        if (p < p_last) fetch(p + 1);  // in flight under the scoring
        if (!wave_on) continue;
        const float ksl = sl2 * pi_f16(sc_cur & 0xFFFFu), vs = pi_f16(sc_cur >> 16) * inv_vref;
#pragma nounroll
        for (int kb = 0; kb < 2; ++kb) {
            const int tb = p * 64 + kb * 32;
            if (tb > t_wlast) break;  // wave-uniform: behind the wave's last row
            image(tb + 31 > t_w0, k_lds + kb * IMG, v_lds + kb * IMG, tb, ksl, vs);
        }
    }
    // normalise: the pair (lane, lane ^ 32) shares the query row and holds the two halves of the row sum (a row attends P + r + 1 >= 2 keys: l > 0)
    const float l_sum = xor32_sum(l_run) * inv_vref;  // (... and the value operands' common 1 / v_ref)
    if (r0 + c < M) {
        u16 *orow = a.out + ((size_t)(ck.first + r0 + c) * a.Hq + hq) * D;
#pragma unroll
        for (int j = 0; j < DT; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // registers 4k .. 4k + 3 <-> dims 32 j + 8 k + 4 h + {0..3}
                const uint2 o = make_uint2(pack2<T>(oacc[j][4 * k] / l_sum, oacc[j][4 * k + 1] / l_sum),
                                           pack2<T>(oacc[j][4 * k + 2] / l_sum, oacc[j][4 * k + 3] / l_sum));
                *reinterpret_cast<uint2 *>(orow + 32 * j + 8 * k + 4 * h) = o;
            }
    }
}

template <class T, int D>
int prefill_attn_i8_launch_d(const PrefillI8Args &a, const int32_t *chunks, int n_chunks, hipStream_t st) {
    const int rep = a.Hq / a.Hkv;
    const int qt = pie_knob(PIE_KNOB_PREFILL_QT);  // test knob, as prefill_attn_launch_d reads it
    const size_t pb = pie_page_i8_bytes(a.Hkv, D);
    for (int c0 = 0; c0 < n_chunks; c0 += PREFILL_I8_MAX_CHUNKS) {
        const int n = n_chunks - c0 < PREFILL_I8_MAX_CHUNKS ? n_chunks - c0 : PREFILL_I8_MAX_CHUNKS;
        PrefillI8Chunks cs = {};
        int max_rows = 0, tiles64 = 0;
        for (int i = 0; i < n; ++i) {
            const int32_t *ch = chunks + 4 * (size_t)(c0 + i);
            cs.ch[i] = {ch[0], ch[1], ch[2], ch[3]};
            max_rows = ch[1] > max_rows ? ch[1] : max_rows;
            tiles64 += (ch[1] + 63) / 64;
        }
        // prefill_attn_launch_d's rule over the launch's chunks: 2 tiles need 2 rep <= 8 waves, and pay only while the halved grid fills the 256 CUs
        const bool two = rep <= 4 && max_rows > 32 && (qt > 0 ? qt == 2 : tiles64 * a.Hkv >= 256);
        const dim3 grid((unsigned)(((max_rows + (two ? 63 : 31)) / (two ? 64 : 32)) * a.Hkv), (unsigned)n);
#define PI_LAUNCH(R)                                                                                                             \
    if (two && R <= 4) hipLaunchKernelGGL((k_prefill_attn_i8<T, D, R, (R <= 4 ? 2 : 1)>), grid, dim3(R * 128), 0, st, a, cs, pb); \
    else hipLaunchKernelGGL((k_prefill_attn_i8<T, D, R, 1>), grid, dim3(R * 64), 0, st, a, cs, pb);                              \
    break
        switch (rep) {
            case 1: PI_LAUNCH(1);
            case 2: PI_LAUNCH(2);
            case 3: PI_LAUNCH(3);
            case 4: PI_LAUNCH(4);
            case 5: PI_LAUNCH(5);
            case 6: PI_LAUNCH(6);
            case 7: PI_LAUNCH(7);
            case 8: PI_LAUNCH(8);
            default: return pie::fail(PIE_E_SHAPE, "prefill_attn_i8: n_heads / n_kv_heads must be between 1 and 8");
        }
#undef PI_LAUNCH
        PIE_LAUNCH_CHECK();
    }
    return PIE_OK;
}

}  // namespace

int prefill_attn_i8_launch(int dtype, int D, const PrefillI8Args &a, const int32_t *chunks, int n_chunks, hipStream_t st) {
    if (dtype == PIE_BF16 && D == 128) return prefill_attn_i8_launch_d<BF16, 128>(a, chunks, n_chunks, st);
    if (dtype == PIE_BF16 && D == 64) return prefill_attn_i8_launch_d<BF16, 64>(a, chunks, n_chunks, st);
    if (dtype == PIE_F16 && D == 128) return prefill_attn_i8_launch_d<F16, 128>(a, chunks, n_chunks, st);
    if (dtype == PIE_F16 && D == 64) return prefill_attn_i8_launch_d<F16, 64>(a, chunks, n_chunks, st);
    return pie::fail(PIE_E_SHAPE, "prefill_attn_i8: head_dim must be 64 or 128 and dtype bf16 / f16");
}

extern "C" int pie_prefill_attn_i8(const void *q, const void *slab, size_t n_pages, size_t slab_bytes, const int32_t *block_tables, int n_seqs, int max_blocks,
                                   const int32_t *chunks_host, int n_chunks, int N, int Hq, int Hkv, int D, int dtype, float scale, void *out, void *stream) {
    PIE_REQUIRE(q && slab && block_tables && chunks_host && out, PIE_E_ARG, "pie_prefill_attn_i8: null pointer");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_prefill_attn_i8: dtype must be PIE_BF16 or PIE_F16");
    PIE_REQUIRE(N >= 1 && N <= 65535 && n_chunks >= 1 && n_chunks <= N && n_seqs >= 1 && n_seqs <= 65535 && max_blocks > 0 && max_blocks <= (1 << 24) && n_pages > 0 &&
                    n_pages < 0x7FFFFFFFu,
                PIE_E_SHAPE, "pie_prefill_attn_i8: bad batch shape");
    PIE_REQUIRE(D == 64 || D == 128, PIE_E_SHAPE, "pie_prefill_attn_i8: head_dim must be 64 or 128");
    PIE_REQUIRE(Hkv > 0 && Hq > 0 && Hq % Hkv == 0 && Hq / Hkv <= 8, PIE_E_SHAPE, "pie_prefill_attn_i8: n_heads must be 1..8 times n_kv_heads");
    PIE_REQUIRE(slab_bytes / pie_page_i8_bytes(Hkv, D) >= n_pages, PIE_E_SHAPE, "pie_prefill_attn_i8: the slab is smaller than n_pages int8 pages");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(slab, 16) && pie_aligned(out, 16), PIE_E_ALIGN, "pie_prefill_attn_i8: q, slab and out need 16-byte alignment");
    PIE_REQUIRE(pie_aligned(block_tables, 4) && pie_aligned(chunks_host, 4), PIE_E_ALIGN, "pie_prefill_attn_i8: the index arrays need 4-byte alignment");
    for (int ci = 0; ci < n_chunks; ++ci) {
        const int32_t *ch = chunks_host + 4 * (size_t)ci;
        PIE_REQUIRE(ch[0] >= 0 && ch[1] >= 1 && ch[1] <= N && ch[0] <= N - ch[1] && ch[2] >= 1 && ch[2] <= (1 << 30) && ch[3] >= 0 && ch[3] < n_seqs &&
                        ((int64_t)ch[2] + ch[1] + PIE_PAGE_TOKENS - 1) / PIE_PAGE_TOKENS <= max_blocks,
                    PIE_E_SHAPE, "pie_prefill_attn_i8: a chunk is {first row >= 0, rows >= 1, cached positions >= 1, sequence < n_seqs} inside the batch and its block table");
    }
    PrefillI8Args a = {};
    a.q = (const u16 *)q, a.slab = slab, a.block_tables = block_tables, a.out = (u16 *)out;
    a.Hq = Hq, a.Hkv = Hkv, a.bt_stride = max_blocks, a.n_pages = (int)n_pages, a.scale = scale;
    return prefill_attn_i8_launch(dtype, D, a, chunks_host, n_chunks, (hipStream_t)stream);
}
