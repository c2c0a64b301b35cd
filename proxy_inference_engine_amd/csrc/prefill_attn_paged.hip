// prefill_attn_paged.hip -- causal attention of prompt chunks that continue a cached prefix, over T pages: every chunk of a pass in ONE
// launch on the MFMA units, split over keys where the launch has too few query tiles to fill the chip.
//
// pie_prefill_attn_i8's contract on T pages: a chunk is {first row, rows M, cached positions P >= 1, block-table row}; query row r sits at
// position P + r and attends keys 0 .. P + r of its sequence's pages (K block then V block, each [Hkv, 64, D]), which already hold the
// chunk's own rows.  k_prefill_attn_paged, grid (kv-heads x key splits x query tiles, chunks), max(REP * QT, 4) waves:
//   * up to 32 chunk descriptors ride in the kernel arguments by value (no device copy, no host sync); blockIdx.y is the chunk, and a
//     workgroup beyond its chunk's own tile count exits at once;
//   * the kv-group is the fastest index of the block id, then the split, tiles longest first (k_prefill_attn's XCD argument: an XCD's L2 holds
//     one group's pages).  A workgroup owns a 32 QT-row query tile, one kv-group and one split: split s of a tile is the s-th run of
//     ceil(pages / splits) WHOLE pages of the pages the tile's last row sees, so no split starts inside a page; a split behind those pages
//     exits and writes nothing (pp_split gives the merge the same count);
//   * wave w < REP * QT owns tile w / REP and q-head g REP + w % REP and keeps its Q fragments in VGPRs; with fewer than four such waves the
//     workgroup is filled up to four by waves that only stage (a page of a kv-head is 16 KB at D = 128: 64 lanes would hold 128 VGPRs of it in
//     flight, 256 lanes hold 32);
//   * the 64 x D elements of (page, kv-head) of K and of V -- contiguous, 16-byte loads, fetched into registers one page ahead of their use --
//     go unconverted into LDS as two 32-key K images and two V images in prefill_attn.hpp's dual-use swizzle: a WHOLE page per barrier pair
//     (32 KB at D = 128), half of k_prefill_attn's barriers per key.  Positions behind the chunk's last one are stored as zeros, whatever
//     the page holds; a page behind every row of the tile is never addressed; a table entry is clamped to n_pages - 1;
//   * per 32-key image, k_prefill_attn's order and arithmetic: S^T[key, row] = K . Q^T (v_mfma_f32_32x32x16, A = K rows by ds_read_b128,
//     B = the Q fragments), score = acc * scale * log2e, base-2 online softmax over registers in fp32, p split into hi + lo halves of T as
//     the B operand of O^T[dim, row] += V^T . P^T with A = V^T through ds_read_b64_tr_b16.  Only an image that crosses the wave's diagonal
//     pays the per-element causal mask (a wave-uniform branch), an image wholly behind the wave's last row is skipped;
//   * one split: normalise and store T -- bit for bit what k_prefill_attn stores for the chunk launched alone.  More: fp32 partials
//     (D accumulators, m, l) per (chunk row, head, split) in k_paged_attn_verify's layout over the chunks' rows only; a row that sees no key
//     of an active split leaves the neutral partial (m = ATTN_NEG, l = 0, zeros) by construction.  k_prefill_attn_paged_merge then merges
//     the active splits of every chunk row in split order and writes those rows of `out`, no other.
#include "prefill_attn_paged.hpp"
#include "prefill_attn.hpp"

namespace {

struct PrefillPagedChunk {
    int first, rows, cached, seq;  // first row of the batch, rows M >= 1, cached positions P >= 1, block-table row
    int part_row;                  // the chunk's first row among the partials
};
struct PrefillPagedChunks {
    PrefillPagedChunk ch[PREFILL_PAGED_MAX_CHUNKS];
};

// pages of the keys the query tile at rows wg_r0 .. wg_r0 + BM - 1 sees (its last row's page, inside the block table), and their cut
struct PpSplit {
    int pages, per, active;  // pages of the tile; whole pages per split; splits that hold at least one
};
__device__ __forceinline__ PpSplit pp_split(int P, int M, int wg_r0, int BM, int bt_stride, int splits) {
    PpSplit s;
    s.pages = min((P + min(wg_r0 + BM, M) - 1) >> 6, bt_stride - 1) + 1;
    s.per = (s.pages + splits - 1) / splits;
    s.active = (s.pages + s.per - 1) / s.per;
    return s;
}

constexpr int pp_waves(int REP, int QT) { return REP * QT < 4 ? 4 : REP * QT; }

template <class T, int D, int REP, int QT>
__global__ void __launch_bounds__(pp_waves(REP, QT) * 64) k_prefill_attn_paged(const PrefillPagedArgs a, const PrefillPagedChunks cs) {
    constexpr int WAVES = REP * QT, NT = pp_waves(REP, QT) * 64, BM = 32 * QT;
    constexpr int KS = D / 16, DT = D / 32;     // k-steps of K . Q^T, 32-dim output tiles
    constexpr int CH = D / 8;                   // 16-byte chunks of a row
    constexpr int PIECES = 64 * CH;             // ... of a page's K (and V) block of one kv-head
    constexpr int PCS = (PIECES + NT - 1) / NT; // ... per thread
    constexpr int IMG = 32 * 2 * D;             // bytes of one 32-key image of T rows
    static_assert(DT >= 2 && PCS >= 1 && PCS <= 4, "head_dim 64 or 128");
    __shared__ __attribute__((aligned(16))) char s_kv[4 * IMG];  // K images 0, 1, then V images 0, 1
    char *const k_lds = s_kv, *const v_lds = s_kv + 2 * IMG;

    const PrefillPagedChunk ck = cs.ch[blockIdx.y];
    const int M = ck.rows, P = ck.cached;
    const int g = (int)blockIdx.x % a.Hkv, rest = (int)blockIdx.x / a.Hkv;
    const int split = rest % a.splits, tile = rest / a.splits;
    const int tiles = (M + BM - 1) / BM;
    if (tile >= tiles) return;  // a shorter chunk of the launch
    const int wg_r0 = (tiles - 1 - tile) * BM;  // longest first
    const PpSplit sp = pp_split(P, M, wg_r0, BM, a.bt_stride, a.splits);
    if (split >= sp.active) return;  // no page of the tile's keys is left for this split: the merge does not read it
    const int p_begin = split * sp.per, p_end = min(sp.pages, p_begin + sp.per);  // p_begin < p_end <= bt_stride

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int r0 = wg_r0 + 32 * (wave / REP), hq = g * REP + wave % REP;  // this wave's 32-row tile and q-head
    const int t_end = P + M;                                               // positions the chunk's pages hold
    const bool wave_on = wave < WAVES && r0 < M;                           // (a staging wave; QT = 2: the second tile of a chunk's last workgroup may be empty)
    const int t_w0 = P + r0, t_wlast = P + min(r0 + 32, M) - 1;           // positions of the wave's first and last row
    const int *bt = a.block_tables + (size_t)ck.seq * a.bt_stride;
    const size_t page_elems = (size_t)2 * 64 * a.Hkv * D;
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

    uint4 kreg[PCS], vreg[PCS];  // (constant indices under full unrolling: registers, no scratch -- the resources table of DESIGN.md 30)
    auto fetch = [&](int p) {    // page p's rows of this kv-head: 64 x D of K, contiguous, and the same of V
        const unsigned pg = min((unsigned)bt[p], last_page);  // a corrupt table must not become a wild address
        const uint4 *kp = reinterpret_cast<const uint4 *>(a.slab + (size_t)pg * page_elems + (size_t)g * 64 * D);
        const uint4 *vp = kp + (size_t)a.Hkv * 64 * CH;
#pragma unroll
        for (int j = 0; j < PCS; ++j) {
            const int x = threadIdx.x + j * NT;
            if (PIECES % NT == 0 || x < PIECES) kreg[j] = kp[x], vreg[j] = vp[x];
        }
    };
    const float sl2 = a.scale * ATTN_LOG2E;
    // transposed-read addressing (prefill_attn.hpp): lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p + 3
    const int grp = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;

    // one 32-key image against the wave's 32 rows, in k_prefill_attn's order; crosses (wave-uniform): the image reaches beyond the wave's
    // first row, so some key is masked for some row -- an image that does not is that kernel's arithmetic with every condition true
    auto image = [&](bool crosses, const char *kimg, const char *vimg, int tb) {
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
        for (int i = 0; i < 16; ++i) sc[i] = sacc[i] * sl2;
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
        float pr[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) pr[i] = attn_exp2(sc[i] - m_run);
        if (crosses) {  // a split's first image may hold no key at all for a row (m_run still ATTN_NEG: exp2(0) = 1): p is masked by position, never by value
#pragma unroll
            for (int i = 0; i < 16; ++i) pr[i] = tb + (i & 3) + 8 * (i >> 2) + 4 * h <= t_row ? pr[i] : 0.0f;
        }
        u32 phi[8], plo[8];
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
            const float pa = pr[i], pb = pr[i + 1];
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

    fetch(p_begin);
    for (int p = p_begin; p < p_end; ++p) {
        __syncthreads();  // the page before is scored
#pragma unroll
        for (int j = 0; j < PCS; ++j) {
            const int x = threadIdx.x + j * NT, row = x / CH, ch = x % CH;
            if (PIECES % NT == 0 || x < PIECES) {
                const bool live = p * 64 + row < t_end;  // behind the chunk's last position: zeros, whatever the page holds
                const int off = (row >> 5) * IMG + pa_off<D>(row & 31, ch);
                *reinterpret_cast<uint4 *>(k_lds + off) = live ? kreg[j] : make_uint4(0u, 0u, 0u, 0u);
                *reinterpret_cast<uint4 *>(v_lds + off) = live ? vreg[j] : make_uint4(0u, 0u, 0u, 0u);
            }
        }
        __syncthreads();
        if (p + 1 < p_end) fetch(p + 1);  // in flight under the scoring
        if (!wave_on) continue;
#pragma nounroll
        for (int kb = 0; kb < 2; ++kb) {
            const int tb = p * 64 + kb * 32;
            if (tb > t_wlast) break;  // wave-uniform: behind the wave's last row
            image(tb + 31 > t_w0, k_lds + kb * IMG, v_lds + kb * IMG, tb);
        }
    }
    if (!wave_on || r0 + c >= M) return;
    // the pair (lane, lane ^ 32) shares the query row and holds the two halves of the row sum
    const float l_sum = xor32_sum(l_run);
    if (a.splits == 1) {  // the partial IS the result (a row attends P + r + 1 >= 2 keys: l > 0)
        const float inv = 1.0f / l_sum;
        u16 *orow = a.out + ((size_t)(ck.first + r0 + c) * a.Hq + hq) * D;
        // k_prefill_attn's two roundings, product to fp32 then to T: without the packed fp32 forms the compiler would fuse an f16 store's
        // pair into v_fma_mixlo_f16, ONE rounding, and one element in 2^13 would land on the other neighbour (measured)
        auto prod = [&](float x) {
            float y = x * inv;
            asm volatile("" : "+v"(y));
            return y;
        };
#pragma unroll
        for (int j = 0; j < DT; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // registers 4k .. 4k + 3 <-> dims 32 j + 8 k + 4 h + {0..3}
                const uint2 o = make_uint2(pack2<T>(prod(oacc[j][4 * k]), prod(oacc[j][4 * k + 1])), pack2<T>(prod(oacc[j][4 * k + 2]), prod(oacc[j][4 * k + 3])));
                *reinterpret_cast<uint2 *>(orow + 32 * j + 8 * k + 4 * h) = o;
            }
        return;
    }
    const size_t part = ((size_t)(ck.part_row + r0 + c) * a.Hq + hq) * a.splits + split;
#pragma unroll
    for (int j = 0; j < DT; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            *reinterpret_cast<float4 *>(a.part_acc + part * D + 32 * j + 8 * k + 4 * h) =
                make_float4(oacc[j][4 * k], oacc[j][4 * k + 1], oacc[j][4 * k + 2], oacc[j][4 * k + 3]);
    if (h == 0) a.part_ml[part * 2 + 0] = m_run, a.part_ml[part * 2 + 1] = l_sum;  // (the pair holds the same maximum)
}

// The merge of the chunks' rows, and of no other row of `out`: grid (rows of the longest chunk, chunks), row r of chunk y merges the active
// splits of ITS tile in split order (split 0 holds key 0, which every row sees: the maximum is finite and the sum positive).
template <class T>
__global__ void __launch_bounds__(256) k_prefill_attn_paged_merge(const PrefillPagedArgs a, const PrefillPagedChunks cs, const int D, const int BM) {
    const PrefillPagedChunk ck = cs.ch[blockIdx.y];
    const int r = blockIdx.x;
    if (r >= ck.rows) return;
    const int active = pp_split(ck.cached, ck.rows, r / BM * BM, BM, a.bt_stride, a.splits).active;
    const int D4 = D / 4;
    for (int o = threadIdx.x; o < a.Hq * D4; o += 256) {
        const int hq = o / D4, d = (o % D4) * 4;
        const size_t base = ((size_t)(ck.part_row + r) * a.Hq + hq) * a.splits;
        float mx = ATTN_NEG;
        for (int j = 0; j < active; ++j) mx = fmaxf(mx, a.part_ml[(base + j) * 2]);
        float l = 0.0f;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int j = 0; j < active; ++j) {
            const float w = attn_exp2(a.part_ml[(base + j) * 2] - mx);  // 0 for a neutral partial
            const float4 pa = *reinterpret_cast<const float4 *>(a.part_acc + (base + j) * D + d);
            l = fmaf(w, a.part_ml[(base + j) * 2 + 1], l);
            acc.x = fmaf(w, pa.x, acc.x), acc.y = fmaf(w, pa.y, acc.y), acc.z = fmaf(w, pa.z, acc.z), acc.w = fmaf(w, pa.w, acc.w);
        }
        *reinterpret_cast<uint2 *>(a.out + ((size_t)(ck.first + r) * a.Hq + hq) * D + d) =
            make_uint2(pack2<T>(acc.x / l, acc.y / l), pack2<T>(acc.z / l, acc.w / l));
    }
}

// prefill_attn_launch_d's rule over the chunks: 2 tiles need 2 rep <= 8 waves, and pay only while the halved grid fills the 256 CUs
bool pp_two_tiles(const int32_t *chunks, int n_chunks, int Hkv, int rep) {
    const int qt = pie_knob(PIE_KNOB_PREFILL_QT);  // test knob, as prefill_attn_launch_d reads it
    long tiles64 = 0;
    int max_rows = 0;
    for (int i = 0; i < n_chunks; ++i) {
        const int m = chunks[4 * (size_t)i + 1];
        max_rows = m > max_rows ? m : max_rows, tiles64 += (m + 63) / 64;
    }
    return rep <= 4 && max_rows > 32 && (qt > 0 ? qt == 2 : tiles64 * Hkv >= 256);
}

template <class T, int D>
int prefill_attn_paged_launch_d(PrefillPagedArgs a, const int32_t *chunks, int n_chunks, hipStream_t st) {
    const int rep = a.Hq / a.Hkv;
    const bool two = pp_two_tiles(chunks, n_chunks, a.Hkv, rep);  // one form for the whole call: the partials of a tile and their merge agree on it
    const int bm = two ? 64 : 32;
    int part_row = 0;
    for (int c0 = 0; c0 < n_chunks; c0 += PREFILL_PAGED_MAX_CHUNKS) {
        const int n = n_chunks - c0 < PREFILL_PAGED_MAX_CHUNKS ? n_chunks - c0 : PREFILL_PAGED_MAX_CHUNKS;
        PrefillPagedChunks cs = {};
        int max_rows = 0;
        for (int i = 0; i < n; ++i) {
            const int32_t *ch = chunks + 4 * (size_t)(c0 + i);
            cs.ch[i] = {ch[0], ch[1], ch[2], ch[3], part_row};
            max_rows = ch[1] > max_rows ? ch[1] : max_rows, part_row += ch[1];
        }
        const dim3 grid((unsigned)(((max_rows + bm - 1) / bm) * a.splits * a.Hkv), (unsigned)n);
#define PP_LAUNCH(R)                                                                                                                        \
    if (two && R <= 4) hipLaunchKernelGGL((k_prefill_attn_paged<T, D, R, (R <= 4 ? 2 : 1)>), grid, dim3(pp_waves(R, R <= 4 ? 2 : 1) * 64), 0, st, a, cs); \
    else hipLaunchKernelGGL((k_prefill_attn_paged<T, D, R, 1>), grid, dim3(pp_waves(R, 1) * 64), 0, st, a, cs);                          \
    break
        switch (rep) {
            case 1: PP_LAUNCH(1);
            case 2: PP_LAUNCH(2);
            case 3: PP_LAUNCH(3);
            case 4: PP_LAUNCH(4);
            case 5: PP_LAUNCH(5);
            case 6: PP_LAUNCH(6);
            case 7: PP_LAUNCH(7);
            case 8: PP_LAUNCH(8);
            default: return pie::fail(PIE_E_SHAPE, "prefill_attn_paged: n_heads / n_kv_heads must be between 1 and 8");
        }
#undef PP_LAUNCH
        PIE_LAUNCH_CHECK();
        if (a.splits > 1) {
            hipLaunchKernelGGL((k_prefill_attn_paged_merge<T>), dim3((unsigned)max_rows, (unsigned)n), dim3(256), 0, st, a, cs, D, bm);
            PIE_LAUNCH_CHECK();
        }
    }
    return PIE_OK;
}

}  // namespace

int prefill_attn_paged_splits(const int32_t *chunks, int n_chunks, int Hkv, int rep, int force) {
    if (!chunks || n_chunks < 1 || Hkv < 1 || rep < 1) return 1;
    const int bm = pp_two_tiles(chunks, n_chunks, Hkv, rep) ? 64 : 32;
    long tiles = 0, rows = 0;
    long max_pages = 1;
    for (int i = 0; i < n_chunks; ++i) {
        const int32_t *ch = chunks + 4 * (size_t)i;
        const long pages = ((long)ch[2] + ch[1] + PIE_PAGE_TOKENS - 1) / PIE_PAGE_TOKENS;
        tiles += (ch[1] + bm - 1) / bm, rows += ch[1];
        max_pages = pages > max_pages ? pages : max_pages;
    }
    const long wgs = tiles * Hkv > 0 ? tiles * Hkv : 1;
    long splits = force > 0 ? force : (wgs >= PREFILL_PAGED_TARGET_WGS ? 1 : (PREFILL_PAGED_TARGET_WGS + wgs - 1) / wgs);
    splits = splits > ATTN_MAX_SPLITS ? ATTN_MAX_SPLITS : splits;
    splits = splits > max_pages ? max_pages : splits;
    if (force <= 0 && splits > max_pages / PREFILL_PAGED_MIN_SPLIT_PAGES) splits = max_pages / PREFILL_PAGED_MIN_SPLIT_PAGES;  // (a forced count may cut page by page)
    // the partials of the call at head_dim 128 stay inside PREFILL_PAGED_WS_CAP (one split needs none)
    const size_t per_split = (size_t)(rows > 0 ? rows : 1) * Hkv * rep * (128 + 2) * sizeof(float);
    const long cap = (long)(PREFILL_PAGED_WS_CAP / per_split);
    splits = splits > cap ? cap : splits;
    return splits < 1 ? 1 : (int)splits;
}

size_t prefill_attn_paged_workspace_bytes(const int32_t *chunks, int n_chunks, int Hq, int D, int splits) {
    if (!chunks || splits <= 1 || n_chunks < 1 || Hq < 1 || D < 1) return 0;
    size_t rows = 0;
    for (int i = 0; i < n_chunks; ++i) rows += (size_t)(chunks[4 * (size_t)i + 1] > 0 ? chunks[4 * (size_t)i + 1] : 0);
    return rows * Hq * splits * (D + 2) * sizeof(float);
}

int prefill_attn_paged_launch(int dtype, int D, const PrefillPagedArgs &a, const int32_t *chunks, int n_chunks, hipStream_t st) {
    if (a.splits < 1 || a.splits > ATTN_MAX_SPLITS || (a.splits > 1 && !(a.part_acc && a.part_ml)))
        return pie::fail(PIE_E_ARG, "prefill_attn_paged: splits must be 1..32, with partials beyond one");
    if (dtype == PIE_BF16 && D == 128) return prefill_attn_paged_launch_d<BF16, 128>(a, chunks, n_chunks, st);
    if (dtype == PIE_BF16 && D == 64) return prefill_attn_paged_launch_d<BF16, 64>(a, chunks, n_chunks, st);
    if (dtype == PIE_F16 && D == 128) return prefill_attn_paged_launch_d<F16, 128>(a, chunks, n_chunks, st);
    if (dtype == PIE_F16 && D == 64) return prefill_attn_paged_launch_d<F16, 64>(a, chunks, n_chunks, st);
    return pie::fail(PIE_E_SHAPE, "prefill_attn_paged: head_dim must be 64 or 128 and dtype bf16 / f16");
}

extern "C" {

int pie_prefill_attn_paged_splits(const int32_t *chunks_host, int n_chunks, int Hq, int Hkv) {
    if (Hkv < 1 || Hq < Hkv || Hq % Hkv) return 1;
    return prefill_attn_paged_splits(chunks_host, n_chunks, Hkv, Hq / Hkv);
}

size_t pie_prefill_attn_paged_workspace_bytes(const int32_t *chunks_host, int n_chunks, int Hq, int D, int splits) {
    return prefill_attn_paged_workspace_bytes(chunks_host, n_chunks, Hq, D, splits);
}

int pie_prefill_attn_paged(const void *q, const void *slab, size_t n_pages, size_t slab_bytes, const int32_t *block_tables, int n_seqs, int max_blocks,
                           const int32_t *chunks_host, int n_chunks, int N, int Hq, int Hkv, int D, int dtype, float scale, int splits, void *out, void *workspace,
                           void *stream) {
    PIE_REQUIRE(q && slab && block_tables && chunks_host && out, PIE_E_ARG, "pie_prefill_attn_paged: null pointer");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_prefill_attn_paged: dtype must be PIE_BF16 or PIE_F16");
    PIE_REQUIRE(splits >= 0 && splits <= ATTN_MAX_SPLITS, PIE_E_ARG, "pie_prefill_attn_paged: splits must be 0 (chosen here) or 1..32");
    PIE_REQUIRE(N >= 1 && N <= 65535 && n_chunks >= 1 && n_chunks <= N && n_seqs >= 1 && n_seqs <= 65535 && max_blocks > 0 && max_blocks <= (1 << 24) && n_pages > 0 &&
                    n_pages < 0x7FFFFFFFu,
                PIE_E_SHAPE, "pie_prefill_attn_paged: bad batch shape");
    PIE_REQUIRE(D == 64 || D == 128, PIE_E_SHAPE, "pie_prefill_attn_paged: head_dim must be 64 or 128");
    PIE_REQUIRE(Hkv > 0 && Hq > 0 && Hq % Hkv == 0 && Hq / Hkv <= 8, PIE_E_SHAPE, "pie_prefill_attn_paged: n_heads must be 1..8 times n_kv_heads");
    PIE_REQUIRE(slab_bytes / ((size_t)2 * PIE_PAGE_TOKENS * Hkv * D * 2) >= n_pages, PIE_E_SHAPE, "pie_prefill_attn_paged: the slab is smaller than n_pages T pages");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(slab, 16) && pie_aligned(out, 16) && pie_aligned(workspace, 16), PIE_E_ALIGN,
                "pie_prefill_attn_paged: q, slab, out and workspace need 16-byte alignment");
    PIE_REQUIRE(pie_aligned(block_tables, 4) && pie_aligned(chunks_host, 4), PIE_E_ALIGN, "pie_prefill_attn_paged: the index arrays need 4-byte alignment");
    size_t rows = 0;
    for (int ci = 0; ci < n_chunks; ++ci) {
        const int32_t *ch = chunks_host + 4 * (size_t)ci;
        PIE_REQUIRE(ch[0] >= 0 && ch[1] >= 1 && ch[1] <= N && ch[0] <= N - ch[1] && ch[2] >= 1 && ch[2] <= (1 << 30) && ch[3] >= 0 && ch[3] < n_seqs &&
                        ((int64_t)ch[2] + ch[1] + PIE_PAGE_TOKENS - 1) / PIE_PAGE_TOKENS <= max_blocks,
                    PIE_E_SHAPE, "pie_prefill_attn_paged: a chunk is {first row >= 0, rows >= 1, cached positions >= 1, sequence < n_seqs} inside the batch and its block table");
        rows += (size_t)ch[1];
    }
    PrefillPagedArgs a = {};
    a.q = (const u16 *)q, a.slab = (const u16 *)slab, a.block_tables = block_tables, a.out = (u16 *)out;
    a.Hq = Hq, a.Hkv = Hkv, a.bt_stride = max_blocks, a.n_pages = (int)n_pages, a.scale = scale;
    a.splits = splits ? splits : prefill_attn_paged_splits(chunks_host, n_chunks, Hkv, Hq / Hkv);
    PIE_REQUIRE(a.splits == 1 || workspace, PIE_E_ARG, "pie_prefill_attn_paged: more than one split needs a workspace (pie_prefill_attn_paged_workspace_bytes)");
    a.part_acc = (float *)workspace;
    a.part_ml = a.part_acc + rows * Hq * a.splits * D;
    return prefill_attn_paged_launch(dtype, D, a, chunks_host, n_chunks, (hipStream_t)stream);
}

}  // extern "C"
