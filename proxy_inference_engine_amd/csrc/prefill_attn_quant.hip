// prefill_attn_quant.hip -- causal flash attention of M query rows at positions offset .. offset + M - 1 straight from the quantized KV cache
// (QuantizedKVCache: codes u32 [Hkv, cap, D*BITS/32], scales / biases T [Hkv, cap, D/gs]), on the MFMA units.
//
// The cache already holds the rows' own K / V as codes (update_and_fetch quantizes before it attends).  k_prefill_attn_q, grid
// (kv-heads x key splits x query tiles), max(REP * QT, 4) waves:
//   * the kv-group is the fastest index of the block id, then the split, tiles longest first (k_prefill_attn's XCD argument).  A workgroup
//     owns a 32 QT-row query tile, one kv-group and one split: split s of a tile is the s-th run of ceil(blocks / splits) WHOLE 32-key
//     blocks of the keys the tile's last row sees; a split behind those blocks exits and writes nothing (pq_split gives the merge the same count);
//   * wave w < REP * QT owns tile w / REP and q-head g REP + w % REP and keeps its Q fragments in VGPRs; with fewer than four such waves
//     the workgroup is filled up to four by waves that only stage;
//   * a 32-key block is prefetched ONE BLOCK AHEAD IN CODE FORM: a thread holds 8 dims of a row as one dword (4-bit) or one 8-byte load
//     (8-bit) per K and V, plus the group's scale and bias -- 6 or 8 VGPRs per piece against the 8 of two uint4 of T rows, and 0.28-0.53 of
//     their bytes from L2 / HBM.  Keys past the tile's last one are clamped to it (masked later): capacity behind offset + M is never read;
//   * the codes are converted ONCE on the way into LDS, T(s q + b) with k_kv_dequant_prefix's arithmetic (the product rounded to fp32,
//     then the sum, then T), so the [32][D] K and V images hold bit for bit what the dequantize-to-T scratch held, in prefill_attn.hpp's
//     dual-use swizzle: K rows read as the A operand (ds_read_b128), V through ds_read_b64_tr_b16;
//   * per image, k_prefill_attn's order and arithmetic: S^T[key, row] = K . Q^T (v_mfma_f32_32x32x16), score = acc * scale * log2e,
//     base-2 online softmax over registers in fp32, p split into hi + lo halves of T as the B operand of O^T[dim, row] += V^T . P^T.
//     Only an image that crosses the wave's diagonal pays the per-element mask, an image wholly behind the wave's last row is skipped;
//   * one split: normalise and store T -- bit for bit k_prefill_attn over the dequantized rows.  More: fp32 partials (D accumulators,
//     m, l) per (row, head, split); a row that sees no key of an active split leaves the neutral partial (m = ATTN_NEG, l = 0, zeros) by
//     construction.  k_prefill_attn_q_merge merges the active splits of every row in split order.
#include "prefill_attn_quant.hpp"
#include "prefill_attn.hpp"

namespace {

// 32-key blocks of the keys the query tile at rows wg_r0 .. wg_r0 + BM - 1 sees (its last row's block, inside the capacity), and their cut
struct PqSplit {
    int t_last, blocks, per, active;  // last key of the tile; its blocks; whole blocks per split; splits that hold at least one
};
__device__ __forceinline__ PqSplit pq_split(int pos0, int M, int cap, int wg_r0, int BM, int splits) {
    PqSplit s;
    s.t_last = max(min(pos0 + min(wg_r0 + BM, M) - 1, cap - 1), 0);  // a bad offset must not become a wild address
    s.blocks = s.t_last / 32 + 1;
    s.per = (s.blocks + splits - 1) / splits;
    s.active = (s.blocks + s.per - 1) / s.per;
    return s;
}

constexpr int pq_waves(int REP, int QT) { return REP * QT < 4 ? 4 : REP * QT; }

template <class T, int D, int BITS, int REP, int QT>
__global__ void __launch_bounds__(pq_waves(REP, QT) * 64) k_prefill_attn_q(const PrefillQuantArgs a) {
    constexpr int WAVES = REP * QT, NT = pq_waves(REP, QT) * 64, BM = 32 * QT, BK = 32;
    constexpr int KS = D / 16, DT = D / 32;      // k-steps of K . Q^T, 32-dim output tiles
    constexpr int CH = D / 8;                    // 8-element pieces of a row (16 bytes of T)
    constexpr int PIECES = BK * CH;              // ... of a 32-key block of K (and of V)
    constexpr int PCS = (PIECES + NT - 1) / NT;  // ... per thread
    constexpr int CW = D * BITS / 32, WPL = BITS / 4;  // code words per row / per piece
    static_assert(PCS >= 1 && PCS <= 2, "head_dim 64 or 128");
    __shared__ __attribute__((aligned(16))) char k_lds[BK * 2 * D], v_lds[BK * 2 * D];

    const int M = a.M, pos0 = a.state ? a.state->pos : a.offset;
    const int g = (int)blockIdx.x % a.Hkv, rest = (int)blockIdx.x / a.Hkv;
    const int split = rest % a.splits, tile = rest / a.splits;
    const int wg_r0 = ((M + BM - 1) / BM - 1 - tile) * BM;  // longest first
    const PqSplit sp = pq_split(pos0, M, a.cap, wg_r0, BM, a.splits);
    if (split >= sp.active) return;  // no block of the tile's keys is left for this split: the merge does not read it
    const int b_begin = split * sp.per, b_end = min(sp.blocks, b_begin + sp.per);

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int r0 = wg_r0 + 32 * (wave / REP), hq = g * REP + wave % REP;  // this wave's 32-row tile and q-head
    const bool wave_on = wave < WAVES && r0 < M;                          // (a staging wave; QT = 2: the second tile of the last workgroup may be empty)
    const int t_w0 = pos0 + r0, t_wlast = pos0 + min(r0 + 32, M) - 1;    // positions of the wave's first and last row

    // Q fragments (B operand of K . Q^T): lane (row c, half h), k-step s holds Q[r0 + c][hq][16 s + 8 h .. + 8]; rows past M are padding, never stored
    const int qrow = min(r0 + c, M - 1);
    uint4 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const uint4 *>(a.q + ((size_t)qrow * a.Hq + hq) * D + 16 * s + 8 * h);
    const int t_row = pos0 + r0 + c;  // the last key this lane's row attends

    f32x16_t oacc[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[j][i] = 0.0f;
    float m_run = ATTN_NEG, l_run = 0.0f;

    // the block in flight, in code form: piece x = threadIdx.x + j NT is (key x / CH, dims 8 (x % CH) .. + 7)
    const int G = D / a.gs, gshift = a.gs == 32 ? 2 : (a.gs == 64 ? 3 : 4);  // group of piece ch: ch >> gshift
    const size_t hrow = (size_t)g * a.cap;
    u32 kq[PCS][WPL], vq[PCS][WPL];
    u16 ksq[PCS], kbq[PCS], vsq[PCS], vbq[PCS];
    auto fetch = [&](int b) {
#pragma unroll
        for (int j = 0; j < PCS; ++j) {
            const int x = threadIdx.x + j * NT;
            if (PIECES % NT == 0 || x < PIECES) {
                const int ch = x % CH;
                const size_t row = hrow + min(b * BK + x / CH, sp.t_last);  // clamp, never branch around a load
                const u32 *kc = a.kv.kc + row * CW + ch * WPL, *vc = a.kv.vc + row * CW + ch * WPL;
                if constexpr (WPL == 2) {  // 8-bit: the piece's two code dwords as one 8-byte load (codes are 8-byte aligned, ABI)
                    const uint2 k2 = *reinterpret_cast<const uint2 *>(kc), v2 = *reinterpret_cast<const uint2 *>(vc);
                    kq[j][0] = k2.x, kq[j][1] = k2.y, vq[j][0] = v2.x, vq[j][1] = v2.y;
                } else {
                    kq[j][0] = *kc, vq[j][0] = *vc;
                }
                const size_t gi = row * G + (ch >> gshift);
                ksq[j] = a.kv.ks[gi], kbq[j] = a.kv.kb[gi], vsq[j] = a.kv.vs[gi], vbq[j] = a.kv.vb[gi];
            }
        }
    };
    // mx.dequantize of one piece, k_kv_dequant_prefix's arithmetic: T(fp32(s q) + b)
    auto dequant = [&](const u32 (&w)[WPL], u16 sc, u16 bi) {
        const float s = T::to_f32(sc), b = T::to_f32(bi);
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = fmaf(s, (float)((w[(i * BITS) >> 5] >> ((i * BITS) & 31)) & ((1u << BITS) - 1u)), 0.0f) + b;
        return make_uint4(pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3]), pack2<T>(o[4], o[5]), pack2<T>(o[6], o[7]));
    };
    const float sl2 = a.scale * ATTN_LOG2E;
    // transposed-read addressing (prefill_attn.hpp): lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p + 3
    const int grp = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;

    // one 32-key image against the wave's 32 rows, in k_prefill_attn's order; crosses (wave-uniform): the image reaches beyond the wave's
    // first row, so some key is masked for some row -- an image that does not is that kernel's arithmetic with every condition true
    auto image = [&](bool crosses, int tb) {
        // S^T = K . Q^T : rows = keys (registers), cols = query rows (lanes)
        f32x16_t sacc;
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint4 kf = *reinterpret_cast<const uint4 *>(k_lds + pa_off<D>(c, 2 * s + h));
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
                    (__attribute__((address_space(3))) v4i16_t *)(v_lds + pa_off<D>(16 * s + 4 * h + tq, ch) + 8 * (tp & 1)));
                const v4i16_t hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) v4i16_t *)(v_lds + pa_off<D>(16 * s + 8 + 4 * h + tq, ch) + 8 * (tp & 1)));
                const uint2 a0 = __builtin_bit_cast(uint2, lo4), a1 = __builtin_bit_cast(uint2, hi4);
                const uint4 vf = make_uint4(a0.x, a0.y, a1.x, a1.y);
                oacc[j] = MfmaT<T>::run(vf, bh, oacc[j]);
                oacc[j] = MfmaT<T>::run(vf, bl, oacc[j]);
            }
        }
    };

    fetch(b_begin);
    for (int b = b_begin; b < b_end; ++b) {
        __syncthreads();  // every wave is done reading the previous block's image
#pragma unroll
        for (int j = 0; j < PCS; ++j) {  // convert once, on the way into LDS
            const int x = threadIdx.x + j * NT;
            if (PIECES % NT == 0 || x < PIECES) {
                const int off = pa_off<D>(x / CH, x % CH);
                *reinterpret_cast<uint4 *>(k_lds + off) = dequant(kq[j], ksq[j], kbq[j]);
                *reinterpret_cast<uint4 *>(v_lds + off) = dequant(vq[j], vsq[j], vbq[j]);
            }
        }
        __syncthreads();
        if (b + 1 < b_end) fetch(b + 1);  // in flight under the scoring
        const int tb = b * BK;
        if (wave_on && tb <= t_wlast) image(tb + BK - 1 > t_w0, tb);  // (wave-uniform: a block behind the wave's last row is skipped)
    }
    if (!wave_on || r0 + c >= M) return;
    // the pair (lane, lane ^ 32) shares the query row and holds the two halves of the row sum
    const float l_sum = xor32_sum(l_run);
    if (a.splits == 1) {  // the partial IS the result (a row attends key 0: l > 0)
        const float inv = 1.0f / l_sum;
        u16 *orow = a.out + ((size_t)(r0 + c) * a.Hq + hq) * D;
        // k_prefill_attn's two roundings, product to fp32 then to T: the product stays in a register of its own so that no fused
        // multiply-and-convert makes them one
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
    const size_t part = ((size_t)(r0 + c) * a.Hq + hq) * a.splits + split;
#pragma unroll
    for (int j = 0; j < DT; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            *reinterpret_cast<float4 *>(a.part_acc + part * D + 32 * j + 8 * k + 4 * h) =
                make_float4(oacc[j][4 * k], oacc[j][4 * k + 1], oacc[j][4 * k + 2], oacc[j][4 * k + 3]);
    if (h == 0) a.part_ml[part * 2 + 0] = m_run, a.part_ml[part * 2 + 1] = l_sum;  // (the pair holds the same maximum)
}

// The merge: workgroup r merges the active splits of row r's tile in split order (split 0 holds key 0, which every row sees: the
// maximum is finite and the sum positive).  k_prefill_attn_paged_merge's arithmetic; its arguments are pages and chunk descriptors.
template <class T>
__global__ void __launch_bounds__(256) k_prefill_attn_q_merge(const PrefillQuantArgs a, const int D, const int BM) {
    const int r = blockIdx.x, pos0 = a.state ? a.state->pos : a.offset;
    const int active = pq_split(pos0, a.M, a.cap, r / BM * BM, BM, a.splits).active;
    const int D4 = D / 4;
    for (int o = threadIdx.x; o < a.Hq * D4; o += 256) {
        const int hq = o / D4, d = (o % D4) * 4;
        const size_t base = ((size_t)r * a.Hq + hq) * a.splits;
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
        *reinterpret_cast<uint2 *>(a.out + ((size_t)r * a.Hq + hq) * D + d) = make_uint2(pack2<T>(acc.x / l, acc.y / l), pack2<T>(acc.z / l, acc.w / l));
    }
}

// prefill_attn_launch_d's rule: 2 tiles need 2 rep <= 8 waves, and pay only while the halved grid fills the 256 CUs
bool pq_two_tiles(int M, int Hkv, int rep) {
    const int qt = pie_knob(PIE_KNOB_PREFILL_QT);  // test knob, as prefill_attn_launch_d reads it
    return rep <= 4 && M > 32 && (qt > 0 ? qt == 2 : ((M + 63) / 64) * Hkv >= 256);
}

template <class T, int D, int BITS>
int prefill_attn_quant_launch_b(const PrefillQuantArgs &a, hipStream_t st) {
    const int rep = a.Hq / a.Hkv;
    const bool two = pq_two_tiles(a.M, a.Hkv, rep);
    const int bm = two ? 64 : 32;
    const dim3 grid((unsigned)(((a.M + bm - 1) / bm) * a.splits * a.Hkv));
#define PQ_LAUNCH(R)                                                                                                                           \
    if (two && R <= 4) hipLaunchKernelGGL((k_prefill_attn_q<T, D, BITS, R, (R <= 4 ? 2 : 1)>), grid, dim3(pq_waves(R, R <= 4 ? 2 : 1) * 64), 0, st, a); \
    else hipLaunchKernelGGL((k_prefill_attn_q<T, D, BITS, R, 1>), grid, dim3(pq_waves(R, 1) * 64), 0, st, a);                                   \
    break
    switch (rep) {
        case 1: PQ_LAUNCH(1);
        case 2: PQ_LAUNCH(2);
        case 4: PQ_LAUNCH(4);
        case 8: PQ_LAUNCH(8);
        default: return pie::fail(PIE_E_SHAPE, "prefill_attn_quant: n_heads / n_kv_heads must be 1, 2, 4 or 8");
    }
#undef PQ_LAUNCH
    PIE_LAUNCH_CHECK();
    if (a.splits > 1) {
        hipLaunchKernelGGL((k_prefill_attn_q_merge<T>), dim3((unsigned)a.M), dim3(256), 0, st, a, D, bm);
        PIE_LAUNCH_CHECK();
    }
    return PIE_OK;
}

template <class T>
int prefill_attn_quant_launch_t(int D, int bits, const PrefillQuantArgs &a, hipStream_t st) {
    if (D == 128) return bits == 4 ? prefill_attn_quant_launch_b<T, 128, 4>(a, st) : prefill_attn_quant_launch_b<T, 128, 8>(a, st);
    return bits == 4 ? prefill_attn_quant_launch_b<T, 64, 4>(a, st) : prefill_attn_quant_launch_b<T, 64, 8>(a, st);
}

}  // namespace

int prefill_attn_quant_splits(int M, int offset, int Hq, int Hkv) {
    if (M < 1 || offset < 0 || Hkv < 1 || Hq < Hkv || Hq % Hkv) return 1;
    const int bm = pq_two_tiles(M, Hkv, Hq / Hkv) ? 64 : 32;
    const long wgs = (long)((M + bm - 1) / bm) * Hkv;
    const long blocks = ((long)offset + M + 31) / 32;
    long splits = wgs >= PREFILL_QUANT_TARGET_WGS ? 1 : (PREFILL_QUANT_TARGET_WGS + wgs - 1) / wgs;
    splits = splits > ATTN_MAX_SPLITS ? ATTN_MAX_SPLITS : splits;
    splits = splits > blocks / PREFILL_QUANT_MIN_SPLIT_BLOCKS ? blocks / PREFILL_QUANT_MIN_SPLIT_BLOCKS : splits;
    // the partials of the call at head_dim 128 stay inside PREFILL_QUANT_WS_CAP (one split needs none)
    const long cap = (long)(PREFILL_QUANT_WS_CAP / ((size_t)M * Hq * (128 + 2) * sizeof(float)));
    splits = splits > cap ? cap : splits;
    return splits < 1 ? 1 : (int)splits;
}

size_t prefill_attn_quant_workspace_bytes(int M, int Hq, int D, int splits) {
    if (splits <= 1 || M < 1 || Hq < 1 || D < 1) return 0;
    return (size_t)M * Hq * splits * (D + 2) * sizeof(float);
}

int prefill_attn_quant_launch(int dtype, int D, int bits, const PrefillQuantArgs &a, hipStream_t st) {
    if (a.splits < 1 || a.splits > ATTN_MAX_SPLITS || (a.splits > 1 && !(a.part_acc && a.part_ml)))
        return pie::fail(PIE_E_ARG, "prefill_attn_quant: splits must be 1..32, with partials beyond one");
    return dtype == PIE_BF16 ? prefill_attn_quant_launch_t<BF16>(D, bits, a, st) : prefill_attn_quant_launch_t<F16>(D, bits, a, st);
}

extern "C" {

int pie_prefill_attn_quant_splits(int M, int offset, int n_heads, int n_kv_heads) { return prefill_attn_quant_splits(M, offset, n_heads, n_kv_heads); }

size_t pie_prefill_attn_quant_workspace_bytes(int M, int n_heads, int head_dim, int splits) {
    return prefill_attn_quant_workspace_bytes(M, n_heads, head_dim, splits);
}

int pie_prefill_attn_quant(const void *q, const void *k_codes, const void *k_scales, const void *k_biases, const void *v_codes, const void *v_scales,
                           const void *v_biases, int n_heads, int n_kv_heads, int M, int offset, int cap, int head_dim, int group_size, int bits, float scale,
                           int dtype, int splits, void *out, void *workspace, void *stream) {
    PIE_REQUIRE(q && k_codes && k_scales && k_biases && v_codes && v_scales && v_biases && out, PIE_E_ARG, "pie_prefill_attn_quant: null pointer");
    if (int rc = kv_quant_check("pie_prefill_attn_quant", dtype, head_dim, group_size, bits)) return rc;
    PIE_REQUIRE(M >= 1 && M <= (1 << 24) && offset >= 0 && (long long)offset + M <= cap, PIE_E_SHAPE, "pie_prefill_attn_quant: need M >= 1, offset >= 0 and offset + M <= cap");
    PIE_REQUIRE(n_kv_heads >= 1 && n_heads >= n_kv_heads && n_heads % n_kv_heads == 0, PIE_E_SHAPE, "pie_prefill_attn_quant: n_heads must be a multiple of n_kv_heads");
    const int rep = n_heads / n_kv_heads;
    PIE_REQUIRE(rep == 1 || rep == 2 || rep == 4 || rep == 8, PIE_E_SHAPE, "pie_prefill_attn_quant: n_heads / n_kv_heads must be 1, 2, 4 or 8");
    PIE_REQUIRE(splits >= 0 && splits <= ATTN_MAX_SPLITS, PIE_E_ARG, "pie_prefill_attn_quant: splits must be 0 (chosen here) or 1..32");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(out, 16) && pie_aligned(workspace, 16), PIE_E_ALIGN, "pie_prefill_attn_quant: q, out and workspace need 16-byte alignment");
    PIE_REQUIRE(pie_aligned(k_codes, 8) && pie_aligned(v_codes, 8) && pie_aligned(k_scales, 2) && pie_aligned(k_biases, 2) && pie_aligned(v_scales, 2) &&
                    pie_aligned(v_biases, 2), PIE_E_ALIGN, "pie_prefill_attn_quant: codes need 8-byte alignment, scales and biases 2-byte");
    PrefillQuantArgs a = {};
    a.q = (const u16 *)q, a.out = (u16 *)out;
    a.kv = {(const u32 *)k_codes, (const u16 *)k_scales, (const u16 *)k_biases, (const u32 *)v_codes, (const u16 *)v_scales, (const u16 *)v_biases};
    a.offset = offset, a.cap = cap, a.gs = group_size, a.M = M, a.Hq = n_heads, a.Hkv = n_kv_heads, a.scale = scale;
    a.splits = splits ? splits : prefill_attn_quant_splits(M, offset, n_heads, n_kv_heads);
    PIE_REQUIRE(a.splits == 1 || workspace, PIE_E_ARG, "pie_prefill_attn_quant: more than one split needs a workspace (pie_prefill_attn_quant_workspace_bytes)");
    a.part_acc = (float *)workspace;
    a.part_ml = a.part_acc + (size_t)M * n_heads * a.splits * head_dim;
    return prefill_attn_quant_launch(dtype, head_dim, bits, a, (hipStream_t)stream);
}

}  // extern "C"
