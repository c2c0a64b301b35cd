// kv_quant.hip -- the quantized KV cache of the single-sequence decode path (QuantizedKVCache, cache/kv_cache/quantized.py).
//
// Storage per layer and kv-head, the reference's mx.quantize layout of every cached row: codes u32 [cap, D*BITS/32] (code k of a row
// in word k / (32/BITS) at bits BITS*(k % (32/BITS))), scales / biases T [cap, D/GS].  bits 4 / 8, group 32 / 64 / 128 (<= D), D 64 / 128.
//
//   k_kv_quant_rows     rows -> codes / scales / biases, bit-exact with mx.quantize (oracle A.1): from_cache, the prompt path's append
//   k_attn_decode_q     one query row over the quantized cache (quantized_scaled_dot_product_attention, models/base.py:56-89 of the
//                       reference), same split-KV geometry and partial format as k_attn_decode (attention.hpp): the decoder's o_proj
//                       prologue or k_attn_combine merges the splits.  With a staging row (decoder) the workgroup whose split holds the
//                       new position first quantizes the row the q|k|v epilogue staged, so the token attends its own quantized K / V.
//
// Rounding points of the reference that are local to one query row are kept: queries *= scale in T (the scale itself a T scalar),
// scores rounded to T.  The probabilities stay fp32 across the split merge (the reference rounds softmax's output to T before the
// value product; a one-pass split kernel never holds the final probabilities).
#include "kv_quant.hpp"

namespace {

// One lane owns 8 consecutive elements of a row (a 16-byte piece): LPT = D/8 lanes per row, groups of GS/8 lanes.  The group's
// min / max are reduced across its lanes; then the mx.quantize arithmetic with IEEE fp32 division (-ffp-contract=off).
template <int BITS>
struct QPiece {
    u32 w[BITS / 4];  // the 8 codes packed as MLX packs them (one word at 4 bits, two at 8)
    float scale, bias;  // the group's scale / bias AFTER rounding to T (what the cache holds)
};

template <class T, int BITS>
__device__ __forceinline__ QPiece<BITS> quant_piece(const float (&v)[8], int lanes_per_group) {
    constexpr float LEVELS = (float)((1 << BITS) - 1);
    float w_max = v[0], w_min = v[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        w_max = v[i] > w_max ? v[i] : w_max;
        w_min = v[i] < w_min ? v[i] : w_min;
    }
    for (int o = 1; o < lanes_per_group; o <<= 1) {  // aligned lane groups: the xor partner stays inside the group
        const float a = __shfl_xor(w_max, o, 64), b = __shfl_xor(w_min, o, 64);
        w_max = a > w_max ? a : w_max;
        w_min = b < w_min ? b : w_min;
    }
    const bool side = fabsf(w_min) > fabsf(w_max);
    float scale = fmaxf(__fdiv_rn(__fsub_rn(w_max, w_min), LEVELS), 1e-7f);
    scale = side ? scale : -scale;
    const float edge = side ? w_min : w_max;
    const float q0 = rintf(__fdiv_rn(edge, scale));
    const bool at_zero = q0 == 0.0f;
    scale = at_zero ? scale : __fdiv_rn(edge, q0);
    const float bias = at_zero ? 0.0f : edge;
    QPiece<BITS> p;
#pragma unroll
    for (int i = 0; i < BITS / 4; ++i) p.w[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float c = rintf(__fdiv_rn(__fsub_rn(v[i], bias), scale));  // the UNROUNDED fp32 scale / bias
        c = c < 0.0f ? 0.0f : (c > LEVELS ? LEVELS : c);
        p.w[(i * BITS) >> 5] |= (u32)c << ((i * BITS) & 31);
    }
    p.scale = round_T<T>(scale), p.bias = round_T<T>(bias);
    return p;
}

template <class T>
__device__ __forceinline__ void load_piece(const u16 *src, float (&v)[8]) {
    const uint4 q = *reinterpret_cast<const uint4 *>(src);
    const u32 qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) v[2 * j] = lo_f32<T>(qq[j]), v[2 * j + 1] = hi_f32<T>(qq[j]);
}

// Stores lane dc's piece of one row: codes at word dc*BITS/4, the group's scale / bias by the group's first lane.
template <class T, int BITS>
__device__ __forceinline__ void store_piece(const QPiece<BITS> &p, int dc, int gs, u32 *codes_row, u16 *scales_row, u16 *biases_row) {
    if constexpr (BITS == 4) codes_row[dc] = p.w[0];
    else *reinterpret_cast<uint2 *>(codes_row + 2 * dc) = make_uint2(p.w[0], p.w[1]);
    if ((dc * 8) % gs == 0) scales_row[dc * 8 / gs] = T::from_f32(p.scale), biases_row[dc * 8 / gs] = T::from_f32(p.bias);
}

// rows [H, n] of x [H, src_cap, D] -> codes [H, dst_cap, D*BITS/32], scales / biases [H, dst_cap, D/gs].  256 threads, 256/LPT rows.
template <class T, int D, int BITS>
__global__ void __launch_bounds__(256) k_kv_quant_rows(const u16 *x, int H, int n, int src_cap, int gs, u32 *codes, u16 *scales, u16 *biases, int dst_cap) {
    constexpr int LPT = D / 8;
    const int dc = threadIdx.x % LPT;
    const long long r = (long long)blockIdx.x * (256 / LPT) + threadIdx.x / LPT;
    const long long total = (long long)H * n;
    const long long rc = r < total ? r : total - 1;  // whole rows are idle together: their lanes' shuffles only meet each other
    const int h = (int)(rc / n), i = (int)(rc % n);
    float v[8];
    load_piece<T>(x + ((size_t)h * src_cap + i) * D + dc * 8, v);
    const QPiece<BITS> p = quant_piece<T, BITS>(v, gs / 8);
    if (r >= total) return;
    const size_t drow = (size_t)h * dst_cap + i;
    store_piece<T, BITS>(p, dc, gs, codes + drow * (D * BITS / 32), scales + drow * (D / gs), biases + drow * (D / gs));
}

}  // namespace

namespace {

constexpr int QATTN_WAVES = 4;
constexpr int QATTN_DEPTH = 4;  // row blocks in flight per wave

// One (kv-head g, split) per workgroup, REP query heads scored against each loaded row.  Lane (ts, dc) of a wave-load holds token
// ts's 8 dims dc*8 .. +7: the codes as one (4-bit) or two (8-bit) dwords plus the group's scale and bias.  Scores per lane are
// s*sum(q*c) + b*sum(q) (sum(q) of the lane's dims is fixed for the step), reduced over the row's lanes by DPP; values accumulate
// p*s*c per dim and p*b per lane, added once after the loop.
template <class T, int D, int REP, int BITS>
__global__ void __launch_bounds__(QATTN_WAVES * 64) k_attn_decode_q(const QAttnArgs a) {
    constexpr int LPT = D / 8, TPW = 64 / LPT, NSUB = QATTN_WAVES, NT = QATTN_WAVES * 64, DA = QATTN_DEPTH;
    constexpr int CW = D * BITS / 32, WPL = BITS / 4;  // code words per row / per lane
    __shared__ float s_m[REP][NSUB], s_l[REP][NSUB];
    __shared__ float s_acc[REP][NSUB][D];
    const int g = blockIdx.x, split = blockIdx.y, q0 = g * REP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ts = lane / LPT, dc = lane % LPT;
    const int Ttot = a.state ? a.state->pos + 1 : a.T;
    const int cap = a.state ? a.state->cap : a.cap;
    const int gs = a.gs, G = D / gs, gi = dc * 8 / gs;
    const AttnSplit sp = attn_split(Ttot, a.splits);
    if (split >= sp.active) {  // the neutral partial (attention.hpp: consumers read every slot)
        for (int o = threadIdx.x; o < REP * D; o += NT) {
            const int h = o / D, d = o % D;
            const size_t hq = (size_t)q0 + h;
            a.part_acc[(hq * a.splits + split) * D + d] = 0.0f;
            if (d == 0) a.part_ml[(hq * a.splits + split) * 2 + 0] = ATTN_NEG, a.part_ml[(hq * a.splits + split) * 2 + 1] = 0.0f;
        }
        return;
    }
    const int t_begin = split * sp.chunk;
    const int t_end = min(Ttot, t_begin + sp.chunk);
    const size_t hrow = (size_t)g * cap;
    const u32 *kc = a.kc + hrow * CW + dc * WPL, *vc = a.vc + hrow * CW + dc * WPL;
    const u16 *ks = a.ks + hrow * G + gi, *kb = a.kb + hrow * G + gi, *vs = a.vs + hrow * G + gi, *vb = a.vb + hrow * G + gi;

    // append: the split that holds the new position quantizes the staged K / V rows of this kv-head before anything is loaded
    if (a.stage && t_end == Ttot) {
        if (wave < 2 && ts == 0) {
            const int p = Ttot - 1;
            const u16 *src = a.stage + ((size_t)wave * a.Hkv * 64 + (size_t)g * 64 + (p & 63)) * D + dc * 8;
            float v[8];
            load_piece<T>(src, v);
            const QPiece<BITS> qp = quant_piece<T, BITS>(v, gs / 8);
            const size_t row = hrow + p;
            if (wave == 0) store_piece<T, BITS>(qp, dc, gs, const_cast<u32 *>(a.kc) + row * CW, const_cast<u16 *>(a.ks) + row * G, const_cast<u16 *>(a.kb) + row * G);
            else store_piece<T, BITS>(qp, dc, gs, const_cast<u32 *>(a.vc) + row * CW, const_cast<u16 *>(a.vs) + row * G, const_cast<u16 *>(a.vb) + row * G);
        }
        __syncthreads();  // workgroup-scope release / acquire: the other waves' loads of that row see the stores
    }

    // this wave's row blocks: block b covers tokens t_begin + (NSUB*b + wave)*TPW + [0, TPW)
    const int first = t_begin + wave * TPW;
    const int n_blk = first < t_end ? (t_end - first + NSUB * TPW - 1) / (NSUB * TPW) : 0;
    u32 kq[DA][WPL], vq[DA][WPL];
    u16 ksq[DA], kbq[DA], vsq[DA], vbq[DA];
    auto issue = [&](int d, int b) {
        int t = first + b * NSUB * TPW + ts;
        t = t < t_end ? t : t_end - 1;  // clamp, never branch around a load
        if constexpr (WPL == 2) {  // 8-bit: the lane's two code dwords as one 8-byte load (codes are 8-byte aligned, ABI)
            const uint2 k2 = *reinterpret_cast<const uint2 *>(kc + (size_t)t * CW), v2 = *reinterpret_cast<const uint2 *>(vc + (size_t)t * CW);
            kq[d][0] = k2.x, kq[d][1] = k2.y, vq[d][0] = v2.x, vq[d][1] = v2.y;
        } else {
            kq[d][0] = kc[(size_t)t * CW], vq[d][0] = vc[(size_t)t * CW];
        }
        ksq[d] = ks[(size_t)t * G], kbq[d] = kb[(size_t)t * G], vsq[d] = vs[(size_t)t * G], vbq[d] = vb[(size_t)t * G];
    };
#pragma unroll
    for (int d = 0; d < DA; ++d) issue(d, d);

    // queries *= scale (base.py:68): a T product with the scale as a T scalar
    const float scale_t = round_T<T>(a.scale);
    float qf[REP][8], qsum[REP];
#pragma unroll
    for (int h = 0; h < REP; ++h) {
        float v[8];
        load_piece<T>(a.q + (size_t)(q0 + h) * D + dc * 8, v);
        qsum[h] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[h][j] = round_T<T>(scale_t * v[j]), qsum[h] += qf[h][j];
    }
    float m[REP], l[REP], acc[REP][8], bacc[REP];
#pragma unroll
    for (int h = 0; h < REP; ++h) {
        m[h] = ATTN_NEG, l[h] = 0.0f, bacc[h] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[h][j] = 0.0f;
    }

    for (int base = 0; base < n_blk; base += DA) {
#pragma unroll
        for (int d = 0; d < DA; ++d) {
            const int b = base + d;
            if (b < n_blk) {  // wave-uniform
                const bool valid = first + b * NSUB * TPW + ts < t_end;
                float kcf[8], vcf[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    kcf[j] = (float)((kq[d][(j * BITS) >> 5] >> ((j * BITS) & 31)) & ((1u << BITS) - 1u));
                    vcf[j] = (float)((vq[d][(j * BITS) >> 5] >> ((j * BITS) & 31)) & ((1u << BITS) - 1u));
                }
                const float k_s = T::to_f32(ksq[d]), k_b = T::to_f32(kbq[d]), v_s = T::to_f32(vsq[d]), v_b = T::to_f32(vbq[d]);
                float sc[REP];
#pragma unroll
                for (int h = 0; h < REP; ++h) {
                    float dot = 0.0f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) dot = fmaf(qf[h][j], kcf[j], dot);
                    sc[h] = fmaf(k_s, dot, k_b * qsum[h]);
                }
#pragma unroll
                for (int h = 0; h < REP; ++h) sc[h] += __builtin_amdgcn_update_dpp(0.0f, sc[h], 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
#pragma unroll
                for (int h = 0; h < REP; ++h) sc[h] += __builtin_amdgcn_update_dpp(0.0f, sc[h], 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
#pragma unroll
                for (int h = 0; h < REP; ++h) sc[h] += __builtin_amdgcn_update_dpp(0.0f, sc[h], 0x141, 0xF, 0xF, true);  // row_half_mirror
                if (LPT == 16) {
#pragma unroll
                    for (int h = 0; h < REP; ++h) sc[h] += __builtin_amdgcn_update_dpp(0.0f, sc[h], 0x140, 0xF, 0xF, true);  // row_mirror
                }
                bool grow = false;
#pragma unroll
                for (int h = 0; h < REP; ++h) {
                    sc[h] = valid ? round_T<T>(sc[h]) * ATTN_LOG2E : ATTN_NEG;  // scores in T (quantized_matmul's output), then base 2
                    grow |= sc[h] > m[h];
                }
                if (grow) {
#pragma unroll
                    for (int h = 0; h < REP; ++h) {
                        const float m_new = sc[h] > m[h] ? sc[h] : m[h];
                        const float alpha = attn_exp2(m[h] - m_new);
                        l[h] *= alpha, bacc[h] *= alpha;
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[h][j] *= alpha;
                        m[h] = m_new;
                    }
                }
#pragma unroll
                for (int h = 0; h < REP; ++h) {
                    const float p = valid ? attn_exp2(sc[h] - m[h]) : 0.0f;
                    const float ps = p * v_s;
                    l[h] += p;
                    bacc[h] = fmaf(p, v_b, bacc[h]);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[h][j] = fmaf(ps, vcf[j], acc[h][j]);
                }
            }
            issue(d, b + DA);
        }
    }

    // merge the token groups of the wave (lanes with equal dc), then one stream per wave through LDS
#pragma unroll
    for (int h = 0; h < REP; ++h) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[h][j] += bacc[h];
        float mw = m[h];
        if (LPT == 8) mw = fmaxf(mw, ror8(mw));
        mw = xor32_max(xor16_max(mw));
        const float wg = attn_exp2(m[h] - mw);
        m[h] = mw;
        l[h] *= wg;
        if (LPT == 8) l[h] += ror8(l[h]);
        l[h] = xor32_sum(xor16_sum(l[h]));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc[h][j] *= wg;
            if (LPT == 8) acc[h][j] += ror8(acc[h][j]);
            acc[h][j] = xor32_sum(xor16_sum(acc[h][j]));
        }
    }
    if (ts == 0) {
#pragma unroll
        for (int h = 0; h < REP; ++h) {
            if (dc == 0) s_m[h][wave] = m[h], s_l[h][wave] = l[h];
#pragma unroll
            for (int j = 0; j < 8; ++j) s_acc[h][wave][dc * 8 + j] = acc[h][j];
        }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < REP * D; o += NT) {
        const int h = o / D, d = o % D;
        float M = ATTN_NEG;
#pragma unroll
        for (int i = 0; i < NSUB; ++i) M = fmaxf(M, s_m[h][i]);
        float Lsum = 0.0f, A = 0.0f;
#pragma unroll
        for (int i = 0; i < NSUB; ++i) {
            const float w = attn_exp2(s_m[h][i] - M);
            Lsum = fmaf(w, s_l[h][i], Lsum);
            A = fmaf(w, s_acc[h][i][d], A);
        }
        const size_t hq = (size_t)q0 + h;
        a.part_acc[(hq * a.splits + split) * D + d] = A;
        if (d == 0) a.part_ml[(hq * a.splits + split) * 2 + 0] = M, a.part_ml[(hq * a.splits + split) * 2 + 1] = Lsum;
    }
}

template <class T, int D, int BITS>
int attn_q_rep(int rep, const QAttnArgs &a, hipStream_t st) {
    const dim3 grid(a.Hkv, a.splits), block(QATTN_WAVES * 64);
    switch (rep) {
        case 1: hipLaunchKernelGGL((k_attn_decode_q<T, D, 1, BITS>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_attn_decode_q<T, D, 2, BITS>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((k_attn_decode_q<T, D, 4, BITS>), grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL((k_attn_decode_q<T, D, 8, BITS>), grid, block, 0, st, a); break;
        default: return pie::fail(PIE_E_SHAPE, "attn_decode_quant: Hq / Hkv must be 1, 2, 4 or 8");
    }
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

template <class T>
int attn_q_dispatch(int D, int bits, int rep, const QAttnArgs &a, hipStream_t st) {
    if (D == 128) return bits == 4 ? attn_q_rep<T, 128, 4>(rep, a, st) : attn_q_rep<T, 128, 8>(rep, a, st);
    return bits == 4 ? attn_q_rep<T, 64, 4>(rep, a, st) : attn_q_rep<T, 64, 8>(rep, a, st);
}

template <class T>
int quant_rows_dispatch(int D, int bits, const u16 *x, int H, int n, int src_cap, int gs, u32 *codes, u16 *scales, u16 *biases, int dst_cap, hipStream_t st) {
    const long long rows = (long long)H * n;
    const int per_block = 256 / (D / 8);
    const dim3 grid((unsigned)((rows + per_block - 1) / per_block)), block(256);
    if (D == 128 && bits == 4) hipLaunchKernelGGL((k_kv_quant_rows<T, 128, 4>), grid, block, 0, st, x, H, n, src_cap, gs, codes, scales, biases, dst_cap);
    else if (D == 128) hipLaunchKernelGGL((k_kv_quant_rows<T, 128, 8>), grid, block, 0, st, x, H, n, src_cap, gs, codes, scales, biases, dst_cap);
    else if (bits == 4) hipLaunchKernelGGL((k_kv_quant_rows<T, 64, 4>), grid, block, 0, st, x, H, n, src_cap, gs, codes, scales, biases, dst_cap);
    else hipLaunchKernelGGL((k_kv_quant_rows<T, 64, 8>), grid, block, 0, st, x, H, n, src_cap, gs, codes, scales, biases, dst_cap);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

}  // namespace

// The formats this path takes; anything else is refused before a launch.
int kv_quant_check(const char *who, int dtype, int D, int group_size, int bits) {
    if (dtype != PIE_BF16 && dtype != PIE_F16) return pie::fail(PIE_E_ARG, std::string(who) + ": dtype must be bf16 or f16");
    if (bits != 4 && bits != 8) return pie::fail(PIE_E_ARG, std::string(who) + ": bits must be 4 or 8");
    if (group_size != 32 && group_size != 64 && group_size != 128) return pie::fail(PIE_E_ARG, std::string(who) + ": group_size must be 32, 64 or 128");
    if (D != 64 && D != 128) return pie::fail(PIE_E_SHAPE, std::string(who) + ": head_dim must be 64 or 128");
    if (D % group_size) return pie::fail(PIE_E_SHAPE, std::string(who) + ": group_size must divide head_dim");
    return PIE_OK;
}

int kv_quant_rows_launch(int dtype, const void *x, int H, int n, int src_cap, int D, int gs, int bits, void *codes, void *scales, void *biases, int dst_cap,
                         hipStream_t st) {
    if (dtype == PIE_BF16) return quant_rows_dispatch<BF16>(D, bits, (const u16 *)x, H, n, src_cap, gs, (u32 *)codes, (u16 *)scales, (u16 *)biases, dst_cap, st);
    return quant_rows_dispatch<F16>(D, bits, (const u16 *)x, H, n, src_cap, gs, (u32 *)codes, (u16 *)scales, (u16 *)biases, dst_cap, st);
}

int attn_decode_quant_launch(int dtype, int D, int bits, const QAttnArgs &a, bool combine, u16 *out, hipStream_t st) {
    PIE_REQUIRE(a.Hkv > 0 && a.Hq % a.Hkv == 0, PIE_E_SHAPE, "attn_decode_quant: Hq must be a multiple of Hkv");
    PIE_REQUIRE(a.splits >= 1 && a.splits <= ATTN_MAX_SPLITS, PIE_E_ARG, "attn_decode_quant: bad split count");
    const int rep = a.Hq / a.Hkv;
    const int rc = dtype == PIE_BF16 ? attn_q_dispatch<BF16>(D, bits, rep, a, st) : attn_q_dispatch<F16>(D, bits, rep, a, st);
    if (rc || !combine) return rc;
    AttnArgs c = {};
    c.state = a.state, c.T = a.T, c.Hq = a.Hq, c.Hkv = a.Hkv, c.splits = a.splits;
    c.part_acc = a.part_acc, c.part_ml = a.part_ml, c.out = out;
    if (dtype == PIE_BF16) hipLaunchKernelGGL(k_attn_combine<BF16>, dim3(a.Hq, 1), dim3(256), 0, st, c, D);
    else hipLaunchKernelGGL(k_attn_combine<F16>, dim3(a.Hq, 1), dim3(256), 0, st, c, D);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// ---------------------------------------------------------------- prompt path (prefill.hip): dequantise-to-T scratch
// The batched prompt pass reads and writes T rows through the decoder's pointer table; on a quantized cache that table points every layer at
// one T scratch [Hkv, cap, D] for K and one for V.  Per layer: k_kv_dequant_prefix fills rows [0, pos) from the codes (mx.dequantize:
// T(s*q + b)), the pass appends the chunk's T rows at [pos, pos + M), k_kv_requant_chunk quantizes those into the codes and writes their
// dequantized values back, so the chunk's own attention sees its quantized K / V as in update_and_fetch (quantized.py:91-103).
namespace {
template <class T, int D, int BITS>
__global__ void __launch_bounds__(256) k_kv_dequant_prefix(QKvLayer lay, const DecState *state, int Hkv, int cap, int gs, u16 *sk, u16 *sv) {
    constexpr int LPT = D / 8, CW = D * BITS / 32, WPL = BITS / 4;
    const long long r = (long long)blockIdx.x * (256 / LPT) + threadIdx.x / LPT;
    const int dc = threadIdx.x % LPT, pos = state->pos;
    if (r >= (long long)Hkv * cap || (int)(r % cap) >= pos) return;
    const bool v = blockIdx.y == 1;
    const u32 *codes = v ? lay.vc : lay.kc;
    const u16 *sc = v ? lay.vs : lay.ks, *bi = v ? lay.vb : lay.kb;
    const int G = D / gs, gi = dc * 8 / gs;
    u32 w[WPL];
#pragma unroll
    for (int i = 0; i < WPL; ++i) w[i] = codes[(size_t)r * CW + dc * WPL + i];
    const float s = T::to_f32(sc[(size_t)r * G + gi]), b = T::to_f32(bi[(size_t)r * G + gi]);
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = fmaf(s, (float)((w[(j * BITS) >> 5] >> ((j * BITS) & 31)) & ((1u << BITS) - 1u)), 0.0f) + b;
    *reinterpret_cast<uint4 *>((v ? sv : sk) + (size_t)r * D + dc * 8) =
        make_uint4(pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3]), pack2<T>(o[4], o[5]), pack2<T>(o[6], o[7]));
}

template <class T, int D, int BITS>
__global__ void __launch_bounds__(256) k_kv_requant_chunk(QKvLayer lay, const DecState *state, int Hkv, int cap, int M, int gs, u16 *sk, u16 *sv) {
    constexpr int LPT = D / 8, CW = D * BITS / 32;
    const long long r = (long long)blockIdx.x * (256 / LPT) + threadIdx.x / LPT;
    const long long total = (long long)Hkv * M;
    const long long rc = r < total ? r : total - 1;  // whole rows idle together (quant_piece's shuffles stay inside a row)
    const int dc = threadIdx.x % LPT;
    const bool v = blockIdx.y == 1;
    const size_t row = (size_t)(rc / M) * cap + state->pos + (int)(rc % M);
    u16 *src = (v ? sv : sk) + row * D + dc * 8;
    float x[8];
    load_piece<T>(src, x);
    const QPiece<BITS> p = quant_piece<T, BITS>(x, gs / 8);
    if (r >= total) return;
    const int G = D / gs;
    store_piece<T, BITS>(p, dc, gs, const_cast<u32 *>(v ? lay.vc : lay.kc) + row * CW, const_cast<u16 *>(v ? lay.vs : lay.ks) + row * G,
                         const_cast<u16 *>(v ? lay.vb : lay.kb) + row * G);
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = fmaf(p.scale, (float)((p.w[(j * BITS) >> 5] >> ((j * BITS) & 31)) & ((1u << BITS) - 1u)), 0.0f) + p.bias;
    *reinterpret_cast<uint4 *>(src) = make_uint4(pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3]), pack2<T>(o[4], o[5]), pack2<T>(o[6], o[7]));
}

template <class T, int D, int BITS>
int prefill_quant_t(bool dequant, const QKvLayer &lay, const DecState *state, int Hkv, int cap, int M, int gs, u16 *sk, u16 *sv, hipStream_t st) {
    const long long rows = dequant ? (long long)Hkv * cap : (long long)Hkv * M;
    const int per_block = 256 / (D / 8);
    const dim3 grid((unsigned)((rows + per_block - 1) / per_block), 2), block(256);
    if (dequant) hipLaunchKernelGGL((k_kv_dequant_prefix<T, D, BITS>), grid, block, 0, st, lay, state, Hkv, cap, gs, sk, sv);
    else hipLaunchKernelGGL((k_kv_requant_chunk<T, D, BITS>), grid, block, 0, st, lay, state, Hkv, cap, M, gs, sk, sv);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}
}  // namespace

int kv_quant_prefill_launch(int dtype, int D, int bits, bool dequant, const QKvLayer &lay, const DecState *state, int Hkv, int cap, int M, int gs,
                            u16 *sk, u16 *sv, hipStream_t st) {
    if (dtype == PIE_BF16) {
        if (D == 128) return bits == 4 ? prefill_quant_t<BF16, 128, 4>(dequant, lay, state, Hkv, cap, M, gs, sk, sv, st) : prefill_quant_t<BF16, 128, 8>(dequant, lay, state, Hkv, cap, M, gs, sk, sv, st);
        return bits == 4 ? prefill_quant_t<BF16, 64, 4>(dequant, lay, state, Hkv, cap, M, gs, sk, sv, st) : prefill_quant_t<BF16, 64, 8>(dequant, lay, state, Hkv, cap, M, gs, sk, sv, st);
    }
    if (D == 128) return bits == 4 ? prefill_quant_t<F16, 128, 4>(dequant, lay, state, Hkv, cap, M, gs, sk, sv, st) : prefill_quant_t<F16, 128, 8>(dequant, lay, state, Hkv, cap, M, gs, sk, sv, st);
    return bits == 4 ? prefill_quant_t<F16, 64, 4>(dequant, lay, state, Hkv, cap, M, gs, sk, sv, st) : prefill_quant_t<F16, 64, 8>(dequant, lay, state, Hkv, cap, M, gs, sk, sv, st);
}

// ---------------------------------------------------------------- C ABI (op level)
int pie_kv_quantize(const void *x, int H, int n, int src_cap, int D, int group_size, int bits, int dtype, void *codes, void *scales, void *biases,
                    int dst_cap, void *stream) {
    PIE_REQUIRE(x && codes && scales && biases, PIE_E_ARG, "pie_kv_quantize: null pointer");
    if (int rc = kv_quant_check("pie_kv_quantize", dtype, D, group_size, bits)) return rc;
    PIE_REQUIRE(H >= 1 && n >= 0 && n <= src_cap && n <= dst_cap, PIE_E_SHAPE, "pie_kv_quantize: need H >= 1 and 0 <= n <= src_cap, dst_cap");
    PIE_REQUIRE(pie_aligned(x, 16) && pie_aligned(codes, 8) && pie_aligned(scales, 2) && pie_aligned(biases, 2), PIE_E_ALIGN,
                "pie_kv_quantize: x must be 16-byte aligned, codes 8-byte");
    if (n == 0) return PIE_OK;
    return kv_quant_rows_launch(dtype, x, H, n, src_cap, D, group_size, bits, codes, scales, biases, dst_cap, (hipStream_t)stream);
}

int pie_attn_decode_quant(const void *q, const void *k_codes, const void *k_scales, const void *k_biases, const void *v_codes, const void *v_scales,
                          const void *v_biases, int Hq, int Hkv, int T, int cap, int D, int group_size, int bits, float scale, int dtype, void *out,
                          void *workspace, void *stream) {
    PIE_REQUIRE(q && k_codes && k_scales && k_biases && v_codes && v_scales && v_biases && out && workspace, PIE_E_ARG, "pie_attn_decode_quant: null pointer");
    if (int rc = kv_quant_check("pie_attn_decode_quant", dtype, D, group_size, bits)) return rc;
    PIE_REQUIRE(Hkv >= 1 && Hq >= Hkv && Hq % Hkv == 0, PIE_E_SHAPE, "pie_attn_decode_quant: Hq must be a multiple of Hkv");
    const int rep = Hq / Hkv;
    PIE_REQUIRE(rep == 1 || rep == 2 || rep == 4 || rep == 8, PIE_E_SHAPE, "pie_attn_decode_quant: Hq / Hkv must be 1, 2, 4 or 8");
    PIE_REQUIRE(T >= 1 && T <= cap, PIE_E_SHAPE, "pie_attn_decode_quant: need 1 <= T <= cap");
    PIE_REQUIRE(pie_aligned(q, 16) && pie_aligned(k_codes, 8) && pie_aligned(v_codes, 8), PIE_E_ALIGN, "pie_attn_decode_quant: q 16-byte, codes 8-byte alignment required");
    QAttnArgs a = {};
    a.q = (const u16 *)q, a.kc = (const u32 *)k_codes, a.vc = (const u32 *)v_codes;
    a.ks = (const u16 *)k_scales, a.kb = (const u16 *)k_biases, a.vs = (const u16 *)v_scales, a.vb = (const u16 *)v_biases;
    a.T = T, a.cap = cap, a.gs = group_size, a.Hq = Hq, a.Hkv = Hkv, a.scale = scale;
    a.splits = T >= 2048 ? ATTN_MAX_SPLITS : (T >= 512 ? 16 : (T >= 128 ? 4 : 1));  // pie_sdpa_decode's plan
    a.part_acc = (float *)workspace;
    a.part_ml = a.part_acc + (size_t)Hq * ATTN_MAX_SPLITS * D;
    return attn_decode_quant_launch(dtype, D, bits, a, true, (u16 *)out, (hipStream_t)stream);
}
