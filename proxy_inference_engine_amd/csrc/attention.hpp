// attention.hpp -- split-KV decode attention (L = 1) over the ReusableKVCache buffers.
//
// Replaces mx.fast.scaled_dot_product_attention(q, k, v, scale, mask=None) at models/base.py:111-113
// (<- models/llama/language.py:98-105) for the decode step.  HBM-bound KV read; K/V rows go straight to
// VGPRs in 16-byte pieces (a wave-load covers 64/LPT whole rows, coalesced) through a register ring that keeps
// ATTN_DEPTH row-blocks in flight per wave; every q-head of the GQA group is scored against the same loaded K/V
// so the cache is read once; online softmax in fp32 per lane-group, merged in-wave by shuffles and across the
// 4 waves through LDS; one partial (m, l, acc[D]) per (q-head, split).  The partials are merged either by
// k_attn_combine (op-level API) or by the o_proj GEMV's staging prologue (decoder), fp32 until the single
// rounding at the end = MLX fused-kernel contract.
#pragma once
#include <type_traits>
#include "common.hpp"

constexpr int ATTN_MAX_SPLITS = 32;  // 8 kv-heads x 32 splits = one workgroup per CU
constexpr int ATTN_DEPTH = 4;  // swept 4 vs 8 with 8-wave workgroups: 8 is 2-3 % slower at every context (VALU-bound, not latency-bound)
constexpr float ATTN_NEG = -3.0e38f;
// Softmax runs in the base-2 domain: scores are scaled by scale*log2(e) once and every exponential is one v_exp_f32
// (expf() expands to ~9 VALU instructions for range handling the scores never need; the loop is VALU-bound at long
// context).  Running maxima m (and the m of the split partials) are therefore log2-domain values; l and acc are the
// same linear-domain sums either way.
constexpr float ATTN_LOG2E = 1.4426950408889634f;
__device__ __forceinline__ float attn_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// Device-resident decode state: lets one captured graph serve every step.
struct DecState {
    int pos;    // cache.offset before the step (reusable.py:111)
    int token;  // input token of the step / greedy output after it
    int cap;    // capacity of the per-layer KV buffers (tokens)
    int pad;
    // RotatingKVCache (pie_decoder_set_kv_ring): window = max_size (0 = unbounded: every other cache), keep = sink rows, rot0 = the
    // position written at row `keep` when the ring last started rotating.  Position p >= rot0 lives in row keep + (p - rot0) % (window - keep),
    // earlier ones in row p; a step attends min(pos + 1, window) rows.  All from pos: the ring fills up inside replayed graphs.
    int window, keep, rot0, pad2;
};
__host__ __device__ __forceinline__ int ring_slot(const DecState &s, int p) { return p < s.rot0 ? p : s.keep + (p - s.rot0) % (s.window - s.keep); }
__host__ __device__ __forceinline__ int ring_len(const DecState &s) { return s.window > 0 && s.pos + 1 > s.window ? s.window : s.pos + 1; }

// How T cached positions are cut into splits: fixed launch geometry (graph-replayable), data-dependent activity.
struct AttnSplit {
    int chunk, active;
};
static inline __host__ __device__ AttnSplit attn_split(int T, int splits) {
    AttnSplit s;
    int chunk = (T + splits - 1) / splits;
    chunk = chunk < 32 ? 32 : chunk;  // never less than two row-blocks per wave: short contexts use fewer splits
    s.chunk = chunk;
    s.active = (T + chunk - 1) / chunk;
    return s;
}

struct AttnArgs {
    const u16 *q;         // [Hq, D]
    const u16 *k, *v;     // [Hkv, cap, D] (op-level) ...
    const unsigned long long *kv_table;  // ... or the decoder's pointer table (k == nullptr)
    int layer, n_layers;
    const DecState *state;  // nullable: T = state->pos + 1, cap = state->cap
    int T, cap;
    int Hq, Hkv, splits;
    int nt_kv;            // non-temporal K/V loads (long-context plan)
    int rows;             // prefill: query rows (blockIdx.z); row r attends T + r positions (causal inside the chunk); 0 = 1
    float scale;
    float *part_acc;  // [Hq, splits, D]
    float *part_ml;   // [Hq, splits, 2]
    u16 *out;         // [Hq, D]
    // Paged KV (PAGED instantiation, block_table != nullptr): token t of row / sequence r lives in page
    // block_table[r * bt_stride + t / 64] at row t % 64.  Page layout: K block then V block, each [Hkv, 64, D] (one kv-head's
    // 64 rows contiguous: 16 KB bursts at D = 128).  Op level: `slab` = the layer's slab, blockIdx.z = sequence, sequence s
    // attends ctx_len[s] positions (0 = idle slot).  Decoder: slab == nullptr, kv_table holds the layers' K / V slab bases,
    // T from `state` as in the contiguous case, bt_stride = 0 (one sequence).
    const u16 *slab;
    const int *block_table, *ctx_len;
    int bt_stride, n_pages;
    unsigned *prof;   // developer build (-DPIE_ATTN_PROF): stamps of workgroup (0, 0, 0), words 2..9 of the decoder's scratch; nullptr otherwise
    // Infinity-Cache warm-up riding on the CUs this launch leaves idle (decoder only): workgroups with blockIdx.y >= splits stream o_proj's
    // weights with plain coalesced loads and discard them, so that launch's 9.4 MB then come from the cache.  Re-decided in round 4
    // ("x 18.7 attention traffic for 0.3 %"): same box, three alternating repetitions -- with it 1.198-1.201 ms per 8B step,
    // without it 1.211-1.217 (+1.3 %), with an XCD-matched one-dword-per-line L2 touch instead 1.222-1.245.  The bytes leave HBM once either
    // way (FETCH_SIZE counts Infinity-Cache hits: o_proj's own fetch is then served on-die); what moves is WHEN they leave it.
    const char *pf_ptr;
    unsigned long long pf_bytes;
    int pf_rows;      // extra blockIdx.y rows doing this (0 = none)
    unsigned *pf_sink;
    // RotatingKVCache (RING instantiation, decoder only): the q|k|v launch staged the step's K / V rows in this page (K block then V block,
    // each [Hkv, 64, D], row pos % 64); the split that holds the row's ring slot moves them there and scores them from the page
    const u16 *ring_stage;
};

constexpr int ATTN_WAVES = 8;  // waves per workgroup (2 per SIMD: one wave's VALU scoring overlaps the other's loads)
// Short caches (the merged-split plan, capacity <= 1024) run 4 waves: a split then holds a few dozen positions, the scoring loop is two or
// three row blocks per wave either way, and half the waves mean half the streams in the closing merge and less barrier skew: 1.250 vs
// 1.263 ms per step at T ~ 200 (16 waves: 1.334).  Long caches keep 8 (the scoring loop is VALU work there).
// ... with up to 4 q-heads per kv-head; with 8 (the 70B geometry) a wave carries twice the heads and the 8-wave form stays ahead
// (70B step: 7.95-8.13 vs 8.27-8.44 ms)
constexpr int attn_short_waves(int rep) { return rep <= 4 ? 4 : ATTN_WAVES; }

// 16-byte K/V row piece.  NT = non-temporal (the cache is read once per step): measured on the 8B decode step with nt weight
// streams, nt K/V is -0.6 % at 200 cached positions (the rows then survive in the Infinity Cache from step to step), +2.1 % at
// 2000, +3.4 % at 8000, +3.5 % at 32000 -- the launcher turns it on with the long-context plan.
template <bool NT>
__device__ __forceinline__ uint4 attn_load_row(const u16 *p) {
    if constexpr (NT) {
        typedef unsigned nt_u32x4 __attribute__((ext_vector_type(4)));
        const nt_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_u32x4 *>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    } else {
        return *reinterpret_cast<const uint4 *>(p);
    }
}

#ifdef PIE_ATTN_PROF  // developer build: s_memrealtime stamps (100 MHz) of workgroup (0, 0, 0), read by tools/step_bench
// stamps go to the decoder's stamp scratch, words 2..9 (pie_debug_buffer(d, 7) hands it out)
#define ATTN_STAMP(i) if (a.prof && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) reinterpret_cast<unsigned long long *>(a.prof)[2 + (i)] = __builtin_amdgcn_s_memrealtime()
#else
#define ATTN_STAMP(i)
#endif

// The workgroup's work for (kv-head group g, split, query row): the body of k_attn_decode, also called by the q|k|v GEMV behind its XCD-local
// seam (w4_gemv.hpp, FUSE: a workgroup of 8 waves of which the first WAVES run this -- the others only join the barrier).
// SEAM: a callable run once, after the first K / V rows of the split are in flight and before anything this step's q|k|v launch wrote is read
// (the fused caller waits for its kv-group there: the old rows' latency hides under the wait); nullptr_t = none.
struct AttnNoSeam {
    __device__ __forceinline__ void operator()() const {}
};
// q0: the first of the REP query heads scored here (the kernel: g * REP, all heads of the kv group; the fused caller: ONE head of group g per
// workgroup -- a head's online softmax never looks at another head, so the grouping does not change a bit).
template <class T, int D, int REP, bool PAGED, bool NTKV, int WAVES, class SEAM = AttnNoSeam, bool RING = false>
__device__ __forceinline__ void attn_decode_body(const AttnArgs &a, const int g, const int split, const int row, const int q0, const SEAM seam = SEAM()) {
    constexpr int LPT = D / 8;     // lanes per token row (16 B each)
    constexpr int TPW = 64 / LPT;  // token rows per wave-load
    constexpr int NSUB = WAVES;  // one merged online-softmax stream per wave reaches LDS
    constexpr int NT = WAVES * 64;
    constexpr int DA = ATTN_DEPTH;
    // WIDE: every 16-lane token group of every wave publishes its own online-softmax stream and the final pass merges all of them -- the
    // permlane merge of a wave's groups (4 heads x 8 accumulators x 2 swap steps, ~1 us measured in a 4.8 us workgroup at T = 190) goes
    // away for the price of a longer final pass.  Where the streams fit 64 KB of LDS (REP 4, D 128: the 8B / 70B geometry).
#ifndef PIE_ATTN_WIDE
#define PIE_ATTN_WIDE 1
#endif
    constexpr bool WIDE = PIE_ATTN_WIDE && (size_t)REP * WAVES * TPW * D * 4 <= 65536;
    constexpr int NSTR = WIDE ? WAVES * TPW : NSUB;  // streams in LDS
    __shared__ float s_m[REP][NSTR], s_l[REP][NSTR];
    __shared__ float s_acc[REP][NSTR][D];

    const bool on = (int)threadIdx.x < NT;  // (a fused caller's extra waves: no loads, no streams, only the barrier)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ts = lane / LPT, dc = lane % LPT;
    const float sl2 = a.scale * ATTN_LOG2E;
    const int Ttot = RING ? ring_len(*a.state) : PAGED && a.ctx_len ? a.ctx_len[row] : (a.state ? a.state->pos + 1 : a.T) + row;
    const int cap = PAGED ? 64 : a.state ? a.state->cap : a.cap;
    const AttnSplit sp = attn_split(Ttot, a.splits);
    const int rslot = RING ? ring_slot(*a.state, a.state->pos) : -1;  // RING: the row the step's K / V go to (every other row is read as cached)
    ATTN_STAMP(1);  // the position has arrived
    if constexpr (PAGED) {
        if (a.splits == 1 && a.ctx_len && sp.active == 0) {  // idle slot of a one-split batch: zeros, as k_attn_combine leaves it
            for (int o = threadIdx.x; o < REP * D; o += NT) a.out[((size_t)row * a.Hq + q0) * D + o] = 0;
            return;
        }
    }
    if (split >= sp.active) {  // uniform for the workgroup
        // an idle split leaves the NEUTRAL partial (max = ATTN_NEG, sum = 0, accumulator = 0: weight exp2(ATTN_NEG - M) = 0 in every merge),
        // so that the consumer that merges in its prologue (o_proj, w4_gemv.hpp) can read all `splits` slots without first loading the
        // position to learn how many are active: one dependent load less at the head of that launch.  k_attn_combine still masks by count.
        if (!(PAGED && a.splits == 1))
            for (int o = threadIdx.x; o < REP * (D / 2); o += NT) {
                const int h = o / (D / 2), d = (o % (D / 2)) * 2;
                const size_t hq = (size_t)row * a.Hq + q0 + h;
                *reinterpret_cast<float2 *>(a.part_acc + (hq * a.splits + split) * D + d) = make_float2(0.0f, 0.0f);
                if (d == 0) a.part_ml[(hq * a.splits + split) * 2 + 0] = ATTN_NEG, a.part_ml[(hq * a.splits + split) * 2 + 1] = 0.0f;
            }
        return;
    }
    const int t_begin = split * sp.chunk;
    const int t_end = min(Ttot, t_begin + sp.chunk);

    const u16 *kbase = PAGED && a.slab ? a.slab : a.k ? a.k : reinterpret_cast<const u16 *>(a.kv_table[a.layer]);
    const u16 *vbase = PAGED && a.slab ? a.slab + (size_t)a.Hkv * 64 * D : a.k ? a.v : reinterpret_cast<const u16 *>(a.kv_table[a.n_layers + a.layer]);
    kbase += (size_t)g * cap * D + dc * 8;
    vbase += (size_t)g * cap * D + dc * 8;
    const u16 *kst = nullptr, *vst = nullptr;  // RING: the staged rows of this kv-head
    if constexpr (RING) {
        kst = a.ring_stage + ((size_t)g * 64 + (a.state->pos & 63)) * D + dc * 8;
        vst = kst + (size_t)a.Hkv * 64 * D;
        if (rslot >= t_begin && rslot < t_end && threadIdx.x < (unsigned)LPT) {  // the slot's one reader moves the rows; it scores them from the page
            const size_t o = (size_t)rslot * D;
            *reinterpret_cast<uint4 *>(const_cast<u16 *>(kbase) + o) = *reinterpret_cast<const uint4 *>(kst);
            *reinterpret_cast<uint4 *>(const_cast<u16 *>(vbase) + o) = *reinterpret_cast<const uint4 *>(vst);
        }
    }
    const int *bt = PAGED ? a.block_table + (size_t)row * a.bt_stride : nullptr;
    const size_t page_elems = (size_t)2 * 64 * a.Hkv * D;
    const unsigned last_page = (unsigned)a.n_pages - 1u;

    // row-blocks of this wave: block b covers tokens t_begin + (NSUB*b + wave)*TPW + [0, TPW)
    const int first = t_begin + wave * TPW;
    const int n_blk = on && first < t_end ? (t_end - first + NSUB * TPW - 1) / (NSUB * TPW) : 0;
    uint4 kq[DA], vq[DA];
    unsigned pgq[DA];  // PAGED: page id of the block ring slot d loads next, fetched one ring turn ahead of its use
    auto page_of = [&](int b) {
        int t = first + b * NSUB * TPW + ts;
        t = t < t_end ? t : t_end - 1;
        return min((unsigned)bt[t >> 6], last_page);  // a corrupt table must not become a wild address
    };
    constexpr bool HAS_SEAM = !std::is_same<SEAM, AttnNoSeam>::value;
    bool before_seam = HAS_SEAM;  // (compile-time false without a seam)
    auto issue = [&](int d, int b) {
        int t = first + b * NSUB * TPW + ts;
        t = t < t_end ? t : t_end - 1;  // clamp, never branch around a load
        // Before the seam NO lane may touch the row this launch writes (position Ttot - 1) -- not even a clamped, discarded load: it would park a
        // stale line of that row in this CU's L1, and the real load after the seam would hit it.  Such lanes read the row before it (an empty
        // cache: the buffer's last row); the one valid lane is loaded again behind the seam.
        // (PAGED: the page id stays the clamped row's -- any row of any of the sequence's pages will do, as long as it is not row (Ttot - 1) % 64 of its page)
        if (HAS_SEAM && before_seam && t >= Ttot - 1) t = Ttot >= 2 ? Ttot - 2 : cap - 1;
        if constexpr (PAGED) {
            const size_t off = (size_t)pgq[d] * page_elems + (size_t)(t & 63) * D;
            kq[d] = attn_load_row<NTKV>(kbase + off);
            vq[d] = attn_load_row<NTKV>(vbase + off);
            pgq[d] = page_of(b + DA);
        } else if constexpr (RING) {
            const bool st = t == rslot;
            kq[d] = attn_load_row<NTKV>(st ? kst : kbase + (size_t)t * D);
            vq[d] = attn_load_row<NTKV>(st ? vst : vbase + (size_t)t * D);
        } else {
            kq[d] = attn_load_row<NTKV>(kbase + (size_t)t * D);
            vq[d] = attn_load_row<NTKV>(vbase + (size_t)t * D);
        }
    };
    if constexpr (PAGED) {
#pragma unroll
        for (int d = 0; d < DA; ++d) pgq[d] = page_of(d);
    }
#pragma unroll
    for (int d = 0; d < DA; ++d) issue(d, d);
    if constexpr (HAS_SEAM) {
        // the rows cached by earlier steps are on their way; now wait for this step's q / k / v, then fetch the one row of the ring that was
        // written in this launch (position Ttot - 1, if this split holds it and it sits in the first DA blocks)
        seam();
        before_seam = false;
        ATTN_STAMP(7);  // released
#pragma unroll
        for (int d = 0; d < DA; ++d) {
            const int t = first + d * NSUB * TPW + ts;
            if (on && t == Ttot - 1 && t < t_end) {
                if constexpr (PAGED) {
                    const size_t off = (size_t)page_of(d) * page_elems + (size_t)(t & 63) * D;
                    kq[d] = attn_load_row<NTKV>(kbase + off), vq[d] = attn_load_row<NTKV>(vbase + off);
                } else {
                    kq[d] = attn_load_row<NTKV>(kbase + (size_t)t * D), vq[d] = attn_load_row<NTKV>(vbase + (size_t)t * D);
                }
            }
        }
    }

    u32 qr[REP][4];
#pragma unroll
    for (int h = 0; h < REP; ++h) {
        uint4 qv = *reinterpret_cast<const uint4 *>(a.q + ((size_t)row * a.Hq + q0 + h) * D + dc * 8);
        qr[h][0] = qv.x, qr[h][1] = qv.y, qr[h][2] = qv.z, qr[h][3] = qv.w;
    }
    float m[REP], l[REP], acc[REP][8];
#pragma unroll
    for (int h = 0; h < REP; ++h) {
        m[h] = ATTN_NEG, l[h] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[h][j] = 0.0f;
    }

#ifdef PIE_ATTN_PROF
    if (kq[0].x == 0x12345678u && vq[0].x == 0x9abcdef0u && a.prof) a.prof[1] = 1;  // forces a wait for the first K / V rows: stamp 2 = they have landed
    ATTN_STAMP(2);
#endif
    // Reductions: DPP inside a 16-lane row; v_permlane{16,32}_swap across rows only in the post-loop merge -- no LDS traffic.
    for (int base = 0; base < n_blk; base += DA) {
#pragma unroll
        for (int d = 0; d < DA; ++d) {
            const int b = base + d;
            if (b < n_blk) {  // wave-uniform; every block has at least one valid token (ts == 0)
                // Long caches (8 waves, two per SIMD): the two waves of a SIMD take turns at the higher issue priority, two row blocks each --
                // the GEMV's finding (w4_gemv.hpp) carries over where the scoring loop is long: 8B step at 32k cached positions 1.998 ->
                // 1.945-1.956 ms, at 8k 1.527 -> 1.516, at 2k unchanged; turns of one or four blocks measured no gain.
                if constexpr (WAVES == 8 && NTKV) {
                    if (((b >> 1) + (wave >> 2)) & 1) __builtin_amdgcn_s_setprio(1);
                    else __builtin_amdgcn_s_setprio(0);
                }
                const bool valid = first + b * NSUB * TPW + ts < t_end;
                const u32 kw[4] = {kq[d].x, kq[d].y, kq[d].z, kq[d].w};
                float vf[8];
                vf[0] = lo_f32<T>(vq[d].x), vf[1] = hi_f32<T>(vq[d].x), vf[2] = lo_f32<T>(vq[d].y), vf[3] = hi_f32<T>(vq[d].y);
                vf[4] = lo_f32<T>(vq[d].z), vf[5] = hi_f32<T>(vq[d].z), vf[6] = lo_f32<T>(vq[d].w), vf[7] = hi_f32<T>(vq[d].w);
                // Scores of all heads first, the DPP reduction steps written head-interleaved (each step depends on the
                // previous one of the same head: back to back they cost a wait state each).  Every 16-lane token group keeps
                // its OWN running max: no cross-row reduction per block, and the rescale is an exec-masked branch that is
                // rarely taken after the first blocks.  The groups are merged once, after the loop.
                float sc[REP];
#pragma unroll
                for (int h = 0; h < REP; ++h) {
                    sc[h] = 0.0f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) sc[h] = T::dot2(qr[h][j], kw[j], sc[h]);
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
                    sc[h] = valid ? sc[h] * sl2 : ATTN_NEG;
                    grow |= sc[h] > m[h];
                }
                if (grow) {
#pragma unroll
                    for (int h = 0; h < REP; ++h) {
                        const float m_new = sc[h] > m[h] ? sc[h] : m[h];
                        const float alpha = attn_exp2(m[h] - m_new);
                        l[h] *= alpha;
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[h][j] *= alpha;
                        m[h] = m_new;
                    }
                }
#pragma unroll
                for (int h = 0; h < REP; ++h) {
                    const float p = valid ? attn_exp2(sc[h] - m[h]) : 0.0f;
                    l[h] += p;
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[h][j] = fmaf(p, vf[j], acc[h][j]);
                }
            }
            issue(d, b + DA);
        }
    }

    ATTN_STAMP(3);  // scoring loop done
    if constexpr (WIDE) {
        // lane (ts, dc): stream wave * TPW + ts, dims dc * 8 .. + 7 of every head
        const int str = wave * TPW + ts;
#pragma unroll
        for (int h = 0; h < REP && on; ++h) {
            if (dc == 0) s_m[h][str] = m[h], s_l[h][str] = l[h];
            *reinterpret_cast<float4 *>(&s_acc[h][str][dc * 8]) = make_float4(acc[h][0], acc[h][1], acc[h][2], acc[h][3]);
            *reinterpret_cast<float4 *>(&s_acc[h][str][dc * 8 + 4]) = make_float4(acc[h][4], acc[h][5], acc[h][6], acc[h][7]);
        }
    } else {
    // merge the token groups of the wave (lanes with equal dc): common max, rescale, plain sums; then one stream per
    // wave goes to LDS
#pragma unroll
    for (int h = 0; h < REP; ++h) {
        float mw = m[h];
        if (LPT == 8) mw = fmaxf(mw, ror8(mw));
        mw = xor32_max(xor16_max(mw));
        const float wg = attn_exp2(m[h] - mw);  // 0 for a group that saw no valid position (m = ATTN_NEG)
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
    if (ts == 0 && on) {
#pragma unroll
        for (int h = 0; h < REP; ++h) {
            if (dc == 0) s_m[h][wave] = m[h], s_l[h][wave] = l[h];
#pragma unroll
            for (int j = 0; j < 8; ++j) s_acc[h][wave][dc * 8 + j] = acc[h][j];
        }
    }
    }
    ATTN_STAMP(4);
    __syncthreads();
    ATTN_STAMP(5);
    // final pass: one (head, dim pair) per thread and iteration -- the streams' weights are computed once for both dims, the
    // accumulators come as 8-byte LDS reads (one dim per thread took 1.0 of the workgroup's 4.2 us at T ~ 200)
    for (int o = threadIdx.x; o < REP * (D / 2); o += NT) {
        const int h = o / (D / 2), d = (o % (D / 2)) * 2;
        float M = ATTN_NEG;
#pragma unroll
        for (int i = 0; i < NSTR; ++i) M = fmaxf(M, s_m[h][i]);
        float Lsum = 0.0f, A0 = 0.0f, A1 = 0.0f;
#pragma unroll
        for (int i = 0; i < NSTR; ++i) {
            const float w = attn_exp2(s_m[h][i] - M);
            const float2 av = *reinterpret_cast<const float2 *>(&s_acc[h][i][d]);
            Lsum = fmaf(w, s_l[h][i], Lsum);
            A0 = fmaf(w, av.x, A0), A1 = fmaf(w, av.y, A1);
        }
        const size_t hq = (size_t)row * a.Hq + q0 + h;
        if constexpr (PAGED) {
            if (a.splits == 1 && a.ctx_len) {  // a batch of short sequences, one split each: the partial IS the result (k_attn_combine would
                // compute fma(1, acc, 0) / fma(1, l, 0) -- the same bits) and the launcher skips the combine launch
                *reinterpret_cast<u32 *>(a.out + hq * D + d) = pack2<T>(A0 / Lsum, A1 / Lsum);
                continue;
            }
        }
        *reinterpret_cast<float2 *>(a.part_acc + (hq * a.splits + split) * D + d) = make_float2(A0, A1);
        if (d == 0) {
            a.part_ml[(hq * a.splits + split) * 2 + 0] = M;
            a.part_ml[(hq * a.splits + split) * 2 + 1] = Lsum;
        }
    }
    ATTN_STAMP(6);
}

template <class T, int D, int REP, bool PAGED = false, bool NTKV = false, int WAVES = ATTN_WAVES, bool RING = false>
__global__ void __launch_bounds__(WAVES * 64) k_attn_decode(const AttnArgs a) {
    constexpr int NT = WAVES * 64;
    const int g = blockIdx.x, split = blockIdx.y;
    if (split >= a.splits) {  // warm-up role (uniform per workgroup)
        const unsigned nblk = (unsigned)a.pf_rows * gridDim.x, bid = (unsigned)(split - a.splits) * gridDim.x + g;
        unsigned acc = 0;
        const unsigned long long n16 = a.pf_bytes >> 4;  // 16-byte pieces
        const uint4 *src = reinterpret_cast<const uint4 *>(a.pf_ptr);
        for (unsigned long long i = (unsigned long long)bid * NT + threadIdx.x; i < n16; i += (unsigned long long)nblk * NT) {
            const uint4 v = src[i];
            acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
        if (acc == 0x9e3779b9u) a.pf_sink[0] = acc;  // keeps the loads alive; practically never taken
        return;
    }
    attn_decode_body<T, D, REP, PAGED, NTKV, WAVES, AttnNoSeam, RING>(a, g, split, (int)blockIdx.z, g * REP);
}

// Merge of the active splits for 8 consecutive dims [d0, d0+8) of q-head h (fp32):
// out[d] = sum_j w_j acc_j[d] / sum_j w_j l_j,  w_j = exp(m_j - max m).  Split in a load half and a math half so a
// caller can put other loads in flight between them.  Loads are issued for all MAXS slots (clamped to an active
// one) so they are independent; inactive slots get weight 0.
template <int MAXS>
struct AttnMergeRegs {
    float mj[MAXS], lj[MAXS];
    float4 a0[MAXS], a1[MAXS];
};
// PAST_L1: the partials were written by other workgroups of THIS launch (the fused q|k|v + attention launch merges a head once its last split
// has arrived, w4_gemv.hpp): every read is an sc1 load served by the XCD's L2, never by a line parked in the CU's L1 (four heads share one
// 128-byte line of part_ml, and a CU can host the mergers of several of them).
template <bool PAST_L1>
__device__ __forceinline__ float2 attn_part_load2(const float *p) {
    if constexpr (PAST_L1) {
        const unsigned long long v = __hip_atomic_load(reinterpret_cast<unsigned long long *>(const_cast<float *>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return make_float2(__builtin_bit_cast(float, (unsigned)v), __builtin_bit_cast(float, (unsigned)(v >> 32)));
    } else {
        return *reinterpret_cast<const float2 *>(p);
    }
}
template <bool PAST_L1>
__device__ __forceinline__ float4 attn_part_load4(const float *p) {
    if constexpr (PAST_L1) {
        const float2 lo = attn_part_load2<true>(p), hi = attn_part_load2<true>(p + 2);
        return make_float4(lo.x, lo.y, hi.x, hi.y);
    } else {
        return *reinterpret_cast<const float4 *>(p);
    }
}
template <int MAXS, bool PAST_L1 = false>
__device__ __forceinline__ void attn_merge_load(const float *part_acc, const float *part_ml, int splits, int active, int h, int D, int d0,
                                                AttnMergeRegs<MAXS> &r) {
#pragma unroll
    for (int j = 0; j < MAXS; ++j) {
        const int jc = j < active ? j : active - 1;
        const float2 ml = attn_part_load2<PAST_L1>(part_ml + ((size_t)h * splits + jc) * 2);
        r.mj[j] = ml.x, r.lj[j] = ml.y;
        const float *pa = part_acc + ((size_t)h * splits + jc) * D + d0;
        r.a0[j] = attn_part_load4<PAST_L1>(pa), r.a1[j] = attn_part_load4<PAST_L1>(pa + 4);
    }
}
template <int MAXS>
__device__ __forceinline__ void attn_merge_finish(const AttnMergeRegs<MAXS> &r, int active, float (&out)[8]) {
    float M = ATTN_NEG;
#pragma unroll
    for (int j = 0; j < MAXS; ++j) M = fmaxf(M, j < active ? r.mj[j] : ATTN_NEG);
    float Lsum = 0.0f, A[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < MAXS; ++j) {
        const float w = j < active ? attn_exp2(r.mj[j] - M) : 0.0f;
        Lsum = fmaf(w, r.lj[j], Lsum);
        A[0] = fmaf(w, r.a0[j].x, A[0]), A[1] = fmaf(w, r.a0[j].y, A[1]), A[2] = fmaf(w, r.a0[j].z, A[2]), A[3] = fmaf(w, r.a0[j].w, A[3]);
        A[4] = fmaf(w, r.a1[j].x, A[4]), A[5] = fmaf(w, r.a1[j].y, A[5]), A[6] = fmaf(w, r.a1[j].z, A[6]), A[7] = fmaf(w, r.a1[j].w, A[7]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = A[i] / Lsum;
}
template <int MAXS>
__device__ __forceinline__ void attn_merge8(const float *part_acc, const float *part_ml, int splits, int active, int h, int D, int d0,
                                            float (&out)[8]) {
    AttnMergeRegs<MAXS> r;
    attn_merge_load<MAXS>(part_acc, part_ml, splits, active, h, D, d0, r);
    attn_merge_finish<MAXS>(r, active, out);
}

// Stand-alone merge (op-level pie_sdpa_decode, and the decoder at long context where more than GEMV_ATTN_SPLITS splits
// are needed to spread the work over the chip): grid Hq, block 256 threads = (D/8 pieces of 8 dims) x (256/(D/8) split
// groups).  Thread (piece, group g) folds splits g, g + NG, ... (all loads independent: one latency, not `active`
// of them in series -- the serial version cost 7 us per layer at 32 splits); the groups are then summed in fixed order.
template <class T>
__global__ void __launch_bounds__(256) k_attn_combine(const AttnArgs a, int D) {
    __shared__ float s_part[32][16][9];  // [group][piece][l, acc[8]]
    const int row = blockIdx.y, PPH = D >> 3, NG = 256 / PPH;
    const size_t h = (size_t)row * a.Hq + blockIdx.x;
    const int pc = threadIdx.x % PPH, grp = threadIdx.x / PPH, d0 = pc * 8, lane = threadIdx.x & 63;
    const int Ttot = a.ctx_len ? a.ctx_len[row] : a.ring_stage ? ring_len(*a.state) : (a.state ? a.state->pos + 1 : a.T) + row;
    const int active = attn_split(Ttot, a.splits).active;  // <= ATTN_MAX_SPLITS <= 64; 0 for an idle paged slot
    const float *ml = a.part_ml + h * a.splits * 2;
    const float *pa = a.part_acc + h * a.splits * D + d0;
    const float M = wave_max(lane < active ? ml[2 * lane] : ATTN_NEG);
    float Lsum = 0.0f, A[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = grp; j < active; j += NG) {
        const float2 mj = *reinterpret_cast<const float2 *>(ml + 2 * j);
        const float4 a0 = *reinterpret_cast<const float4 *>(pa + (size_t)j * D), a1 = *reinterpret_cast<const float4 *>(pa + (size_t)j * D + 4);
        const float w = attn_exp2(mj.x - M);
        Lsum = fmaf(w, mj.y, Lsum);
        A[0] = fmaf(w, a0.x, A[0]), A[1] = fmaf(w, a0.y, A[1]), A[2] = fmaf(w, a0.z, A[2]), A[3] = fmaf(w, a0.w, A[3]);
        A[4] = fmaf(w, a1.x, A[4]), A[5] = fmaf(w, a1.y, A[5]), A[6] = fmaf(w, a1.z, A[6]), A[7] = fmaf(w, a1.w, A[7]);
    }
    s_part[grp][pc][0] = Lsum;
#pragma unroll
    for (int i = 0; i < 8; ++i) s_part[grp][pc][1 + i] = A[i];
    __syncthreads();
    if (grp == 0) {
        const int ng = active < NG ? active : NG;  // groups beyond the active splits hold zeros
        for (int g = 1; g < ng; ++g) {
            Lsum += s_part[g][pc][0];
#pragma unroll
            for (int i = 0; i < 8; ++i) A[i] += s_part[g][pc][1 + i];
        }
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = active ? A[i] / Lsum : 0.0f;
        *reinterpret_cast<uint4 *>(a.out + h * D + d0) =
            make_uint4(pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3]), pack2<T>(o[4], o[5]), pack2<T>(o[6], o[7]));
    }
}

// combine = false: leave the partials for the consumer's prologue (decoder: o_proj GEMV, PRO_ATTN).
int attn_decode_launch(int dtype, int D, AttnArgs &a, bool combine, hipStream_t stream);
