// tail.hpp -- the end of _inference (engine/inference_engine.py:254,268-271) with the greedy sampler
// (samplers/__init__.py:37-38): logprobs = f32(logits) - logsumexp(f32(logits)); token = first argmax.
//
// Two stages: per-tile (max, sum exp(x - max), first argmax) partials -- produced either by the lm_head
// GEMV epilogue (EPI_LOGITS) or by k_logits_stats -- then k_logits_finish, in which every workgroup merges
// the partials (a few thousand, L2-resident) and writes its slice of the fp32 logprobs.
#pragma once
#include "common.hpp"
#include "w4_gemv.hpp"  // LogitStat, DecState
#include "count_penalty.hpp"  // frequency / presence penalties: step (4) of a tail

constexpr int TAIL_STAT_TILES = 256;
constexpr int TAIL_FINISH_BLOCKS = 64;

// MASKED: the token mask of the step's tail (include/pie_hip.h, "token mask and logit bias") rides this pass: token i is allowed iff bit
// i & 31 of mask[i >> 5] is set (mask holds at least ceil(V / 32) words: checked by every caller before the launch); a disallowed id is
// written back as -inf and counted as -inf, an allowed one keeps its bits.  The second loop re-reads what the same thread wrote.
template <class T, bool MASKED>
__device__ __forceinline__ void logits_stats_tile(u16 *logits, int V, LogitStat *stats, const unsigned *mask) {
    __shared__ float s_max[4], s_sum[4];
    __shared__ int s_arg[4];
    logits += (size_t)blockIdx.y * V, stats += (size_t)blockIdx.y * gridDim.x;  // blockIdx.y: row of a batch of logit vectors
    const int tile_len = (V + gridDim.x - 1) / gridDim.x;
    const int begin = blockIdx.x * tile_len, end = min(V, begin + tile_len);
    float mx = -INFINITY;
    // a thread's first index is its argmax until a larger value comes: a tile (or row) of -inf answers its first index, like mx.argmax
    int arg = begin + (int)threadIdx.x < end ? begin + (int)threadIdx.x : 0x7fffffff;
    for (int i = begin + threadIdx.x; i < end; i += 256) {
        float v;
        if constexpr (MASKED) {
            if ((mask[i >> 5] >> (i & 31)) & 1u) v = T::to_f32(logits[i]);
            else logits[i] = T::from_f32(-INFINITY), v = -INFINITY;
        } else {
            v = T::to_f32(logits[i]);
        }
        if (v > mx) mx = v, arg = i;  // ascending i per thread: first maximal index wins
    }
    const float wmax = wave_max(mx);
    int cand = (mx == wmax) ? arg : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_max[wave] = wmax, s_arg[wave] = cand;
    __syncthreads();
    float tmax = s_max[0];
    int targ = s_arg[0];
    for (int w = 1; w < 4; ++w)
        if (s_max[w] > tmax || (s_max[w] == tmax && s_arg[w] < targ)) tmax = s_max[w], targ = s_arg[w];
    float se = 0.0f;
    for (int i = begin + threadIdx.x; i < end; i += 256) se += expf(T::to_f32(logits[i]) - tmax);
    se = wave_sum(se);
    if ((threadIdx.x & 63) == 0) s_sum[wave] = se;
    __syncthreads();
    if (threadIdx.x == 0) {
        LogitStat st;
        st.max = tmax, st.sumexp = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3], st.argmax = targ, st.pad = 0;
        stats[blockIdx.x] = st;  // empty tile: max = -inf, sumexp = 0, argmax = INT_MAX (loses every tie with a real -inf tile)
    }
}

template <class T>
__global__ void __launch_bounds__(256) k_logits_stats(const u16 *logits, int V, LogitStat *stats) {
    logits_stats_tile<T, false>(const_cast<u16 *>(logits), V, stats, nullptr);
}

template <class T>
__global__ void __launch_bounds__(256) k_logits_stats_masked(u16 *logits, int V, LogitStat *stats, const unsigned *mask) {
    logits_stats_tile<T, true>(logits, V, stats, mask);
}

// The masked partials of a batch of rows, each under its own mask (pie_logprobs_argmax_rows_masked): row blockIdx.y reads the
// words masks + blockIdx.y * mask_words when mask_on[blockIdx.y] != 0 and runs k_logits_stats' unmasked body otherwise (every logit keeps its
// bits, whatever the row's words hold).  mask_on is device memory the host rewrites between launches: one thread reads it and the workgroup
// takes the decision from LDS, so the branch around the tile bodies' barriers is block-uniform by construction.
template <class T>
__global__ void __launch_bounds__(256) k_logits_stats_rows_masked(u16 *logits, int V, LogitStat *stats, const unsigned *masks, int mask_words,
                                                                  const int *mask_on) {
    __shared__ int s_on;
    if (threadIdx.x == 0) s_on = mask_on[blockIdx.y];
    __syncthreads();
    if (s_on != 0) logits_stats_tile<T, true>(logits, V, stats, masks + (size_t)blockIdx.y * mask_words);
    else logits_stats_tile<T, false>(logits, V, stats, nullptr);
}

constexpr int TAIL_MAX_STATS = 4096;  // 256 threads x 16 register-resident partials

template <class T>
__global__ void __launch_bounds__(256) k_logits_finish(const u16 *logits, int V, const LogitStat *stats, int n_stats, float *logprobs,
                                                       int *token, DecState *state, int *history, int hist_cap, const unsigned *err_word) {
    __shared__ float s_max[4], s_sum[4];
    __shared__ int s_arg[4];
    logits += (size_t)blockIdx.y * V, stats += (size_t)blockIdx.y * n_stats, logprobs += (size_t)blockIdx.y * V, token += blockIdx.y;  // batch row
    // every workgroup merges all partials: 16 independent 16-byte loads per thread, then two register passes
    LogitStat st[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = threadIdx.x + 256 * k;
        const uint4 raw = *reinterpret_cast<const uint4 *>(stats + (i < n_stats ? i : n_stats - 1));
        st[k].max = i < n_stats ? __builtin_bit_cast(float, raw.x) : -INFINITY;
        st[k].sumexp = i < n_stats ? __builtin_bit_cast(float, raw.y) : 0.0f;
        st[k].argmax = i < n_stats ? (int)raw.z : 0x7fffffff;
    }
    float mx = -INFINITY;
    int arg = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (st[k].max > mx || (st[k].max == mx && st[k].argmax < arg)) mx = st[k].max, arg = st[k].argmax;
    const float wmax = wave_max(mx);
    int cand = (mx == wmax) ? arg : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_max[wave] = wmax, s_arg[wave] = cand;
    __syncthreads();
    float M = s_max[0];
    int tok = s_arg[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (s_max[w] > M || (s_max[w] == M && s_arg[w] < tok)) M = s_max[w], tok = s_arg[w];
    float se = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) se += st[k].sumexp > 0.0f ? st[k].sumexp * expf(st[k].max - M) : 0.0f;
    se = wave_sum(se);
    if ((threadIdx.x & 63) == 0) s_sum[wave] = se;
    __syncthreads();
    const float lse = M + logf((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
    const int slice = (((V + gridDim.x - 1) / gridDim.x) + 7) & ~7;  // 8 logits per thread and pass
    const int begin = blockIdx.x * slice, end = min(V, begin + slice);
    for (int i = begin + threadIdx.x * 8; i < end; i += 256 * 8) {
        if (i + 8 <= end && (V & 7) == 0) {
            const uint4 v = *reinterpret_cast<const uint4 *>(logits + i);
            float4 o0 = make_float4(lo_f32<T>(v.x) - lse, hi_f32<T>(v.x) - lse, lo_f32<T>(v.y) - lse, hi_f32<T>(v.y) - lse);
            float4 o1 = make_float4(lo_f32<T>(v.z) - lse, hi_f32<T>(v.z) - lse, lo_f32<T>(v.w) - lse, hi_f32<T>(v.w) - lse);
            *reinterpret_cast<float4 *>(logprobs + i) = o0;
            *reinterpret_cast<float4 *>(logprobs + i + 4) = o1;
        } else {
            for (int k = i; k < min(i + 8, end); ++k) logprobs[k] = T::to_f32(logits[k]) - lse;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (err_word && *err_word != 0u) tok = -1;  // the persistent launch gave up a bounded wait (sticky): no plausible-looking id from garbage
        *token = tok;
        if (state) {
            const int next_pos = state->pos + 1;  // the position the chosen token will occupy
            if (history && next_pos < hist_cap) history[next_pos] = tok;  // device-side token history (PromptCache.computed_ids)
            state->token = tok;   // greedy auto-feed of the next step
            state->pos = next_pos;  // cache.offset += 1 (reusable.py:139)
        }
    }
}

// `rows` logit vectors [rows, V] at once (the multi-sequence decode step): stats_buf = rows * TAIL_STAT_TILES partials of scratch.
static inline int logits_tail_rows_launch(int dtype, const u16 *logits, int V, int rows, LogitStat *stats_buf, float *logprobs, int *tokens,
                                          hipStream_t st) {
    if (dtype != PIE_BF16 && dtype != PIE_F16) return pie::fail(PIE_E_ARG, "logits tail: dtype must be PIE_BF16 or PIE_F16");
    const dim3 g1(TAIL_STAT_TILES, rows), g2(TAIL_FINISH_BLOCKS, rows);
    if (dtype == PIE_BF16) {
        hipLaunchKernelGGL(k_logits_stats<BF16>, g1, dim3(256), 0, st, logits, V, stats_buf);
        hipLaunchKernelGGL(k_logits_finish<BF16>, g2, dim3(256), 0, st, logits, V, stats_buf, TAIL_STAT_TILES, logprobs, tokens, nullptr, nullptr, 0, (const unsigned *)nullptr);
    } else {
        hipLaunchKernelGGL(k_logits_stats<F16>, g1, dim3(256), 0, st, logits, V, stats_buf);
        hipLaunchKernelGGL(k_logits_finish<F16>, g2, dim3(256), 0, st, logits, V, stats_buf, TAIL_STAT_TILES, logprobs, tokens, nullptr, nullptr, 0, (const unsigned *)nullptr);
    }
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// The same two launches with every row's own token mask riding the partials pass (k_logits_stats_rows_masked): masks [rows, mask_words],
// mask_words >= ceil(V / 32) (checked by every caller), mask_on [rows].
static inline int logits_tail_rows_masked_launch(int dtype, u16 *logits, int V, int rows, LogitStat *stats_buf, const unsigned *masks, int mask_words,
                                                 const int *mask_on, float *logprobs, int *tokens, hipStream_t st) {
    if (dtype != PIE_BF16 && dtype != PIE_F16) return pie::fail(PIE_E_ARG, "logits tail: dtype must be PIE_BF16 or PIE_F16");
    const dim3 g1(TAIL_STAT_TILES, rows), g2(TAIL_FINISH_BLOCKS, rows);
    if (dtype == PIE_BF16) {
        hipLaunchKernelGGL(k_logits_stats_rows_masked<BF16>, g1, dim3(256), 0, st, logits, V, stats_buf, masks, mask_words, mask_on);
        hipLaunchKernelGGL(k_logits_finish<BF16>, g2, dim3(256), 0, st, logits, V, stats_buf, TAIL_STAT_TILES, logprobs, tokens, nullptr, nullptr, 0, (const unsigned *)nullptr);
    } else {
        hipLaunchKernelGGL(k_logits_stats_rows_masked<F16>, g1, dim3(256), 0, st, logits, V, stats_buf, masks, mask_words, mask_on);
        hipLaunchKernelGGL(k_logits_finish<F16>, g2, dim3(256), 0, st, logits, V, stats_buf, TAIL_STAT_TILES, logprobs, tokens, nullptr, nullptr, 0, (const unsigned *)nullptr);
    }
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// stats == nullptr (op-level API): the per-tile partials are computed from the logits first, into
// stream-ordered scratch (hipMallocAsync; the decoder path passes its own stats and never allocates).
static inline int logits_tail_launch(int dtype, const u16 *logits, int V, const LogitStat *stats, int n_stats, float *logprobs,
                                     int *token, DecState *state, int *history, int hist_cap, hipStream_t st, const unsigned *err_word = nullptr) {
    if (dtype != PIE_BF16 && dtype != PIE_F16) return pie::fail(PIE_E_ARG, "logits tail: dtype must be PIE_BF16 or PIE_F16");
    if (stats && n_stats > TAIL_MAX_STATS) return pie::fail(PIE_E_SHAPE, "logits tail: too many partials");
    LogitStat *tmp = nullptr;
    if (!stats) {
        if (hipMallocAsync((void **)&tmp, sizeof(LogitStat) * TAIL_STAT_TILES, st) != hipSuccess)
            return pie::fail(PIE_E_HIP, "logits tail: hipMallocAsync failed");
        if (dtype == PIE_BF16) hipLaunchKernelGGL(k_logits_stats<BF16>, dim3(TAIL_STAT_TILES), dim3(256), 0, st, logits, V, tmp);
        else hipLaunchKernelGGL(k_logits_stats<F16>, dim3(TAIL_STAT_TILES), dim3(256), 0, st, logits, V, tmp);
        PIE_LAUNCH_CHECK();
        stats = tmp, n_stats = TAIL_STAT_TILES;
    }
    if (dtype == PIE_BF16)
        hipLaunchKernelGGL(k_logits_finish<BF16>, dim3(TAIL_FINISH_BLOCKS), dim3(256), 0, st, logits, V, stats, n_stats, logprobs, token, state, history, hist_cap, err_word);
    else
        hipLaunchKernelGGL(k_logits_finish<F16>, dim3(TAIL_FINISH_BLOCKS), dim3(256), 0, st, logits, V, stats, n_stats, logprobs, token, state, history, hist_cap, err_word);
    PIE_LAUNCH_CHECK();
    if (tmp) PIE_HIP_TRY(hipFreeAsync(tmp, st));
    return PIE_OK;
}

// ---------------------------------------------------------------- repetition penalty (logits_processors/repetition.py:11-22)
// logits[id] = T(x < 0 ? x * penalty : x / penalty), x = f32(logits[id]), once for every distinct id of a window of at most PEN_MAX_IDS token
// ids: the reference gathers, computes and scatters, so an id that occurs several times is penalised once.  One workgroup, a thread per
// window entry; an entry owns its id when no earlier entry holds it.  Ids outside [0, V) are skipped, never indexed.
// The window is either ids[0..n) (the op, pie_logits_penalty) or -- state != nullptr, the decode step's tail -- the positions
// max(0, pos + 1 - context) .. pos of ids_by_pos, pos = state->pos: the ids the model was fed, the row's own input included
// (prompt_cache.update(ids) runs before the processors, inference_engine.py:255-266).  record: the step's input token is state->token
// (fed back by the previous tail, or set by the caller): it is written to ids_by_pos[pos] first, so fed-back tokens never visit the host.
// Every index into ids_by_pos is checked against ids_cap here.
constexpr int PEN_MAX_IDS = 1024;

struct PenArgs {
    u16 *logits;
    int V;
    float penalty;
    const int *ids;  // the op's window
    int n;
    int *ids_by_pos;  // the step's window
    int ids_cap, context;
    const DecState *state;
    int record;
};

template <class T>
__device__ __forceinline__ void logits_penalty_phase(const PenArgs &a, int *s_ids) {
    const int t = threadIdx.x;
    int n = a.n, id = -1;
    if (a.state) {
        const int pos = a.state->pos, lo = pos + 1 - a.context > 0 ? pos + 1 - a.context : 0;
        n = pos + 1 - lo;  // <= context <= PEN_MAX_IDS
        const int p = lo + t;
        if (t < n && p >= 0 && p < a.ids_cap) {
            if (a.record && p == pos) id = a.state->token, a.ids_by_pos[p] = id;
            else id = a.ids_by_pos[p];
        }
    } else if (t < n) {
        id = a.ids[t];
    }
    s_ids[t] = id;
    __syncthreads();
    if (t >= n || id < 0 || id >= a.V) return;
    for (int j = 0; j < t; ++j)
        if (s_ids[j] == id) return;  // an earlier entry owns this id
    const float x = T::to_f32(a.logits[id]);
    a.logits[id] = T::from_f32(x < 0.0f ? __fmul_rn(x, a.penalty) : __fdiv_rn(x, a.penalty));  // -0.0 is not < 0: divided
}

template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_logits_penalty(const PenArgs a) {
    __shared__ int s_ids[PEN_MAX_IDS];
    logits_penalty_phase<T>(a, s_ids);
}

// The logit bias (logits_params.hpp: logit_bias; logit_processor_factory.cpp builds it after the repetition penalty), in the penalty's launch:
// phase 1 is logits_penalty_phase (skipped when b.penalise == 0: then nothing is recorded in ids_by_pos either), phase 2 one thread per
// entry t < n: logits[ids[t]] = T(f32(logits[ids[t]]) + bias[t]), one fp32 addition and one rounding, for every entry whose id is in [0, V) and
// not held by an earlier entry (k_logits_penalty's rule, decided through the same LDS array).  ids / bias are read on the device each launch.
// Phase 2 reads what phase 1 stored to the same id from another wave.  The rule this rests on: __syncthreads() is a workgroup-scope release /
// acquire fence around the barrier, and at workgroup scope that needs no cache maintenance here -- the waves of one workgroup run on one CU
// (the library is not built with -mtgsplit) and their global accesses go through that CU's one in-order vector L1, so a plain store issued
// before the barrier is what a plain load issued after it returns.  Nothing here crosses a workgroup.
struct BiasArgs {
    const int *ids;
    const float *bias;
    int n;  // 1..PEN_MAX_IDS
    int penalise;  // run phase 1 (the caller's own decision: no float sentinel)
};

template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_logits_edit(const PenArgs a, const BiasArgs b) {
    __shared__ int s_ids[PEN_MAX_IDS];
    if (b.penalise) logits_penalty_phase<T>(a, s_ids);  // block-uniform
    __syncthreads();  // phase 1's stores are visible, and its readers of s_ids are done
    const int t = threadIdx.x;
    const int id = t < b.n ? b.ids[t] : -1;
    s_ids[t] = id;
    __syncthreads();
    if (id < 0 || id >= a.V) return;
    for (int j = 0; j < t; ++j)
        if (s_ids[j] == id) return;  // an earlier entry owns this id
    a.logits[id] = T::from_f32(__fadd_rn(T::to_f32(a.logits[id]), b.bias[t]));
}

static inline int logits_edit_launch(int dtype, const PenArgs &a, const BiasArgs &b, hipStream_t st) {
    if (dtype != PIE_BF16 && dtype != PIE_F16) return pie::fail(PIE_E_ARG, "logits bias: dtype must be PIE_BF16 or PIE_F16");
    if (dtype == PIE_BF16) hipLaunchKernelGGL(k_logits_edit<BF16>, dim3(1), dim3(PEN_MAX_IDS), 0, st, a, b);
    else hipLaunchKernelGGL(k_logits_edit<F16>, dim3(1), dim3(PEN_MAX_IDS), 0, st, a, b);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

static inline int logits_penalty_launch(int dtype, const PenArgs &a, hipStream_t st) {
    if (dtype != PIE_BF16 && dtype != PIE_F16) return pie::fail(PIE_E_ARG, "logits penalty: dtype must be PIE_BF16 or PIE_F16");
    if (dtype == PIE_BF16) hipLaunchKernelGGL(k_logits_penalty<BF16>, dim3(1), dim3(PEN_MAX_IDS), 0, st, a);
    else hipLaunchKernelGGL(k_logits_penalty<F16>, dim3(1), dim3(PEN_MAX_IDS), 0, st, a);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// The same penalty for every row of a multi-sequence pass at once (pie_logits_penalty_rows): one workgroup per output row s, the penalty and
// the window size from the row's record (device memory, untrusted: the context is clamped to [1, PEN_MAX_IDS]), the window from the row's
// ring recent[s][q & 1023] = the id fed at position q.  Source row i = out_rows ? out_rows[s] : s of the pass's ids / ctx (checked against
// n_src); pos = ctx[i] - 1 < 0: an idle slot, skipped.  The row's own input id is recorded at pos first; a penalty of exactly 1.0 stops there.
struct PenRowsArgs {
    u16 *logits;
    int V, n_src;
    const pie_row_tail *table;
    int *recent;
    const int *ids, *ctx, *out_rows;
};

template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_logits_penalty_rows(const PenRowsArgs a) {
    __shared__ int s_ids[PEN_MAX_IDS];
    const int t = threadIdx.x, s = blockIdx.x;
    const int i = a.out_rows ? a.out_rows[s] : s;
    if (i < 0 || i >= a.n_src) return;  // block-uniform, like every return before the barrier
    const int pos = a.ctx[i] - 1;
    if (pos < 0) return;
    int *ring = a.recent + (size_t)s * PEN_MAX_IDS;
    const float penalty = a.table[s].penalty;
    if (penalty == 1.0f) {
        if (t == 0) ring[pos & (PEN_MAX_IDS - 1)] = a.ids[i];
        return;
    }
    int context = a.table[s].context_size;
    context = context < 1 ? 1 : (context > PEN_MAX_IDS ? PEN_MAX_IDS : context);
    const int lo = pos + 1 - context > 0 ? pos + 1 - context : 0, n = pos + 1 - lo;  // 1 <= n <= context
    int id = -1;
    if (t < n) {
        const int p = lo + t;
        if (p == pos) id = a.ids[i], ring[p & (PEN_MAX_IDS - 1)] = id;
        else id = ring[p & (PEN_MAX_IDS - 1)];
    }
    s_ids[t] = id;
    __syncthreads();
    if (t >= n || id < 0 || id >= a.V) return;
    for (int j = 0; j < t; ++j)
        if (s_ids[j] == id) return;  // an earlier entry owns this id
    u16 *logits = a.logits + (size_t)s * a.V;
    const float x = T::to_f32(logits[id]);
    logits[id] = T::from_f32(x < 0.0f ? __fmul_rn(x, penalty) : __fdiv_rn(x, penalty));  // k_logits_penalty's arithmetic
}

static inline int logits_penalty_rows_launch(int dtype, const PenRowsArgs &a, int rows, hipStream_t st) {
    if (dtype != PIE_BF16 && dtype != PIE_F16) return pie::fail(PIE_E_ARG, "logits penalty: dtype must be PIE_BF16 or PIE_F16");
    if (dtype == PIE_BF16) hipLaunchKernelGGL(k_logits_penalty_rows<BF16>, dim3(rows), dim3(PEN_MAX_IDS), 0, st, a);
    else hipLaunchKernelGGL(k_logits_penalty_rows<F16>, dim3(rows), dim3(PEN_MAX_IDS), 0, st, a);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// The rows' penalties and the rows' logit biases in one launch (pie_logits_bias_rows, and the multi-sequence passes' tail when a bias is
// configured): one workgroup per output row s.  Phase 1 is k_logits_penalty_rows' body on that row (b.penalise == 0, no batch
// tail: off, and nothing is recorded in the ring), phase 2 k_logits_edit's bias phase on the row's logits with the row's own table: entries
// t < n[s] (device memory, untrusted: clamped to [0, cap]) of ids / bias [rows, cap], ownership among duplicate ids through the same LDS array.
// k_logits_penalty_rows leaves before its barrier for an idle slot, a source row out of range and a penalty of exactly 1.0; a row of the
// last kind may still carry a bias, so here only the first two leave (such a row gets neither phase) and everything else that skips phase 1
// is a block-uniform decision (a kernel argument, or a value every thread reads from one address that no thread writes), after which
// every thread reaches phase 2's barriers.  The ring is written where k_logits_penalty_rows writes it.  a.ctx == nullptr (the op): every row
// is live.  Phase 2 reads what phase 1 stored to the same id from another wave: the workgroup-scope argument above k_logits_edit.
struct BiasRowsArgs {
    const int *ids;     // [rows, cap]
    const float *bias;  // [rows, cap]
    const int *n;       // [rows]
    int cap;            // 1..PEN_MAX_IDS
    int penalise;       // run phase 1 (the caller's own decision: a batch tail is set)
};

template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_logits_edit_rows(const PenRowsArgs a, const BiasRowsArgs b) {
    __shared__ int s_ids[PEN_MAX_IDS];
    const int t = threadIdx.x, s = blockIdx.x;
    int i = s, pos = 0;
    if (a.ctx) {
        i = a.out_rows ? a.out_rows[s] : s;
        if (i < 0 || i >= a.n_src) return;  // block-uniform, and before every barrier
        pos = a.ctx[i] - 1;
        if (pos < 0) return;  // likewise
    }
    u16 *logits = a.logits + (size_t)s * a.V;
    const float penalty = b.penalise ? a.table[s].penalty : 1.0f;
    if (b.penalise && penalty == 1.0f && t == 0) a.recent[(size_t)s * PEN_MAX_IDS + (pos & (PEN_MAX_IDS - 1))] = a.ids[i];
    if (penalty != 1.0f) {  // block-uniform: phase 1, k_logits_penalty_rows from its window on
        int *ring = a.recent + (size_t)s * PEN_MAX_IDS;
        int context = a.table[s].context_size;
        context = context < 1 ? 1 : (context > PEN_MAX_IDS ? PEN_MAX_IDS : context);
        const int lo = pos + 1 - context > 0 ? pos + 1 - context : 0, n = pos + 1 - lo;  // 1 <= n <= context
        int id = -1;
        if (t < n) {
            const int p = lo + t;
            if (p == pos) id = a.ids[i], ring[p & (PEN_MAX_IDS - 1)] = id;
            else id = ring[p & (PEN_MAX_IDS - 1)];
        }
        s_ids[t] = id;
        __syncthreads();
        bool own = t < n && id >= 0 && id < a.V;
        for (int j = 0; own && j < t; ++j) own = s_ids[j] != id;  // an earlier entry owns this id
        if (own) {
            const float x = T::to_f32(logits[id]);
            logits[id] = T::from_f32(x < 0.0f ? __fmul_rn(x, penalty) : __fdiv_rn(x, penalty));  // k_logits_penalty's arithmetic
        }
    }
    __syncthreads();  // phase 1's stores are visible, and its readers of s_ids are done
    int bn = b.n[s];
    bn = bn < 0 ? 0 : (bn > b.cap ? b.cap : bn);
    const int id = t < bn ? b.ids[(size_t)s * b.cap + t] : -1;
    s_ids[t] = id;
    __syncthreads();
    if (id < 0 || id >= a.V) return;
    for (int j = 0; j < t; ++j)
        if (s_ids[j] == id) return;  // an earlier entry owns this id
    logits[id] = T::from_f32(__fadd_rn(T::to_f32(logits[id]), b.bias[(size_t)s * b.cap + t]));
}

static inline int logits_edit_rows_launch(int dtype, const PenRowsArgs &a, const BiasRowsArgs &b, int rows, hipStream_t st) {
    if (dtype != PIE_BF16 && dtype != PIE_F16) return pie::fail(PIE_E_ARG, "logits bias: dtype must be PIE_BF16 or PIE_F16");
    if (dtype == PIE_BF16) hipLaunchKernelGGL(k_logits_edit_rows<BF16>, dim3(rows), dim3(PEN_MAX_IDS), 0, st, a, b);
    else hipLaunchKernelGGL(k_logits_edit_rows<F16>, dim3(rows), dim3(PEN_MAX_IDS), 0, st, a, b);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// The per-tile partials of `logits` as pie_logprobs_argmax computes them (k_logits_stats over TAIL_STAT_TILES tiles), into caller-owned
// scratch: the step's tail after a penalty, whose lm_head epilogue partials are stale.
static inline int logits_stats_launch(int dtype, const u16 *logits, int V, LogitStat *stats, hipStream_t st) {
    if (dtype == PIE_BF16) hipLaunchKernelGGL(k_logits_stats<BF16>, dim3(TAIL_STAT_TILES), dim3(256), 0, st, logits, V, stats);
    else hipLaunchKernelGGL(k_logits_stats<F16>, dim3(TAIL_STAT_TILES), dim3(256), 0, st, logits, V, stats);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// The same partials with the token mask applied on the way (k_logits_stats_masked): `logits` then hold -inf at every disallowed id.
static inline int logits_stats_masked_launch(int dtype, u16 *logits, int V, const unsigned *mask, LogitStat *stats, hipStream_t st) {
    if (dtype != PIE_BF16 && dtype != PIE_F16) return pie::fail(PIE_E_ARG, "logits mask: dtype must be PIE_BF16 or PIE_F16");
    if (dtype == PIE_BF16) hipLaunchKernelGGL(k_logits_stats_masked<BF16>, dim3(TAIL_STAT_TILES), dim3(256), 0, st, logits, V, stats, mask);
    else hipLaunchKernelGGL(k_logits_stats_masked<F16>, dim3(TAIL_STAT_TILES), dim3(256), 0, st, logits, V, stats, mask);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}
