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

// The merge of one row's partials by a workgroup of 256 threads: the row's log-sum-exp (returned by every thread) and its first argmax.
// 16 independent 16-byte loads per thread, then two register passes.  k_logits_finish and the prompt scoring (prompt_logprobs.hip) both
// call it, so a row's lse has the same bits wherever it is computed.  Two barriers; called by every thread of the workgroup.
__device__ __forceinline__ float logits_merge_partials(const LogitStat *stats, int n_stats, int &tok) {
    __shared__ float s_max[4], s_sum[4];
    __shared__ int s_arg[4];
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
    tok = s_arg[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (s_max[w] > M || (s_max[w] == M && s_arg[w] < tok)) M = s_max[w], tok = s_arg[w];
    float se = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) se += st[k].sumexp > 0.0f ? st[k].sumexp * expf(st[k].max - M) : 0.0f;
    se = wave_sum(se);
    if ((threadIdx.x & 63) == 0) s_sum[wave] = se;
    __syncthreads();
    return M + logf((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
}

// Workgroup blockIdx.x of gridDim.x writes its slice of one row's log-probabilities, logprobs[i] = f32(logits[i]) - lse: the tail's finish and
// the speculative verify's rows (speculative.hip) store the same bits through it.
template <class T>
__device__ __forceinline__ void logits_write_logprobs(const u16 *logits, int V, float lse, float *logprobs) {
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
}

template <class T>
__global__ void __launch_bounds__(256) k_logits_finish(const u16 *logits, int V, const LogitStat *stats, int n_stats, float *logprobs,
                                                       int *token, DecState *state, int *history, int hist_cap, const unsigned *err_word) {
    logits += (size_t)blockIdx.y * V, stats += (size_t)blockIdx.y * n_stats, logprobs += (size_t)blockIdx.y * V, token += blockIdx.y;  // batch row
    int tok;
    const float lse = logits_merge_partials(stats, n_stats, tok);  // every workgroup merges all partials
    logits_write_logprobs<T>(logits, V, lse, logprobs);
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

// ---------------------------------------------------------------- launchers of the two stages
// The per-tile partials of one logit vector as pie_logprobs_argmax computes them (k_logits_stats over TAIL_STAT_TILES tiles), into caller-owned
// scratch: the step's tail after an edit, whose lm_head epilogue partials are stale.  mask != nullptr: the token mask is applied on the way
// (k_logits_stats_masked), and `logits` then hold -inf at every disallowed id; without one the logits are only read.
static inline int logits_stats_launch(int dtype, u16 *logits, int V, LogitStat *stats, hipStream_t st, const unsigned *mask = nullptr) {
    return launch_for_dtype(dtype, mask ? "logits mask:" : "logits tail:", [&](auto t) {
        using T = decltype(t);
        if (mask) hipLaunchKernelGGL(k_logits_stats_masked<T>, dim3(TAIL_STAT_TILES), dim3(256), 0, st, logits, V, stats, mask);
        else hipLaunchKernelGGL(k_logits_stats<T>, dim3(TAIL_STAT_TILES), dim3(256), 0, st, (const u16 *)logits, V, stats);
    });
}

// k_logits_finish over `rows` logit vectors [rows, V], each with its own n_stats partials (stats [rows, n_stats]) and its own token.
// state / history / err_word belong to the single-sequence step (rows == 1) and are nullptr elsewhere.
static inline int logits_finish_launch(int dtype, const u16 *logits, int V, int rows, const LogitStat *stats, int n_stats, float *logprobs, int *tokens,
                                       DecState *state, int *history, int hist_cap, const unsigned *err_word, hipStream_t st) {
    if (n_stats > TAIL_MAX_STATS) return pie::fail(PIE_E_SHAPE, "logits tail: too many partials");
    return launch_for_dtype(dtype, "logits tail:", [&](auto t) {
        hipLaunchKernelGGL(k_logits_finish<decltype(t)>, dim3(TAIL_FINISH_BLOCKS, rows), dim3(256), 0, st, logits, V, stats, n_stats, logprobs, tokens, state, history,
                           hist_cap, err_word);
    });
}

// `rows` logit vectors [rows, V] at once (the multi-sequence passes): stats_buf = rows * TAIL_STAT_TILES partials of scratch.  masks != nullptr:
// every row's own token mask rides the partials pass (k_logits_stats_rows_masked): masks [rows, mask_words], mask_words >= ceil(V / 32)
// (checked by every caller), mask_on [rows].  Without masks the partials pass is k_logits_stats and the logits are only read.
static inline int logits_tail_rows_launch(int dtype, u16 *logits, int V, int rows, LogitStat *stats_buf, float *logprobs, int *tokens, hipStream_t st,
                                          const unsigned *masks = nullptr, int mask_words = 0, const int *mask_on = nullptr) {
    const int rc = launch_for_dtype(dtype, "logits tail:", [&](auto t) {
        using T = decltype(t);
        const dim3 grid(TAIL_STAT_TILES, rows);
        if (masks) hipLaunchKernelGGL(k_logits_stats_rows_masked<T>, grid, dim3(256), 0, st, logits, V, stats_buf, masks, mask_words, mask_on);
        else hipLaunchKernelGGL(k_logits_stats<T>, grid, dim3(256), 0, st, (const u16 *)logits, V, stats_buf);
    });
    return rc ? rc : logits_finish_launch(dtype, logits, V, rows, stats_buf, TAIL_STAT_TILES, logprobs, tokens, nullptr, nullptr, 0, nullptr, st);
}

// The single-sequence tail over given partials.  stats == nullptr (op-level API): the per-tile partials are computed from the logits first,
// into stream-ordered scratch (hipMallocAsync; the decoder path passes its own stats and never allocates).
static inline int logits_tail_launch(int dtype, const u16 *logits, int V, const LogitStat *stats, int n_stats, float *logprobs,
                                     int *token, DecState *state, int *history, int hist_cap, hipStream_t st, const unsigned *err_word = nullptr) {
    if (stats) return logits_finish_launch(dtype, logits, V, 1, stats, n_stats, logprobs, token, state, history, hist_cap, err_word, st);
    LogitStat *tmp = nullptr;
    if (hipMallocAsync((void **)&tmp, sizeof(LogitStat) * TAIL_STAT_TILES, st) != hipSuccess)
        return pie::fail(PIE_E_HIP, "logits tail: hipMallocAsync failed");
    int rc = logits_stats_launch(dtype, const_cast<u16 *>(logits), V, tmp, st);  // unmasked: read only
    if (!rc) rc = logits_finish_launch(dtype, logits, V, 1, tmp, TAIL_STAT_TILES, logprobs, token, state, history, hist_cap, err_word, st);
    if (rc) {
        (void)hipFreeAsync(tmp, st);
        return rc;
    }
    PIE_HIP_TRY(hipFreeAsync(tmp, st));
    return PIE_OK;
}

// ---------------------------------------------------------------- the logits edits: repetition penalty and logit bias
// Repetition penalty (logits_processors/repetition.py:11-22): logits[id] = T(x < 0 ? x * penalty : x / penalty), x = f32(logits[id]), once for
// every distinct id of a window of at most PEN_MAX_IDS token ids: the reference gathers, computes and scatters, so an id that occurs several
// times is penalised once.  Logit bias (logits_params.hpp: logit_bias; logit_processor_factory.cpp builds it after the repetition penalty):
// logits[ids[t]] = T(f32(logits[ids[t]]) + bias[t]), one fp32 addition and one rounding, once for every distinct id of at most PEN_MAX_IDS entries.
//
// Four kernels -- the penalty alone or the penalty and the bias in one launch, for one logit vector (the op and the decode step) or one
// workgroup per row of a multi-sequence pass -- composed of the device phases below, each written once.  A workgroup is PEN_MAX_IDS threads,
// a thread per window entry or bias entry, and one LDS array s_ids[PEN_MAX_IDS] that both phases decide ownership through.
constexpr int PEN_MAX_IDS = 1024;

// Ownership: entry t owns `id` when the id lies in [0, V) -- anything else is skipped, never indexed -- and no earlier entry holds it.
// The scan takes two entries per LDS read (s_ids is 8-byte aligned) and compares both without a branch between them: a wave waits for
// every read before it can leave the loop, so the reads are the loop's cost (EXPERIMENTS.md, "One set of device phases").
__device__ __forceinline__ bool owns_id(const int *s_ids, int t, int id, int V) {
    bool own = id >= 0 && id < V;
    int j = 0;
    for (; own && j + 1 < t; j += 2) {
        const int2 e = *reinterpret_cast<const int2 *>(s_ids + j);
        own = (e.x != id) & (e.y != id);  // an earlier entry owns this id
    }
    return own && (j >= t || s_ids[j] != id);
}

// Penalise phase: this thread's window entry is `id` (-1: none).  One barrier; then the owners do the one read-modify-write.  Returns to the
// kernel on every path, so that a bias phase can follow.
template <class T>
__device__ __forceinline__ void penalise_phase(u16 *logits, int V, float penalty, int id, int *s_ids) {
    const int t = threadIdx.x;
    s_ids[t] = id;
    __syncthreads();
    if (!owns_id(s_ids, t, id, V)) return;
    const float x = T::to_f32(logits[id]);
    logits[id] = T::from_f32(x < 0.0f ? __fmul_rn(x, penalty) : __fdiv_rn(x, penalty));  // -0.0 is not < 0: divided
}

// Bias phase: entries base + t, t < n, of ids / bias (read on the device each launch), ownership among duplicate ids as above.  Two barriers.
// It reads what a penalise phase in front of it stored to the same id from another wave.  The rule this rests on: __syncthreads() is a
// workgroup-scope release / acquire fence around the barrier, and at workgroup scope that needs no cache maintenance here -- the waves of one
// workgroup run on one CU (the library is not built with -mtgsplit) and their global accesses go through that CU's one in-order vector L1, so
// a plain store issued before the barrier is what a plain load issued after it returns.  Nothing here crosses a workgroup.
template <class T>
__device__ __forceinline__ void bias_phase(u16 *logits, int V, const int *ids, const float *bias, int n, size_t base, int *s_ids) {
    __syncthreads();  // the penalise phase's stores are visible, and its readers of s_ids are done
    const int t = threadIdx.x;
    const int id = t < n ? ids[base + t] : -1;
    s_ids[t] = id;
    __syncthreads();
    if (owns_id(s_ids, t, id, V)) logits[id] = T::from_f32(__fadd_rn(T::to_f32(logits[id]), bias[base + t]));
}

// One logit vector.  The window is either ids[0..n) (the op, pie_logits_penalty) or -- state != nullptr, the decode step's tail -- the
// positions max(0, pos + 1 - context) .. pos of ids_by_pos, pos = state->pos: the ids the model was fed, the row's own input included
// (prompt_cache.update(ids) runs before the processors, inference_engine.py:255-266).  record: the step's input token is state->token
// (fed back by the previous tail, or set by the caller): it is written to ids_by_pos[pos] first, so fed-back tokens never visit the host.
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

// Step window: this thread's entry of the window, -1 beyond it.  Every index into ids_by_pos is checked against ids_cap here.
__device__ __forceinline__ int step_window_id(const PenArgs &a) {
    const int t = threadIdx.x;
    if (!a.state) return t < a.n ? a.ids[t] : -1;
    const int pos = a.state->pos, lo = pos + 1 - a.context > 0 ? pos + 1 - a.context : 0;
    const int n = pos + 1 - lo, p = lo + t;  // n <= context <= PEN_MAX_IDS
    if (t >= n || p < 0 || p >= a.ids_cap) return -1;
    if (a.record && p == pos) return a.ids_by_pos[p] = a.state->token;
    return a.ids_by_pos[p];
}

template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_logits_penalty(const PenArgs a) {
    __shared__ alignas(8) int s_ids[PEN_MAX_IDS];
    penalise_phase<T>(a.logits, a.V, a.penalty, step_window_id(a), s_ids);
}

struct BiasArgs {
    const int *ids;
    const float *bias;
    int n;  // 1..PEN_MAX_IDS
    int penalise;  // run the penalise phase (the caller's own decision: no float sentinel); off: nothing is recorded in ids_by_pos either
};

template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_logits_edit(const PenArgs a, const BiasArgs b) {
    __shared__ alignas(8) int s_ids[PEN_MAX_IDS];
    if (b.penalise) penalise_phase<T>(a.logits, a.V, a.penalty, step_window_id(a), s_ids);  // block-uniform
    bias_phase<T>(a.logits, a.V, b.ids, b.bias, b.n, 0, s_ids);
}

static inline int logits_penalty_launch(int dtype, const PenArgs &a, hipStream_t st) {
    return launch_for_dtype(dtype, "logits penalty:", [&](auto t) { hipLaunchKernelGGL(k_logits_penalty<decltype(t)>, dim3(1), dim3(PEN_MAX_IDS), 0, st, a); });
}

static inline int logits_edit_launch(int dtype, const PenArgs &a, const BiasArgs &b, hipStream_t st) {
    return launch_for_dtype(dtype, "logits bias:", [&](auto t) { hipLaunchKernelGGL(k_logits_edit<decltype(t)>, dim3(1), dim3(PEN_MAX_IDS), 0, st, a, b); });
}

// Every row of a multi-sequence pass at once (pie_logits_penalty_rows, pie_logits_bias_rows and the passes' tail): one
// workgroup per output row s, the penalty and the window size from the row's record table[s], the window from the row's ring
// recent[s][q & 1023] = the id fed at position q, the bias from the row's own entries t < n[s] of ids / bias [rows, cap].
struct PenRowsArgs {
    u16 *logits;
    int V, n_src;
    const pie_row_tail *table;
    int *recent;
    const int *ids, *ctx, *out_rows;
};

struct BiasRowsArgs {
    const int *ids;     // [rows, cap]
    const float *bias;  // [rows, cap]
    const int *n;       // [rows]: device memory, untrusted: clamped to [0, cap]
    int cap;            // 1..PEN_MAX_IDS
    int penalise;       // run the rows' penalties (the caller's own decision: a batch tail is set); off: nothing is recorded in the ring
};

// Row lookup: output row s is source row i = out_rows ? out_rows[s] : s of the pass's ids / ctx, at position pos = ctx[i] - 1.  False for a
// source row outside [0, n_src) and for an idle slot (pos < 0): the workgroup then returns before any barrier.
__device__ __forceinline__ bool row_lookup(const PenRowsArgs &a, int s, int &i, int &pos) {
    i = a.out_rows ? a.out_rows[s] : s;
    if (i < 0 || i >= a.n_src) return false;
    pos = a.ctx[i] - 1;
    return pos >= 0;
}

// Ring window: this thread's entry of the positions max(0, pos + 1 - context) .. pos of a row's ring, -1 beyond them.  context is device
// memory, untrusted: clamped to [1, PEN_MAX_IDS].  The window's last thread holds position pos: the row's own input id, which it records.
__device__ __forceinline__ int ring_window_id(int *ring, int context, int pos, const int *input_id) {
    const int t = threadIdx.x;
    context = context < 1 ? 1 : (context > PEN_MAX_IDS ? PEN_MAX_IDS : context);
    const int lo = pos + 1 - context > 0 ? pos + 1 - context : 0, n = pos + 1 - lo, p = lo + t;  // 1 <= n <= context
    if (t >= n) return -1;
    if (p == pos) return ring[p & (PEN_MAX_IDS - 1)] = *input_id;
    return ring[p & (PEN_MAX_IDS - 1)];
}

// A penalty of exactly 1.0 edits nothing, but the row's input id still has to reach the ring: such a row takes a window of that one entry,
// which thread 0 records.  The two rows kernels differ in what follows.  k_logits_penalty_rows leaves there, before its one barrier.
// k_logits_edit_rows must not: the row may still carry a bias, so it only skips the penalise phase.  Every exit before a barrier and every
// skipped phase is a block-uniform decision: a kernel argument, or a value that every thread reads from one address that no thread writes.
template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_logits_penalty_rows(const PenRowsArgs a) {
    __shared__ alignas(8) int s_ids[PEN_MAX_IDS];
    const int s = blockIdx.x;
    int i, pos;
    if (!row_lookup(a, s, i, pos)) return;
    const float penalty = a.table[s].penalty;
    const int id = ring_window_id(a.recent + (size_t)s * PEN_MAX_IDS, penalty == 1.0f ? 1 : a.table[s].context_size, pos, a.ids + i);
    if (penalty == 1.0f) return;
    penalise_phase<T>(a.logits + (size_t)s * a.V, a.V, penalty, id, s_ids);
}

// a.ctx == nullptr (the op, pie_logits_bias_rows): every row is live.  A row that the lookup rejects gets neither phase.
template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_logits_edit_rows(const PenRowsArgs a, const BiasRowsArgs b) {
    __shared__ alignas(8) int s_ids[PEN_MAX_IDS];
    const int s = blockIdx.x;
    int i = s, pos = 0;
    if (a.ctx && !row_lookup(a, s, i, pos)) return;
    u16 *logits = a.logits + (size_t)s * a.V;
    if (b.penalise) {
        const float penalty = a.table[s].penalty;
        const int id = ring_window_id(a.recent + (size_t)s * PEN_MAX_IDS, penalty == 1.0f ? 1 : a.table[s].context_size, pos, a.ids + i);
        if (penalty != 1.0f) penalise_phase<T>(logits, a.V, penalty, id, s_ids);
    }
    const int n = b.n[s];
    bias_phase<T>(logits, a.V, b.ids, b.bias, n < 0 ? 0 : (n > b.cap ? b.cap : n), (size_t)s * b.cap, s_ids);
}

static inline int logits_penalty_rows_launch(int dtype, const PenRowsArgs &a, int rows, hipStream_t st) {
    return launch_for_dtype(dtype, "logits penalty:", [&](auto t) { hipLaunchKernelGGL(k_logits_penalty_rows<decltype(t)>, dim3(rows), dim3(PEN_MAX_IDS), 0, st, a); });
}

static inline int logits_edit_rows_launch(int dtype, const PenRowsArgs &a, const BiasRowsArgs &b, int rows, hipStream_t st) {
    return launch_for_dtype(dtype, "logits bias:", [&](auto t) { hipLaunchKernelGGL(k_logits_edit_rows<decltype(t)>, dim3(rows), dim3(PEN_MAX_IDS), 0, st, a, b); });
}

#include "dry_penalty.hpp"  // the DRY penalty: step (5) of a tail; built on the window and row lookups above
