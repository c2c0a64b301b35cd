// dry_penalty.hpp -- the DRY ("don't repeat yourself") sequence-repetition penalty (include/pie_hip.h, "DRY penalty"): only the
// token that would extend a verbatim repeat of the window's tail is penalised, exponentially in the length of that repeat.
//
// With the window c[0..n) (c[n-1] = the row's input id), every position i < n-1 with c[i] == c[n-1] is a candidate for the id t = c[i+1]; its
// match length L_i counts how far the ids in front of i repeat the ids in front of n-1 (at most DRY_MAX_MATCH, never across a breaker, never
// before the window's first position).  M[t] = max L_i; where M[t] >= allowed_length, x'[t] = T(f32(x[t]) - multiplier * base^(M[t] - allowed_length)),
// the power as repeated fp32 multiplications.
//
// Kernel shape: k_logits_penalty's (tail.hpp) -- one workgroup of PEN_MAX_IDS threads per logit vector, thread t holds window position t,
// everything else goes through LDS.  dry_phase is written once; k_logits_dry (the op and the decode step) and k_logits_dry_rows (one workgroup
// per row of a multi-sequence pass) differ in where the window comes from.  Three barriers, no atomics, nothing crosses a workgroup.
#pragma once
#include "tail.hpp"  // PEN_MAX_IDS, PenArgs / step_window_id, PenRowsArgs / row_lookup, ring_window_id (tail.hpp includes this file at its end)

constexpr int DRY_MAX_MATCH = PIE_DRY_MAX_MATCH, DRY_BREAKERS_MAX = PIE_DRY_BREAKERS_MAX;

// A record as the kernels use it.  The fields come from device memory and are not trusted: the three integers are clamped, multiplier and
// base only enter arithmetic (and the one comparison with 0 that switches a row off).
struct DryParams {
    float multiplier, base;
    int allowed, range, n_breakers;
};

__device__ __forceinline__ DryParams dry_params(const pie_dry_penalty &r) {
    DryParams p;
    p.multiplier = r.multiplier, p.base = r.base;
    p.allowed = r.allowed_length < 1 ? 1 : (r.allowed_length > DRY_MAX_MATCH ? DRY_MAX_MATCH : r.allowed_length);
    p.range = r.range < 1 ? 1 : (r.range > PEN_MAX_IDS ? PEN_MAX_IDS : r.range);
    p.n_breakers = r.n_breakers < 0 ? 0 : (r.n_breakers > DRY_BREAKERS_MAX ? DRY_BREAKERS_MAX : r.n_breakers);
    return p;
}

struct DryLds {
    int c[PEN_MAX_IDS];              // the window
    int2 cand[PEN_MAX_IDS];          // position i: (t = c[i+1], L_i) of a candidate, (-1, 0) otherwise
    unsigned char brk[PEN_MAX_IDS];  // c[t] is a sequence breaker
};

// The phase: this thread's window entry is `id`, at window position threadIdx.x < n (threads beyond the window hold nothing).  n, p and
// breakers are the same for every thread of the workgroup, so the one early return between the barriers is block-uniform: it reads LDS
// words that the barrier in front of it published.  Called by every thread of the workgroup.
template <class T>
__device__ __forceinline__ void dry_phase(u16 *logits, int V, const DryParams &p, const int *breakers, int id, int n, DryLds &s) {
    const int i = threadIdx.x;
    if (i < n) {
        bool b = false;
        for (int k = 0; k < p.n_breakers; ++k) b |= breakers[k] == id;  // once per window position (the loop bound and the loads are uniform)
        s.c[i] = id, s.brk[i] = b;
    }
    __syncthreads();
    if (n < 2 || s.brk[n - 1]) return;
    const int last = s.c[n - 1];
    int t = -1, L = 0;
    if (i < n - 1 && id == last) {
        const int next = s.c[i + 1];
        if (next >= 0 && next < V && !s.brk[i + 1]) {  // anything else is skipped, never indexed
            const int cap = i + 1 < DRY_MAX_MATCH ? i + 1 : DRY_MAX_MATCH;
            t = next, L = 1;
            while (L < cap && s.c[i - L] == s.c[n - 1 - L] && !s.brk[n - 1 - L]) ++L;  // i - L >= 0 and n - 1 - L > i - L
        }
    }
    if (i < n - 1) s.cand[i] = make_int2(t, L);
    __syncthreads();
    if (L < p.allowed) return;  // (not a candidate: L == 0 < 1 <= allowed) -- no barrier follows
    // ownership among the candidates of one id: the larger L, then the lower position -- so M[t] is a maximum whatever the arrival order
    bool own = true;
    for (int j = 0; own && j < n - 1; ++j) {
        const int2 e = s.cand[j];
        own = !(e.x == t && (e.y > L || (e.y == L && j < i)));
    }
    if (!own) return;
    float pen = p.multiplier;
    for (int k = p.allowed; k < L; ++k) pen = __fmul_rn(pen, p.base);  // L - allowed <= 63 roundings, each one fp32 multiplication
    logits[t] = T::from_f32(__fsub_rn(T::to_f32(logits[t]), pen));
}

// One logit vector.  The op (state == nullptr): the window is ids[0..n) and the record is `value`.  The decode step's tail: the record and
// the breakers are device memory read by every launch, the window the positions max(0, pos + 1 - range) .. pos of ids_by_pos, found and
// bounds-checked by step_window_id, which also records state->token at ids_by_pos[pos] when w.record is set.
struct DryArgs {
    PenArgs w;  // logits, V, ids / n or ids_by_pos / ids_cap / state / record (penalty and context are not used: the range is the record's)
    pie_dry_penalty value;
    const pie_dry_penalty *record;  // nullptr: `value`
    const int *breakers;            // [>= n_breakers]
};

template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_logits_dry(const DryArgs a) {
    __shared__ DryLds s;
    const DryParams p = dry_params(a.record ? *a.record : a.value);
    PenArgs w = a.w;
    int n = w.n;
    if (w.state) {
        const int pos = w.state->pos;
        if (pos < 0 || pos >= w.ids_cap) return;  // block-uniform: no window to speak of (the step's other launches report a full history)
        w.context = p.range;
        n = pos + 1 < p.range ? pos + 1 : p.range;
    }
    const int id = step_window_id(w);  // records the input token whatever the multiplier
    if (p.multiplier == 0.0f) return;  // off, block-uniform: the row keeps every bit
    dry_phase<T>(w.logits, w.V, p, a.breakers, id, n, s);
}

// One workgroup per output row s of a multi-sequence pass: record records[s], breakers[s][0..64), the window from the row's own ring
// recent[s][q & 1023].  The row's input id reaches the ring on every live row, zero record or not.
struct DryRowsArgs {
    PenRowsArgs r;  // logits, V, n_src, recent, ids, ctx, out_rows (table is not used)
    const pie_dry_penalty *records;
    const int *breakers;  // [rows, DRY_BREAKERS_MAX]
};

template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_logits_dry_rows(const DryRowsArgs a) {
    __shared__ DryLds s;
    const int row = blockIdx.x;
    int i, pos;
    if (!row_lookup(a.r, row, i, pos)) return;
    const DryParams p = dry_params(a.records[row]);
    const int id = ring_window_id(a.r.recent + (size_t)row * PEN_MAX_IDS, p.range, pos, a.r.ids + i);
    if (p.multiplier == 0.0f) return;  // block-uniform: one address that no thread writes
    dry_phase<T>(a.r.logits + (size_t)row * a.r.V, a.r.V, p, a.breakers + (size_t)row * DRY_BREAKERS_MAX, id, pos + 1 < p.range ? pos + 1 : p.range, s);
}

static inline int logits_dry_launch(int dtype, const DryArgs &a, hipStream_t st) {
    return launch_for_dtype(dtype, "logits dry penalty:", [&](auto t) { hipLaunchKernelGGL(k_logits_dry<decltype(t)>, dim3(1), dim3(PEN_MAX_IDS), 0, st, a); });
}

static inline int logits_dry_rows_launch(int dtype, const DryRowsArgs &a, int rows, hipStream_t st) {
    return launch_for_dtype(dtype, "logits dry penalty:", [&](auto t) { hipLaunchKernelGGL(k_logits_dry_rows<decltype(t)>, dim3(rows), dim3(PEN_MAX_IDS), 0, st, a); });
}
