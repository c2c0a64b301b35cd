// topn_select.hpp -- the sort-free selection of a row's n best values, shared by top_logprobs.hip (fp32 log-probabilities) and
// prompt_logprobs.hip (16-bit logits minus the row's log-sum-exp): the composite encoding, the workgroup max, and the bodies of the two
// launches, each written once over a `value(i)` the kernel supplies.
//   * launch 1 spreads a row over ceil(V / 512) workgroups, as sampler.hip does.  A workgroup turns its slice into 64-bit composites
//     okey(x) << 32 | (0xFFFFFFFF - id) -- one unsigned max is then the rank order "value descending, id ascending" -- and extracts its best
//     c by c rounds of a workgroup max (wave64 shuffles, 4 partials through LDS, one barrier per round), removing the winner each round;
//   * launch 2, one workgroup per row, holds the slices' candidates in registers (at most 20 per thread) and takes c rounds of the same max.
//     Values are recovered from the keys (okey is a bijection), so no id read from the workspace is ever used as an index.
// No atomics, nothing depends on workgroup arrival order, and every workspace word launch 2 reads was written by launch 1 of the same call.
#pragma once
#include "sampler.hpp"  // okey / okey_inv

constexpr int TLP_T = 256;           // threads per workgroup of launch 1
constexpr int TLP_SLICE = 512;       // ids per workgroup
constexpr int TLP_MAX_WGS = 1024;    // V <= 524288
constexpr int TLP_PER = PIE_TOP_LOGPROBS_MAX;  // candidates per thread of launch 2

static inline int tlp_slices(int V) { return (V + TLP_SLICE - 1) / TLP_SLICE; }

// What both launches are given besides the row's values
struct TlpOut {
    int V, n;
    const int *tokens, *count;
    int *out_ids;
    float *out_vals;
    unsigned long long *ws;  // rows x slices x n composites; a row with count c uses the first slices x c, slice s at [s * c, s * c + c)
};

// the row's count as both launches see it: > n acts as n, < 0 skips the row.  Block-uniform.
__device__ __forceinline__ int tlp_count(const TlpOut &a, unsigned row) {
    const int c = a.count ? a.count[row] : a.n;
    return c > a.n ? a.n : c;
}

// a composite of a real id is never 0: its low word is 0xFFFFFFFF - id > 0
__device__ __forceinline__ unsigned long long tlp_composite(float v, int id) { return ((unsigned long long)okey(v) << 32) | (0xFFFFFFFFu - (unsigned)id); }
__device__ __forceinline__ int tlp_id(unsigned long long w) { return (int)(0xFFFFFFFFu - (unsigned)w); }
__device__ __forceinline__ float tlp_value(unsigned long long w) { return okey_inv((unsigned)(w >> 32)); }

// max over the workgroup of one composite per thread; every thread returns it.  s: this round's NW partials -- the caller alternates two sets,
// so a round's stores cannot overtake the previous round's loads with one barrier per round.
template <int NW>
__device__ __forceinline__ unsigned long long tlp_block_max(unsigned long long v, unsigned long long *s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ov = __shfl_xor(v, o, 64);
        v = ov > v ? ov : v;
    }
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = s[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = s[w] > m ? s[w] : m;
    return m;
}

// launch 1: grid (slices, rows), TLP_T threads.  The slice's best min(c, slice size) composites in rank order, then zeros.
// value(i): the value of id i < V of row blockIdx.y; called only for such i.
template <class F>
__device__ __forceinline__ void tlp_slices_body(const TlpOut &a, F value) {
    __shared__ unsigned long long s_part[2][TLP_T / 64];
    const unsigned row = blockIdx.y, G = gridDim.x;
    const int c = tlp_count(a, row);
    if (c <= 0) return;  // skipped row, or slot 0 only: launch 2 reads no candidate
    unsigned long long v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = (int)blockIdx.x * TLP_SLICE + (int)threadIdx.x + TLP_T * j;
        v[j] = i < a.V ? tlp_composite(value(i), i) : 0ull;
    }
    unsigned long long *dst = a.ws + (size_t)row * G * a.n + (size_t)blockIdx.x * c;
    for (int r = 0; r < c; ++r) {
        const unsigned long long w = tlp_block_max<TLP_T / 64>(v[0] > v[1] ? v[0] : v[1], s_part[r & 1]);
        if (v[0] == w) v[0] = 0;
        if (v[1] == w) v[1] = 0;
        if (threadIdx.x == 0) dst[r] = w;  // 0 once the slice is exhausted
    }
}

// launch 2: one workgroup of NT threads per row (blockIdx.x), NT * TLP_PER >= slices * n (the host picks NT).  value(id): as above; asked
// by one thread for the row's token in slot 0, after the id was checked against [0, V).
template <int NT, class F>
__device__ __forceinline__ void tlp_merge_body(const TlpOut &a, int G, F value) {
    __shared__ unsigned long long s_part[2][NT / 64];
    const unsigned row = blockIdx.x;
    const int c = tlp_count(a, row);
    if (c < 0) return;  // the row's record stays as it is
    const unsigned long long *src = a.ws + (size_t)row * G * a.n;
    const int total = G * c;
    unsigned long long cand[TLP_PER];
#pragma unroll
    for (int k = 0; k < TLP_PER; ++k) {
        const int i = (int)threadIdx.x + NT * k;
        cand[k] = i < total ? src[i] : 0ull;
    }
    int *oi = a.out_ids + (size_t)row * (a.n + 1);
    float *ov = a.out_vals + (size_t)row * (a.n + 1);
    for (int r = 0; r < c; ++r) {
        unsigned long long m = 0;
#pragma unroll
        for (int k = 0; k < TLP_PER; ++k) m = cand[k] > m ? cand[k] : m;
        const unsigned long long w = tlp_block_max<NT / 64>(m, s_part[r & 1]);
#pragma unroll
        for (int k = 0; k < TLP_PER; ++k)
            if (cand[k] == w) cand[k] = 0;
        if (threadIdx.x == 0) {
            oi[r + 1] = w ? tlp_id(w) : -1;  // fewer than c ids in the row (V < c): the fill
            ov[r + 1] = w ? tlp_value(w) : -INFINITY;
        }
    }
    if (threadIdx.x == 0) {
        for (int r = c; r < a.n; ++r) oi[r + 1] = -1, ov[r + 1] = -INFINITY;
        const int id = a.tokens ? a.tokens[row] : -1;
        const bool ok = id >= 0 && id < a.V;  // an id outside the row is never indexed
        oi[0] = ok ? id : -1;
        ov[0] = ok ? value(id) : -INFINITY;
    }
}

// launch 2's width for G slices of n candidates: G * n <= 1024 * 20
static inline bool tlp_merge_narrow(int G, int n) { return G * n <= 256 * TLP_PER; }
