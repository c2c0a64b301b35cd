// top_logprobs.hip -- the n best log-probabilities of every row plus the chosen token's own, sort-free.
//
// The reference answers a `top_logprobs` request with get_top_logprobs (engine/utils.py:4-48): an argpartition of the [V] row, a gather and
// a sort of the k survivors.  Restated with library ops that is a sort of 128 k floats and two host round trips per token; here it is two
// launches that read the row once:
//   * launch 1 spreads a row over ceil(V / 512) workgroups, as sampler.hip does.  A workgroup turns its slice into 64-bit composites
//     okey(x) << 32 | (0xFFFFFFFF - id) -- one unsigned max is then the rank order "value descending, id ascending" -- and extracts its best
//     c by c rounds of a workgroup max (wave64 shuffles, 4 partials through LDS, one barrier per round), removing the winner each round;
//   * launch 2, one workgroup per row, holds the slices' candidates in registers (at most 20 per thread) and takes c rounds of the same max.
//     Values are recovered from the keys (okey is a bijection), so no id read from the workspace is ever used as an index.
// No atomics, nothing depends on workgroup arrival order, and every workspace word launch 2 reads was written by launch 1 of the same call.
#include "sampler.hpp"
#include "top_logprobs.hpp"

namespace {

constexpr int TLP_T = 256;           // threads per workgroup of launch 1
constexpr int TLP_SLICE = 512;       // ids per workgroup
constexpr int TLP_MAX_WGS = 1024;    // V <= 524288
constexpr int TLP_PER = PIE_TOP_LOGPROBS_MAX;  // candidates per thread of launch 2

struct TlpArgs {
    const float *logprobs;
    int V, n;
    const int *tokens, *count;
    int *out_ids;
    float *out_vals;
    unsigned long long *ws;  // rows x slices x n composites; a row with count c uses the first slices x c, slice s at [s * c, s * c + c)
};

// the row's count as both launches see it: > n acts as n, < 0 skips the row.  Block-uniform.
__device__ __forceinline__ int tlp_count(const TlpArgs &a, unsigned row) {
    const int c = a.count ? a.count[row] : a.n;
    return c > a.n ? a.n : c;
}

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

// launch 1: grid (slices, rows).  The slice's best min(c, slice size) composites in rank order, then zeros (a composite of a real id is never 0:
// its low word is 0xFFFFFFFF - id > 0).
__global__ void __launch_bounds__(TLP_T) k_tlp_slices(const TlpArgs a) {
    __shared__ unsigned long long s_part[2][TLP_T / 64];
    const unsigned row = blockIdx.y, G = gridDim.x;
    const int c = tlp_count(a, row);
    if (c <= 0) return;  // skipped row, or slot 0 only: launch 2 reads no candidate
    const float *x = a.logprobs + (size_t)row * a.V;
    unsigned long long v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = (int)blockIdx.x * TLP_SLICE + (int)threadIdx.x + TLP_T * j;
        v[j] = i < a.V ? ((unsigned long long)okey(x[i]) << 32) | (0xFFFFFFFFu - (unsigned)i) : 0ull;
    }
    unsigned long long *dst = a.ws + (size_t)row * G * a.n + (size_t)blockIdx.x * c;
    for (int r = 0; r < c; ++r) {
        const unsigned long long w = tlp_block_max<TLP_T / 64>(v[0] > v[1] ? v[0] : v[1], s_part[r & 1]);
        if (v[0] == w) v[0] = 0;
        if (v[1] == w) v[1] = 0;
        if (threadIdx.x == 0) dst[r] = w;  // 0 once the slice is exhausted
    }
}

// launch 2: one workgroup of NT threads per row, NT * TLP_PER >= slices * n (the host picks NT).
template <int NT>
__global__ void __launch_bounds__(NT) k_tlp_merge(const TlpArgs a, int G) {
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
            oi[r + 1] = w ? (int)(0xFFFFFFFFu - (unsigned)w) : -1;  // fewer than c ids in the row (V < c): the fill
            ov[r + 1] = w ? okey_inv((unsigned)(w >> 32)) : -INFINITY;
        }
    }
    if (threadIdx.x == 0) {
        for (int r = c; r < a.n; ++r) oi[r + 1] = -1, ov[r + 1] = -INFINITY;
        const int id = a.tokens ? a.tokens[row] : -1;
        const bool ok = id >= 0 && id < a.V;  // an id outside the row is never indexed
        oi[0] = ok ? id : -1;
        ov[0] = ok ? a.logprobs[(size_t)row * a.V + id] : -INFINITY;
    }
}

}  // namespace

int top_logprobs_check(const char *who, int rows, int V, int n, bool have_logprobs, const void *logprobs, const void *tokens, const void *count,
                       const void *out_ids, const void *out_vals, const void *workspace) {
    const std::string w(who);
    PIE_REQUIRE(n >= 1 && n <= PIE_TOP_LOGPROBS_MAX, PIE_E_ARG, w + ": n must be 1..20");
    PIE_REQUIRE((logprobs || !have_logprobs) && out_ids && out_vals && workspace, PIE_E_ARG, w + ": null pointer");
    PIE_REQUIRE(rows >= 1 && rows <= 65535 && V >= 1 && V <= TLP_MAX_WGS * TLP_SLICE, PIE_E_SHAPE, w + ": 1 <= rows <= 65535 and 1 <= V <= 524288");
    PIE_REQUIRE((!have_logprobs || pie_aligned(logprobs, 4)) && pie_aligned(tokens, 4) && pie_aligned(count, 4) && pie_aligned(out_ids, 4) && pie_aligned(out_vals, 4), PIE_E_ALIGN,
                w + ": logprobs, tokens, count and the outputs need 4-byte alignment");
    PIE_REQUIRE(pie_aligned(workspace, 8), PIE_E_ALIGN, w + ": workspace needs 8-byte alignment");
    return PIE_OK;
}

int top_logprobs_launch(const float *logprobs, int rows, int V, int n, const int *tokens, const int *count, int *out_ids, float *out_vals, void *workspace,
                        hipStream_t st) {
    TlpArgs a = {};
    a.logprobs = logprobs, a.V = V, a.n = n, a.tokens = tokens, a.count = count, a.out_ids = out_ids, a.out_vals = out_vals;
    a.ws = (unsigned long long *)workspace;
    const int G = (V + TLP_SLICE - 1) / TLP_SLICE;
    hipLaunchKernelGGL(k_tlp_slices, dim3((unsigned)G, (unsigned)rows), dim3(TLP_T), 0, st, a);
    if (G * n <= 256 * TLP_PER) hipLaunchKernelGGL(k_tlp_merge<256>, dim3((unsigned)rows), dim3(256), 0, st, a, G);
    else hipLaunchKernelGGL(k_tlp_merge<1024>, dim3((unsigned)rows), dim3(1024), 0, st, a, G);  // G * n <= 1024 * 20
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

extern "C" {

size_t pie_top_logprobs_workspace_bytes(int rows, int V, int n) {
    if (rows < 1 || V < 1 || n < 1 || n > PIE_TOP_LOGPROBS_MAX) return 0;
    const int G = (V + TLP_SLICE - 1) / TLP_SLICE;
    return G > TLP_MAX_WGS ? 0 : (size_t)rows * G * n * sizeof(unsigned long long);
}

int pie_top_logprobs(const float *logprobs, int rows, int V, int n, const int32_t *tokens, const int32_t *count, int32_t *out_ids, float *out_vals,
                     void *workspace, void *stream) {
    if (int rc = top_logprobs_check("pie_top_logprobs", rows, V, n, true, logprobs, tokens, count, out_ids, out_vals, workspace)) return rc;
    return top_logprobs_launch(logprobs, rows, V, n, tokens, count, out_ids, out_vals, workspace, (hipStream_t)stream);
}

}  // extern "C"
