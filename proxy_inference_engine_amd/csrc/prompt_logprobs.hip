// prompt_logprobs.hip -- the log-probabilities of prompt tokens (`echo`, vLLM's prompt_logprobs): every row's target token and its n best,
// straight from a block of 16-bit logits.
//
// The composition it replaces -- pie_logprobs_argmax per row, then pie_top_logprobs -- writes and re-reads an fp32 [rows, V] block of
// log-probabilities to keep rows x (n + 1) pairs.  Here no fp32 row exists: four launches read the T logits twice and write the records.
//   1. k_logits_stats over (TAIL_STAT_TILES, rows): the tail's own per-tile partials (tail.hpp);
//   2. k_plp_lse, one workgroup per row: logits_merge_partials -- the very function k_logits_finish ends its merge in -- into one float
//      per row.  Once per row, not once per slice workgroup: a row of V = 128256 has 251 slice workgroups, and each merging the row's 4 KB
//      of partials for itself would read 1 MB through L2 to rank 256 KB of logits;
//   3. k_plp_slices / 4. k_plp_merge: topn_select.hpp's selection over value(i) = f32(logits[i]) - lse, the subtraction k_logits_finish
//      stores.  Ranking on these values, not on the logits: two logits may round to one log-probability, and the tie then goes to the lower id.
// A row with count <= 0 leaves launch 3 at once; count < 0 leaves launch 4 too.  Deterministic: no atomics, no arrival order.
#include "prompt_logprobs.hpp"
#include "tail.hpp"
#include "topn_select.hpp"

namespace {

struct PlpArgs {
    const u16 *logits;
    const float *lse;  // [rows]
    TlpOut o;
};

// workspace: the partials, the rows' lse (padded to 8 bytes), the slices' candidates
struct PlpLayout {
    size_t lse, cand, bytes;
    PlpLayout(int rows, int V, int n) {
        lse = sizeof(LogitStat) * TAIL_STAT_TILES * (size_t)rows;
        cand = lse + (((size_t)rows * sizeof(float) + 7) & ~(size_t)7);
        bytes = cand + (size_t)rows * tlp_slices(V) * n * sizeof(unsigned long long);
    }
};

__global__ void __launch_bounds__(256) k_plp_lse(const LogitStat *stats, const int *count, float *lse) {
    if (count && count[blockIdx.x] < 0) return;  // block-uniform: the row is not scored
    int tok;
    const float v = logits_merge_partials(stats + (size_t)blockIdx.x * TAIL_STAT_TILES, TAIL_STAT_TILES, tok);
    if (threadIdx.x == 0) lse[blockIdx.x] = v;
}

template <class T>
__global__ void __launch_bounds__(TLP_T) k_plp_slices(const PlpArgs a) {
    const u16 *x = a.logits + (size_t)blockIdx.y * a.o.V;
    const float lse = a.lse[blockIdx.y];  // (a row that is not scored: whatever the workspace held, and never used)
    tlp_slices_body(a.o, [x, lse](int i) { return T::to_f32(x[i]) - lse; });
}

template <class T, int NT>
__global__ void __launch_bounds__(NT) k_plp_merge(const PlpArgs a, int G) {
    const u16 *x = a.logits + (size_t)blockIdx.x * a.o.V;
    const float lse = a.lse[blockIdx.x];
    tlp_merge_body<NT>(a.o, G, [x, lse](int i) { return T::to_f32(x[i]) - lse; });
}

}  // namespace

int prompt_logprobs_check(const char *who, int rows, int V, int dtype, int n, bool have_logits, const void *logits, const void *targets, const void *count,
                          const void *out_ids, const void *out_vals, const void *workspace) {
    const std::string w(who);
    PIE_REQUIRE(n >= 1 && n <= PIE_TOP_LOGPROBS_MAX, PIE_E_ARG, w + ": n must be 1..20");
    PIE_REQUIRE((logits || !have_logits) && out_ids && out_vals && workspace, PIE_E_ARG, w + ": null pointer");
    PIE_REQUIRE(rows >= 1 && rows <= 65535 && V >= 1 && V <= TLP_MAX_WGS * TLP_SLICE, PIE_E_SHAPE, w + ": 1 <= rows <= 65535 and 1 <= V <= 524288");
    PIE_REQUIRE(pie_aligned(targets, 4) && pie_aligned(count, 4) && pie_aligned(out_ids, 4) && pie_aligned(out_vals, 4), PIE_E_ALIGN,
                w + ": targets, count and the outputs need 4-byte alignment");
    PIE_REQUIRE(!have_logits || pie_aligned(logits, 2), PIE_E_ALIGN, w + ": logits need 2-byte alignment");
    PIE_REQUIRE(pie_aligned(workspace, 8), PIE_E_ALIGN, w + ": workspace needs 8-byte alignment");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, w + ": dtype must be PIE_BF16 or PIE_F16");
    return PIE_OK;
}

int prompt_logprobs_launch(const u16 *logits, int rows, int V, int dtype, int n, const int *targets, const int *count, int *out_ids, float *out_vals,
                           void *workspace, hipStream_t st) {
    const PlpLayout lay(rows, V, n);
    LogitStat *stats = (LogitStat *)workspace;
    float *lse = (float *)((char *)workspace + lay.lse);
    const PlpArgs a = {logits, lse, {V, n, targets, count, out_ids, out_vals, (unsigned long long *)((char *)workspace + lay.cand)}};
    const int G = tlp_slices(V);
    return launch_for_dtype(dtype, "prompt logprobs:", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_logits_stats<T>, dim3(TAIL_STAT_TILES, (unsigned)rows), dim3(256), 0, st, logits, V, stats);
        hipLaunchKernelGGL(k_plp_lse, dim3((unsigned)rows), dim3(256), 0, st, (const LogitStat *)stats, count, lse);
        hipLaunchKernelGGL(k_plp_slices<T>, dim3((unsigned)G, (unsigned)rows), dim3(TLP_T), 0, st, a);
        if (tlp_merge_narrow(G, n)) hipLaunchKernelGGL((k_plp_merge<T, 256>), dim3((unsigned)rows), dim3(256), 0, st, a, G);
        else hipLaunchKernelGGL((k_plp_merge<T, 1024>), dim3((unsigned)rows), dim3(1024), 0, st, a, G);  // G * n <= 1024 * 20
    });
}

extern "C" {

size_t pie_prompt_logprobs_workspace_bytes(int rows, int V, int n) {
    if (rows < 1 || rows > 65535 || V < 1 || V > TLP_MAX_WGS * TLP_SLICE || n < 1 || n > PIE_TOP_LOGPROBS_MAX) return 0;
    return PlpLayout(rows, V, n).bytes;
}

int pie_prompt_logprobs(const void *logits, int rows, int V, int dtype, int n, const int32_t *targets, const int32_t *count, int32_t *out_ids,
                        float *out_vals, void *workspace, void *stream) {
    if (int rc = prompt_logprobs_check("pie_prompt_logprobs", rows, V, dtype, n, true, logits, targets, count, out_ids, out_vals, workspace)) return rc;
    return prompt_logprobs_launch((const u16 *)logits, rows, V, dtype, n, targets, count, out_ids, out_vals, workspace, (hipStream_t)stream);
}

}  // extern "C"
