// top_logprobs.hip -- the n best log-probabilities of every row plus the chosen token's own, sort-free.
//
// The reference answers a `top_logprobs` request with get_top_logprobs (engine/utils.py:4-48): an argpartition of the [V] row, a gather and
// a sort of the k survivors.  Restated with library ops that is a sort of 128 k floats and two host round trips per token; here it is two
// launches that read the row once: the selection of topn_select.hpp over the row's fp32 log-probabilities.
#include "top_logprobs.hpp"
#include "topn_select.hpp"

namespace {

struct TlpArgs {
    const float *logprobs;
    TlpOut o;
};

__global__ void __launch_bounds__(TLP_T) k_tlp_slices(const TlpArgs a) {
    const float *x = a.logprobs + (size_t)blockIdx.y * a.o.V;
    tlp_slices_body(a.o, [x](int i) { return x[i]; });
}

template <int NT>
__global__ void __launch_bounds__(NT) k_tlp_merge(const TlpArgs a, int G) {
    const float *x = a.logprobs + (size_t)blockIdx.x * a.o.V;
    tlp_merge_body<NT>(a.o, G, [x](int i) { return x[i]; });
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
    const TlpArgs a = {logprobs, {V, n, tokens, count, out_ids, out_vals, (unsigned long long *)workspace}};
    const int G = tlp_slices(V);
    hipLaunchKernelGGL(k_tlp_slices, dim3((unsigned)G, (unsigned)rows), dim3(TLP_T), 0, st, a);
    if (tlp_merge_narrow(G, n)) hipLaunchKernelGGL(k_tlp_merge<256>, dim3((unsigned)rows), dim3(256), 0, st, a, G);
    else hipLaunchKernelGGL(k_tlp_merge<1024>, dim3((unsigned)rows), dim3(1024), 0, st, a, G);  // G * n <= 1024 * 20
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

extern "C" {

size_t pie_top_logprobs_workspace_bytes(int rows, int V, int n) {
    if (rows < 1 || V < 1 || n < 1 || n > PIE_TOP_LOGPROBS_MAX) return 0;
    const int G = tlp_slices(V);
    return G > TLP_MAX_WGS ? 0 : (size_t)rows * G * n * sizeof(unsigned long long);
}

int pie_top_logprobs(const float *logprobs, int rows, int V, int n, const int32_t *tokens, const int32_t *count, int32_t *out_ids, float *out_vals,
                     void *workspace, void *stream) {
    if (int rc = top_logprobs_check("pie_top_logprobs", rows, V, n, true, logprobs, tokens, count, out_ids, out_vals, workspace)) return rc;
    return top_logprobs_launch(logprobs, rows, V, n, tokens, count, out_ids, out_vals, workspace, (hipStream_t)stream);
}

}  // extern "C"
