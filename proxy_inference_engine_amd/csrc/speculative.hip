// speculative.hip -- greedy speculative decoding: the prompt-lookup drafter, the verify of a block of logits against a
// draft, and the decoder entry that forwards [token, drafts] through the single-sequence many-row pass and accepts the longest agreeing run.
//
// pie_ngram_draft, 2 launches, deterministic (no atomics, nothing depends on arrival order):
//   1. k_ngram_search over a grid sized from `cap` (one workgroup per 2048 ids, at most 1024, grid-stride beyond): a thread takes END
//      positions e of candidate matches.  A match of length n that ends at e -- ids[e - n : e] == ids[len - n : len] -- contains the
//      matches of every shorter length ending there, so one backwards comparison of at most ngram_max ids gives e's longest match, and
//      "the largest start of the largest n" is the largest key (length << 27 | e): a max reduction, one partial per workgroup;
//   2. k_ngram_pick, one workgroup: the maximum of the partials, then ONE thread copies k ids from e on, reading its own draft once the
//      copy runs past the sequence's end (LZ77's overlapped copy: a period-3 tail drafts k ids, not 3).
// pie_spec_verify, 3 launches:
//   1. k_logits_stats over (TAIL_STAT_TILES, rows): the tail's own per-tile partials (tail.hpp);
//   2. k_spec_merge, one workgroup per row: logits_merge_partials -- the function k_logits_finish ends its merge in -- into the row's
//      greedy token and log-sum-exp;
//   3. k_spec_accept over (TAIL_FINISH_BLOCKS, rows): every workgroup counts the accepted drafts from the rows' tokens (at most 31
//      comparisons); a row behind them leaves at once, the others write their slice of the log-probabilities as k_logits_finish does;
//      workgroup (0, 0) writes the tokens, their number and -- for the decoder -- the device-side state.
#include "speculative.hpp"

#include "decoder.hpp"
#include "tail.hpp"

namespace {

constexpr int NGRAM_T = 256, NGRAM_MAX_WGS = 1024, NGRAM_IDS_PER_WG = 2048;

__device__ __forceinline__ int clamp_len(const int *len, int cap) {
    const int L = *len;
    return L < 0 ? 0 : (L > cap ? cap : L);  // `len` is device memory: the search never reads beyond the `cap` ids the caller vouches for
}

// The longest match that ends at e (exclusive), 1 <= e <= L - 1: how many ids before e equal the ids before L, at most nmax and at most e.
__device__ __forceinline__ int match_len(const int *ids, const int *suffix, int e, int nmax) {
    int n = 0;
    bool run = true;
#pragma unroll
    for (int j = 0; j < SPEC_MAX_NGRAM; ++j) {  // suffix[j] = ids[L - 1 - j]; unrolled: the suffix stays in registers
        run = run && j < nmax && j < e && ids[e - 1 - j] == suffix[j];
        n += run ? 1 : 0;
    }
    return n;
}

__global__ void __launch_bounds__(NGRAM_T) k_ngram_search(const int *ids, const int *len, int cap, int nmax, int nmin, unsigned *partials) {
    __shared__ unsigned s_best[NGRAM_T / 64];
    const int L = clamp_len(len, cap);
    int suffix[SPEC_MAX_NGRAM];
#pragma unroll
    for (int j = 0; j < SPEC_MAX_NGRAM; ++j) suffix[j] = j < L ? ids[L - 1 - j] : -1;
    unsigned best = 0u;  // 0: no match (a real key has a length >= 1 in its top bits)
    for (int e = 1 + (int)(blockIdx.x * NGRAM_T + threadIdx.x); e <= L - 1; e += (int)(gridDim.x * NGRAM_T)) {
        const int n = match_len(ids, suffix, e, nmax);
        if (n >= nmin) best = max(best, ((unsigned)n << 27) | (unsigned)e);  // ascending e per thread: max keeps the longest, then the latest
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, o, 64));
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = max(max(s_best[0], s_best[1]), max(s_best[2], s_best[3]));
}

__global__ void __launch_bounds__(NGRAM_T) k_ngram_pick(const int *ids, const int *len, int cap, const unsigned *partials, int n_partials, int k,
                                                        int *out_ids, int *out_count) {
    __shared__ unsigned s_best[NGRAM_T / 64];
    __shared__ int s_draft[SPEC_MAX_ROWS];
    unsigned best = 0u;
    for (int i = threadIdx.x; i < n_partials; i += NGRAM_T) best = max(best, partials[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, o, 64));
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    best = max(max(s_best[0], s_best[1]), max(s_best[2], s_best[3]));
    if (best == 0u) {  // no match for any n (or len <= ngram_min): out_ids keeps its contents
        *out_count = 0;
        return;
    }
    const int L = clamp_len(len, cap), e = (int)(best & ((1u << 27) - 1u));  // 1 <= e <= L - 1
    for (int i = 0; i < k; ++i) {  // draft[i] = (ids ++ draft)[e + i]; e + i - L < i: only ids this thread has already copied
        const int src = e + i;
        const int v = src < L ? ids[src] : s_draft[src - L];
        s_draft[i] = v, out_ids[i] = v;
    }
    *out_count = k;
}

struct SpecLayout {  // pie_spec_verify's workspace: the partials, then the rows' tokens and log-sum-exps
    size_t tok, lse, bytes;
    explicit SpecLayout(int rows) {
        tok = sizeof(LogitStat) * TAIL_STAT_TILES * (size_t)rows;
        lse = tok + sizeof(int) * SPEC_MAX_ROWS;
        bytes = lse + sizeof(float) * SPEC_MAX_ROWS;
    }
};

__global__ void __launch_bounds__(256) k_spec_merge(const LogitStat *stats, int *tok, float *lse) {
    int t;
    const float v = logits_merge_partials(stats + (size_t)blockIdx.x * TAIL_STAT_TILES, TAIL_STAT_TILES, t);
    if (threadIdx.x == 0) tok[blockIdx.x] = t, lse[blockIdx.x] = v;
}

struct SpecArgs {
    const u16 *logits;
    int rows, V;
    const int *draft;  // [rows - 1]
    const int *tok;    // [rows]: the rows' greedy tokens
    const float *lse;  // [rows]
    int *out_tokens, *out_n;
    float *logprobs;   // nullable
    SpecState s;
};

template <class T>
__global__ void __launch_bounds__(256) k_spec_accept(const SpecArgs a) {
    __shared__ int s_acc;
    if (threadIdx.x == 0) {  // the accepted drafts: the longest run draft[i] == the token row i chose; an id outside [0, V) ends it
        int n = 0;
        while (n < a.rows - 1) {
            const int d = a.draft[n];
            if (d < 0 || d >= a.V || d != a.tok[n]) break;
            ++n;
        }
        s_acc = n;
    }
    __syncthreads();
    const int n_acc = s_acc, r = blockIdx.y;
    if (r > n_acc) return;  // block-uniform: a row behind the accepted run is not written
    if (a.logprobs) logits_write_logprobs<T>(a.logits + (size_t)r * a.V, a.V, a.lse[r], a.logprobs + (size_t)r * a.V);
    if (r != 0 || blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int i = 0; i < a.rows; ++i) a.out_tokens[i] = i <= n_acc ? a.tok[i] : -1;
    const int n = n_acc + 1, last = a.tok[n_acc];
    *a.out_n = n;
    const SpecState &s = a.s;
    if (!s.state) return;
    const int o = s.state->pos - a.rows;  // the pass and its tail advanced the position over every row
    for (int i = 0; i < n; ++i) {         // the token row i chose occupies position o + 1 + i
        const int p = o + 1 + i;
        if (s.history && p >= 0 && p < s.hist_cap) s.history[p] = a.tok[i];
        if (s.seq_ids && p >= 0 && p < s.seq_cap) s.seq_ids[p] = a.tok[i];
    }
    if (s.seq_ids && o >= 0 && o < s.seq_cap) s.seq_ids[o] = s.fed[0];
    if (s.seq_len) *s.seq_len = o + n + 1;
    if (s.token_out) *s.token_out = last;
    s.state->token = last;
    s.state->pos = o + n;
}

// pie_decoder_spec_step's input rows: fed[0] = the device-side token, fed[1 + i] = draft[i]; an id the embedding could not index is fed as
// id 0 (the verify reads the caller's draft, where such an id ends the accepted run: the row's result is never used).
__global__ void k_spec_gather(const DecState *state, const int *draft, int m, int vocab, int *fed) {
    const int i = threadIdx.x;
    if (i > m) return;
    const int id = i == 0 ? state->token : draft[i - 1];
    fed[i] = id >= 0 && id < vocab ? id : 0;
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

size_t spec_verify_workspace_bytes(int rows) { return rows < 2 || rows > SPEC_MAX_ROWS ? 0 : SpecLayout(rows).bytes; }

int spec_verify_launch(const u16 *logits, int rows, int V, int dtype, const int *draft, int *out_tokens, int *out_n, float *logprobs, void *workspace,
                       const SpecState &s, hipStream_t st) {
    const SpecLayout lay(rows);
    LogitStat *stats = (LogitStat *)workspace;
    int *tok = (int *)((char *)workspace + lay.tok);
    float *lse = (float *)((char *)workspace + lay.lse);
    const SpecArgs a = {logits, rows, V, draft, tok, lse, out_tokens, out_n, logprobs, s};
    return launch_for_dtype(dtype, "spec verify:", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_logits_stats<T>, dim3(TAIL_STAT_TILES, (unsigned)rows), dim3(256), 0, st, logits, V, stats);
        hipLaunchKernelGGL(k_spec_merge, dim3((unsigned)rows), dim3(256), 0, st, (const LogitStat *)stats, tok, lse);
        hipLaunchKernelGGL(k_spec_accept<T>, dim3(TAIL_FINISH_BLOCKS, (unsigned)rows), dim3(256), 0, st, a);
    });
}

extern "C" {

size_t pie_ngram_draft_workspace_bytes(void) { return sizeof(unsigned) * NGRAM_MAX_WGS; }

int pie_ngram_draft(const int32_t *ids, const int32_t *len, int cap, int ngram_max, int ngram_min, int k, int32_t *out_ids, int32_t *out_count,
                    void *workspace, void *stream) {
    PIE_REQUIRE(ngram_min >= 1 && ngram_min <= ngram_max && ngram_max <= SPEC_MAX_NGRAM, PIE_E_ARG, "pie_ngram_draft: need 1 <= ngram_min <= ngram_max <= 8");
    PIE_REQUIRE(k >= 1 && k <= SPEC_MAX_ROWS - 1, PIE_E_ARG, "pie_ngram_draft: k must be 1..31");
    PIE_REQUIRE(ids && len && out_ids && out_count && workspace, PIE_E_ARG, "pie_ngram_draft: null pointer");
    PIE_REQUIRE(cap >= 1 && cap <= SPEC_MAX_IDS, PIE_E_SHAPE, "pie_ngram_draft: cap must be 1..2^27");
    PIE_REQUIRE(pie_aligned(ids, 4) && pie_aligned(len, 4) && pie_aligned(out_ids, 4) && pie_aligned(out_count, 4) && pie_aligned(workspace, 4), PIE_E_ALIGN,
                "pie_ngram_draft: 4-byte alignment required");
    hipStream_t st = (hipStream_t)stream;
    const int wgs = (cap + NGRAM_IDS_PER_WG - 1) / NGRAM_IDS_PER_WG;
    const int G = wgs < 1 ? 1 : (wgs > NGRAM_MAX_WGS ? NGRAM_MAX_WGS : wgs);
    hipLaunchKernelGGL(k_ngram_search, dim3((unsigned)G), dim3(NGRAM_T), 0, st, ids, len, cap, ngram_max, ngram_min, (unsigned *)workspace);
    PIE_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ngram_pick, dim3(1), dim3(NGRAM_T), 0, st, ids, len, cap, (const unsigned *)workspace, G, k, out_ids, out_count);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

size_t pie_spec_verify_workspace_bytes(int rows) { return spec_verify_workspace_bytes(rows); }

int pie_spec_verify(const void *logits, int rows, int V, int dtype, const int32_t *draft, int32_t *out_tokens, int32_t *out_n, float *logprobs,
                    void *workspace, void *stream) {
    PIE_REQUIRE(logits && draft && out_tokens && out_n && workspace, PIE_E_ARG, "pie_spec_verify: null pointer");
    PIE_REQUIRE(rows >= 2 && rows <= SPEC_MAX_ROWS && V >= 1, PIE_E_SHAPE, "pie_spec_verify: need 2 <= rows <= 32 and V >= 1");
    PIE_REQUIRE(pie_aligned(logits, 2) && pie_aligned(draft, 4) && pie_aligned(out_tokens, 4) && pie_aligned(out_n, 4) && pie_aligned(logprobs, 4), PIE_E_ALIGN,
                "pie_spec_verify: logits need 2-byte, the draft and the outputs 4-byte alignment");
    PIE_REQUIRE(pie_aligned(workspace, 16), PIE_E_ALIGN, "pie_spec_verify: workspace needs 16-byte alignment");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_spec_verify: dtype must be PIE_BF16 or PIE_F16");
    return spec_verify_launch((const u16 *)logits, rows, V, dtype, draft, out_tokens, out_n, logprobs, workspace, SpecState(), (hipStream_t)stream);
}

// workspace: the logits block [rows, vocab] T | the pass's input ids [32] | pie_spec_verify's workspace
size_t pie_decoder_spec_workspace_bytes(const pie_decoder *d, int rows) {
    if (!d || rows < 2 || rows > SPEC_MAX_ROWS) return 0;
    return align16((size_t)rows * d->cfg.vocab * 2) + align16(sizeof(int) * SPEC_MAX_ROWS) + spec_verify_workspace_bytes(rows);
}

int pie_decoder_spec_step(pie_decoder *d, const int32_t *draft_ids, int n_draft, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows, void *workspace,
                          int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream) {
    PIE_REQUIRE(d && draft_ids && out_tokens && out_n && workspace, PIE_E_ARG, "pie_decoder_spec_step: null pointer");
    PIE_REQUIRE(!d->tp(), PIE_E_STATE, "pie_decoder_spec_step: not available on a tensor-parallel shard");
    PIE_REQUIRE(!d->kv_quant && !d->ring, PIE_E_STATE, "pie_decoder_spec_step: not available on a quantized or rotating KV cache");
    PIE_REQUIRE(!d->kv_i8, PIE_E_STATE, "pie_decoder_spec_step: not available on int8 KV pages");
    PIE_REQUIRE(!d->tail_configured() && !d->prompt.n, PIE_E_STATE,
                "pie_decoder_spec_step: speculation is greedy and raw: no sampler, penalty, mask, bias, top-logprobs, counts or prompt scoring may be set");
    PIE_REQUIRE(!d->xtc_record, PIE_E_STATE, "pie_decoder_spec_step: speculation is greedy: no XTC record may be set");
    const int rows = n_draft + 1;
    PIE_REQUIRE(n_draft >= 1 && rows >= prefill_min_rows(), PIE_E_SHAPE, "pie_decoder_spec_step: fewer rows than the many-row pass takes (run a plain step)");
    PIE_REQUIRE(rows <= SPEC_MAX_ROWS, PIE_E_SHAPE, "pie_decoder_spec_step: at most 31 drafts");
    PIE_REQUIRE(seq_cap >= 0 && (seq_ids || seq_cap == 0), PIE_E_ARG, "pie_decoder_spec_step: bad sequence buffer");
    PIE_REQUIRE(pie_aligned(draft_ids, 4) && pie_aligned(out_tokens, 4) && pie_aligned(out_n, 4) && pie_aligned(logprobs_rows, 4) && pie_aligned(seq_ids, 4) &&
                    pie_aligned(seq_len, 4), PIE_E_ALIGN, "pie_decoder_spec_step: 4-byte alignment required");
    PIE_REQUIRE(pie_aligned(workspace, 16), PIE_E_ALIGN, "pie_decoder_spec_step: workspace needs 16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    const pie_decoder_config &c = d->cfg;
    u16 *block = (u16 *)workspace;
    int *fed = (int *)((char *)workspace + align16((size_t)rows * c.vocab * 2));
    void *verify_ws = (char *)fed + align16(sizeof(int) * SPEC_MAX_ROWS);
    PIE_REQUIRE(d->glob_set && d->kv_set && d->out_set, PIE_E_STATE, "pie_decoder: set_globals, set_kv and bind_outputs must be called before stepping");
    hipLaunchKernelGGL(k_spec_gather, dim3(1), dim3(SPEC_MAX_ROWS), 0, st, (const DecState *)d->state, draft_ids, n_draft, d->embed_vocab(), fed);
    PIE_LAUNCH_CHECK();
    // raw logits on every row; the pass ends in the greedy tail of its last row, which leaves pos = o + rows
    if (int rc = pie_decoder_prefill(d, fed, rows, block, stream)) return rc;
    SpecState s;
    s.state = d->state, s.history = d->history, s.hist_cap = d->hist_cap, s.fed = fed;
    s.seq_ids = seq_ids, s.seq_cap = seq_cap, s.seq_len = seq_len, s.token_out = d->token_out;
    return spec_verify_launch(block, rows, c.vocab, c.dtype, draft_ids, out_tokens, out_n, logprobs_rows, verify_ws, s, st);
}

}  // extern "C"
