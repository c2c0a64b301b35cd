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
// pie_spec_verify_sampled, 3 launches under the greedy sampler, 9 with a sampler (10 with an XTC record):
//   1. k_logits_stats and k_logits_finish over every row (logits_tail_rows_launch): all log-probabilities and the rows' argmaxes;
//   2. k_spec_fill_rows, one workgroup: the call's first stream position c = counter[0], read on the device, and one pie_row_tail per row
//      with calls = c + r (and the shared XTC record once per row), in the workspace;
//   3. pie_sample_rows(_xtc)'s launches (sample_rows_launch): row r drawn as the one-row pie_sample call number c + r of the seed;
//   4. k_spec_accept_sampled, ONE thread: the accepted run against the drawn tokens, the outputs, counter = {c + n, 0} and -- for the
//      decoder -- the device-side state, through the functions k_spec_accept ends in.
// pie_decoder_spec_step_tail puts k_spec_edit_rows in front: one workgroup per row applies the decoder's repetition penalty over the row's
// own window (ids_by_pos below the offset, the fed token at it, the drafts behind it) and its logit bias (tail.hpp's phases).
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

// The accepted drafts: the longest run draft[i] == the token row i chose; an id outside [0, V) ends it.  At most rows - 1 comparisons.
__device__ __forceinline__ int spec_count_accepted(const int *draft, const int *tok, int rows, int V) {
    int n = 0;
    while (n < rows - 1) {
        const int d = draft[n];
        if (d < 0 || d >= V || d != tok[n]) break;
        ++n;
    }
    return n;
}

// What the one writer of a verify leaves: the tokens, their number and -- for the decoder -- the device-side state (speculative.hpp).
__device__ __forceinline__ void spec_commit(const SpecState &s, const int *tok, int rows, int n_acc, int *out_tokens, int *out_n) {
    for (int i = 0; i < rows; ++i) out_tokens[i] = i <= n_acc ? tok[i] : -1;
    const int n = n_acc + 1, last = tok[n_acc];
    *out_n = n;
    if (!s.state) return;
    const int o = s.state->pos - rows;  // the pass and its tail advanced the position over every row
    for (int i = 0; i < n; ++i) {       // the token row i chose occupies position o + 1 + i
        const int p = o + 1 + i;
        if (s.history && p >= 0 && p < s.hist_cap) s.history[p] = tok[i];
        if (s.seq_ids && p >= 0 && p < s.seq_cap) s.seq_ids[p] = tok[i];
        if (s.ids_by_pos && p >= 0 && p < s.ids_cap) s.ids_by_pos[p] = tok[i];
    }
    if (s.seq_ids && o >= 0 && o < s.seq_cap) s.seq_ids[o] = s.fed[0];
    if (s.seq_len) *s.seq_len = o + n + 1;
    if (s.token_out) *s.token_out = last;
    s.state->token = last;
    s.state->pos = o + n;
}

template <class T>
__global__ void __launch_bounds__(256) k_spec_accept(const SpecArgs a) {
    __shared__ int s_acc;
    if (threadIdx.x == 0) s_acc = spec_count_accepted(a.draft, a.tok, a.rows, a.V);
    __syncthreads();
    const int n_acc = s_acc, r = blockIdx.y;
    if (r > n_acc) return;  // block-uniform: a row behind the accepted run is not written
    if (a.logprobs) logits_write_logprobs<T>(a.logits + (size_t)r * a.V, a.V, a.lse[r], a.logprobs + (size_t)r * a.V);
    if (r != 0 || blockIdx.x != 0 || threadIdx.x != 0) return;
    spec_commit(a.s, a.tok, a.rows, n_acc, a.out_tokens, a.out_n);
}

// ---------------------------------------------------------------- the verify under a sampler
// pie_spec_verify_sampled's workspace: the tail's partials | the rows' tokens | the call's first stream position | one pie_row_tail and one
// pie_xtc per row | pie_sample_rows' workspace (the part that has to be zeroed once).
struct SpecSampledLayout {
    size_t tok, base, table, xtc, smp, bytes;
    SpecSampledLayout(int rows, int V) {
        tok = sizeof(LogitStat) * TAIL_STAT_TILES * (size_t)rows;
        base = tok + sizeof(int) * SPEC_MAX_ROWS;
        table = base + 16;
        xtc = table + sizeof(pie_row_tail) * SPEC_MAX_ROWS;
        smp = (xtc + sizeof(pie_xtc) * SPEC_MAX_ROWS + 15) & ~(size_t)15;
        bytes = smp + pie_sample_workspace_bytes(rows, V);
    }
};

struct SpecFillArgs {
    int rows, mode, k;
    float inv_temp, thr;
    unsigned long long seed;
    const unsigned long long *counter;
    const pie_xtc *xtc;  // nullable: the one record every row shares
    unsigned long long *base;
    pie_row_tail *table;
    pie_xtc *xtc_rows;
    unsigned long long *smp_ws;  // pie_sample_rows' workspace, row stride smp_row_words 64-bit words
    size_t smp_row_words;
};

// Row r draws at stream position counter[0] + r: the position a plain loop's draw number r from here would have.  The position is device
// memory (a replayed step advances it without the host), so the records are made here and not by the caller.
__global__ void __launch_bounds__(SPEC_MAX_ROWS) k_spec_fill_rows(const SpecFillArgs a) {
    const int r = threadIdx.x;
    if (r >= a.rows) return;
    const unsigned long long c = a.counter[0];
    if (r == 0) *a.base = c;
    pie_row_tail t = {};
    t.mode = a.mode, t.inv_temp = a.inv_temp, t.thr = a.thr, t.k = a.k, t.seed = a.seed, t.calls = c + (unsigned long long)r;
    t.penalty = 1.0f, t.context_size = 1;
    a.table[r] = t;
    if (a.xtc) a.xtc_rows[r] = *a.xtc;
    // The workspace's parts lie where the call's row count puts them, so a row's header may hold what a pass of another size left there:
    // the two words the sampler expects to be zero are zeroed here, in front of its launches.
    unsigned long long *hdr = a.smp_ws + (size_t)r * a.smp_row_words;
    hdr[SMP_WS_MAXKEY_WORD] = 0ull, hdr[SMP_WS_XTC_WORD] = 0ull;
}

struct SpecSampledArgs {
    int rows, V;
    const int *draft;  // [rows - 1]
    const int *tok;    // [rows]: the rows' drawn tokens (their argmaxes under the greedy sampler)
    int *out_tokens, *out_n;
    const unsigned long long *base;  // the call's first stream position
    unsigned long long *counter;     // nullable (the greedy sampler): {base + n, 0} afterwards
    SpecState s;
};

// The log-probabilities of every row are already written (the draws read them): one thread does what is left.
__global__ void k_spec_accept_sampled(const SpecSampledArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int n_acc = spec_count_accepted(a.draft, a.tok, a.rows, a.V);
    spec_commit(a.s, a.tok, a.rows, n_acc, a.out_tokens, a.out_n);
    if (a.counter) a.counter[0] = *a.base + (unsigned long long)(n_acc + 1), a.counter[1] = 0ull;  // the rejected rows' positions are not consumed
}

// pie_decoder_spec_step_tail's edit: workgroup r is row r of the block, at position o + r, o = state->pos - rows (the pass has run).
struct SpecEditArgs {
    u16 *logits;
    int V, rows;
    float penalty;
    int context;  // 1..PEN_MAX_IDS with a penalty
    int *ids_by_pos;
    int ids_cap;
    const DecState *state;
    const int *fed, *draft;
    BiasArgs b;
};

// Row window: this thread's entry of the positions max(0, o + r + 1 - context) .. o + r, -1 beyond them: ids_by_pos below o, the fed token
// at o -- recorded there, as the step's tail records its input (every row that sees o stores the same value; no row reads it back) -- and
// draft[q - o - 1] behind it (q <= o + r: an index below rows - 1).  Every position is checked against ids_cap, as step_window_id's are.
__device__ __forceinline__ int spec_window_id(const SpecEditArgs &a, int r) {
    const int t = threadIdx.x, o = a.state->pos - a.rows, pos = o + r;
    const int lo = pos + 1 - a.context > 0 ? pos + 1 - a.context : 0, n = pos + 1 - lo, p = lo + t;
    if (o < 0 || t >= n || p < 0 || p >= a.ids_cap) return -1;
    if (p > o) return a.draft[p - o - 1];
    if (p == o) return a.ids_by_pos[p] = a.fed[0];
    return a.ids_by_pos[p];
}

template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_spec_edit_rows(const SpecEditArgs a) {
    __shared__ alignas(8) int s_ids[PEN_MAX_IDS];
    const int r = blockIdx.x;
    u16 *logits = a.logits + (size_t)r * a.V;
    if (a.b.penalise) penalise_phase<T>(logits, a.V, a.penalty, spec_window_id(a, r), s_ids);  // block-uniform: launch arguments
    if (a.b.n) bias_phase<T>(logits, a.V, a.b.ids, a.b.bias, a.b.n, 0, s_ids);
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

// pie_spec_verify_sampled's launches behind whatever made the logits (arguments already checked).  mode PIE_SAMPLE_GREEDY (the decoder's
// penalty- or bias-only tails): the rows' tokens are their argmaxes, nothing is drawn and the counter is not touched.
static int spec_verify_sampled_launch(u16 *logits, int rows, int V, int dtype, const int *draft, int mode, double temp, double p, int k, unsigned long long seed,
                                      unsigned long long *counter, const pie_xtc *xtc, int *out_tokens, int *out_n, float *logprobs, void *workspace,
                                      const SpecState &s, hipStream_t st) {
    const SpecSampledLayout lay(rows, V);
    char *ws = (char *)workspace;
    int *tok = (int *)(ws + lay.tok);
    unsigned long long *base = (unsigned long long *)(ws + lay.base);
    if (int rc = logits_tail_rows_launch(dtype, logits, V, rows, (LogitStat *)ws, logprobs, tok, st)) return rc;
    const bool draws = mode != PIE_SAMPLE_GREEDY;
    if (draws) {
        SpecFillArgs f = {};
        f.rows = rows, f.mode = mode, f.seed = seed, f.counter = counter, f.xtc = xtc, f.base = base;
        f.table = (pie_row_tail *)(ws + lay.table), f.xtc_rows = (pie_xtc *)(ws + lay.xtc);
        f.smp_ws = (unsigned long long *)(ws + lay.smp), f.smp_row_words = pie_sample_workspace_bytes(1, V) / sizeof(unsigned long long);
        sample_derive(mode, temp, p, k, &f.inv_temp, &f.thr, &f.k);
        hipLaunchKernelGGL(k_spec_fill_rows, dim3(1), dim3(SPEC_MAX_ROWS), 0, st, f);
        PIE_LAUNCH_CHECK();
        if (int rc = sample_rows_launch(logprobs, rows, V, f.table, ws + lay.smp, tok, nullptr, nullptr, st, SampleXtc{xtc ? f.xtc_rows : nullptr, nullptr})) return rc;
    }
    const SpecSampledArgs a = {rows, V, draft, tok, out_tokens, out_n, base, draws ? counter : nullptr, s};
    hipLaunchKernelGGL(k_spec_accept_sampled, dim3(1), dim3(64), 0, st, a);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
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

size_t pie_spec_verify_sampled_workspace_bytes(int rows, int V) {
    if (rows < 2 || rows > SPEC_MAX_ROWS || pie_sample_workspace_bytes(rows, V) == 0) return 0;
    return SpecSampledLayout(rows, V).bytes;
}

int pie_spec_verify_sampled(const void *logits, int rows, int V, int dtype, const int32_t *draft, int mode, double temp, double p, int k, unsigned long long seed,
                            unsigned long long *counter, const pie_xtc *xtc, int32_t *out_tokens, int32_t *out_n, float *logprobs, void *workspace, void *stream) {
    PIE_REQUIRE(logits && draft && counter && out_tokens && out_n && logprobs && workspace, PIE_E_ARG, "pie_spec_verify_sampled: null pointer");
    PIE_REQUIRE(mode != PIE_SAMPLE_GREEDY, PIE_E_ARG, "pie_spec_verify_sampled: the greedy sampler draws nothing (use pie_spec_verify)");
    PIE_REQUIRE(rows >= 2 && rows <= SPEC_MAX_ROWS && V >= 1, PIE_E_SHAPE, "pie_spec_verify_sampled: need 2 <= rows <= 32 and V >= 1");
    PIE_REQUIRE(pie_aligned(logits, 2) && pie_aligned(draft, 4) && pie_aligned(out_tokens, 4) && pie_aligned(out_n, 4) && pie_aligned(logprobs, 4) && pie_aligned(xtc, 4),
                PIE_E_ALIGN, "pie_spec_verify_sampled: logits need 2-byte, the draft, the XTC record and the outputs 4-byte alignment");
    PIE_REQUIRE(pie_aligned(counter, 8), PIE_E_ALIGN, "pie_spec_verify_sampled: the counter needs 8-byte alignment");
    PIE_REQUIRE(pie_aligned(workspace, 16), PIE_E_ALIGN, "pie_spec_verify_sampled: workspace needs 16-byte alignment");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, "pie_spec_verify_sampled: dtype must be PIE_BF16 or PIE_F16");
    if (int rc = sample_check("pie_spec_verify_sampled", V, mode, temp, p, k, workspace)) return rc;
    return spec_verify_sampled_launch((u16 *)const_cast<void *>(logits), rows, V, dtype, draft, mode, temp, p, k, seed, counter, xtc, out_tokens, out_n, logprobs,
                                      workspace, SpecState(), (hipStream_t)stream);
}

// workspace: the logits block [rows, vocab] T | the pass's input ids [32] | pie_spec_verify's workspace
size_t pie_decoder_spec_workspace_bytes(const pie_decoder *d, int rows) {
    if (!d || rows < 2 || rows > SPEC_MAX_ROWS) return 0;
    return align16((size_t)rows * d->cfg.vocab * 2) + align16(sizeof(int) * SPEC_MAX_ROWS) + spec_verify_workspace_bytes(rows);
}

// workspace: the logits block [rows, vocab] T | the pass's input ids [32] | pie_spec_verify_sampled's workspace
size_t pie_decoder_spec_tail_workspace_bytes(const pie_decoder *d, int rows) {
    if (!d || rows < 2 || rows > SPEC_MAX_ROWS || pie_sample_workspace_bytes(rows, d->cfg.vocab) == 0) return 0;
    return align16((size_t)rows * d->cfg.vocab * 2) + align16(sizeof(int) * SPEC_MAX_ROWS) + SpecSampledLayout(rows, d->cfg.vocab).bytes;
}

}  // extern "C"

namespace {

// What the two pie_decoder_spec_step* entries share: the entry's refusals -- with_tail: which parts of the step's tail the pass admits is
// StepTail's answer (decoder.hpp) --, the shape and alignment checks, the workspace's carve-up (the logits block at its head, then s->fed,
// then *verify_ws), the gather of the input rows, the SpecState fill and the many-row pass itself, raw logits on every row.
int spec_prologue(const char *entry, bool with_tail, pie_decoder *d, const int32_t *draft_ids, int n_draft, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows,
                  void *workspace, int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream, SpecState *s, void **verify_ws) {
    const std::string who = std::string(entry) + ": ";
    PIE_REQUIRE(d && draft_ids && out_tokens && out_n && (logprobs_rows || !with_tail) && workspace, PIE_E_ARG, who + "null pointer");
    PIE_REQUIRE(!d->tp(), PIE_E_STATE, who + "not available on a tensor-parallel shard");
    PIE_REQUIRE(!d->kv_quant && !d->ring, PIE_E_STATE, who + "not available on a quantized or rotating KV cache");
    PIE_REQUIRE(!d->kv_i8, PIE_E_STATE, who + "not available on int8 KV pages");
    const StepTail &t = d->tail;
    if (!with_tail) {
        PIE_REQUIRE(!t.configured() && !d->prompt.n, PIE_E_STATE,
                    who + "speculation is greedy and raw: no sampler, penalty, mask, bias, top-logprobs, counts or prompt scoring may be set");
        PIE_REQUIRE(!t.xtc.on(), PIE_E_STATE, who + "speculation is greedy: no XTC record may be set");
    } else {
        const char *part = t.spec_tail_refused();
        PIE_REQUIRE(!part, PIE_E_STATE, who + "not available with " + part);
        PIE_REQUIRE(!d->prompt.n, PIE_E_STATE, who + "not available with prompt scoring");
        PIE_REQUIRE(t.spec_tail_admitted(), PIE_E_STATE,
                    who + "no sampler, XTC record, repetition penalty or logit bias is set (the greedy and raw pass is pie_decoder_spec_step)");
    }
    const int rows = n_draft + 1, V = d->cfg.vocab;
    PIE_REQUIRE(n_draft >= 1 && rows >= prefill_min_rows(), PIE_E_SHAPE, who + "fewer rows than the many-row pass takes (run a plain step)");
    PIE_REQUIRE(rows <= SPEC_MAX_ROWS, PIE_E_SHAPE, who + "at most 31 drafts");
    PIE_REQUIRE(seq_cap >= 0 && (seq_ids || seq_cap == 0), PIE_E_ARG, who + "bad sequence buffer");
    PIE_REQUIRE(pie_aligned(draft_ids, 4) && pie_aligned(out_tokens, 4) && pie_aligned(out_n, 4) && pie_aligned(logprobs_rows, 4) && pie_aligned(seq_ids, 4) &&
                    pie_aligned(seq_len, 4), PIE_E_ALIGN, who + "4-byte alignment required");
    PIE_REQUIRE(pie_aligned(workspace, 16), PIE_E_ALIGN, who + "workspace needs 16-byte alignment");
    PIE_REQUIRE(!with_tail || pie_sample_workspace_bytes(rows, V) != 0, PIE_E_SHAPE, who + "the vocabulary is larger than the sampler takes (524288)");
    int *fed = (int *)((char *)workspace + align16((size_t)rows * V * 2));
    *verify_ws = (char *)fed + align16(sizeof(int) * SPEC_MAX_ROWS);
    PIE_REQUIRE(d->glob_set && d->kv_set && d->out_set, PIE_E_STATE, "pie_decoder: set_globals, set_kv and bind_outputs must be called before stepping");
    hipLaunchKernelGGL(k_spec_gather, dim3(1), dim3(SPEC_MAX_ROWS), 0, (hipStream_t)stream, (const DecState *)d->state, draft_ids, n_draft, d->embed_vocab(), fed);
    PIE_LAUNCH_CHECK();
    s->state = d->state, s->history = d->history, s->hist_cap = d->hist_cap, s->fed = fed;
    s->seq_ids = seq_ids, s->seq_cap = seq_cap, s->seq_len = seq_len, s->token_out = d->token_out;
    // Raw logits on every row: logits_all != nullptr makes the pass's own last-row tail raw and greedy (pie_decoder::tail_raw), which leaves
    // pos = o + rows; a configured sampler draws nothing there and its counter stays where it is.
    return pie_decoder_prefill(d, fed, rows, workspace, stream);
}

}  // namespace

extern "C" {

int pie_decoder_spec_step(pie_decoder *d, const int32_t *draft_ids, int n_draft, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows, void *workspace,
                          int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream) {
    SpecState s;
    void *verify_ws;
    if (int rc = spec_prologue("pie_decoder_spec_step", false, d, draft_ids, n_draft, out_tokens, out_n, logprobs_rows, workspace, seq_ids, seq_cap, seq_len, stream, &s, &verify_ws)) return rc;
    return spec_verify_launch((const u16 *)workspace, n_draft + 1, d->cfg.vocab, d->cfg.dtype, draft_ids, out_tokens, out_n, logprobs_rows, verify_ws, s, (hipStream_t)stream);
}

int pie_decoder_spec_step_tail(pie_decoder *d, const int32_t *draft_ids, int n_draft, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows, void *workspace,
                               int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream) {
    SpecState s;
    void *verify_ws;
    if (int rc = spec_prologue("pie_decoder_spec_step_tail", true, d, draft_ids, n_draft, out_tokens, out_n, logprobs_rows, workspace, seq_ids, seq_cap, seq_len, stream, &s, &verify_ws)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const pie_decoder_config &c = d->cfg;
    const StepTail &t = d->tail;
    const int rows = n_draft + 1;
    if (t.penalty.on() || t.bias.on()) {  // the rows' edits, in the step tail's order: penalty, then bias
        SpecEditArgs e = {};
        e.logits = (u16 *)workspace, e.V = c.vocab, e.rows = rows, e.penalty = (float)t.penalty.value, e.context = t.penalty.context, e.ids_by_pos = t.penalty.ids_by_pos, e.ids_cap = t.penalty.ids_cap;
        e.state = d->state, e.fed = s.fed, e.draft = draft_ids;
        e.b = BiasArgs{t.bias.ids, t.bias.vals, t.bias.n, t.penalty.on()};
        if (int rc = launch_for_dtype(c.dtype, "spec edit:", [&](auto ty) { hipLaunchKernelGGL(k_spec_edit_rows<decltype(ty)>, dim3((unsigned)rows), dim3(PEN_MAX_IDS), 0, st, e); }))
            return rc;
    }
    if (t.penalty.on()) s.ids_by_pos = t.penalty.ids_by_pos, s.ids_cap = t.penalty.ids_cap;
    const StepTail::Sampler &m = t.sampler;
    return spec_verify_sampled_launch((u16 *)workspace, rows, c.vocab, c.dtype, draft_ids, m.mode, m.temp, m.p, m.k, m.seed, m.counter, m.on() ? t.xtc.record : nullptr, out_tokens, out_n,
                                      logprobs_rows, verify_ws, s, st);
}

}  // extern "C"
