// speculative.hip -- speculative decoding: the prompt-lookup drafter, the six verifies of a block of logits
// against a draft, and the decoder entries that forward [token, drafts] through the single-sequence many-row pass and accept a run of them.
//
// Written once, used by every verify: Carve / SpecPassLayout (speculative.hpp) and verify_head lay the workspaces out;
// spec_greedy_rows (k_logits_stats over (TAIL_STAT_TILES, rows), the tail's own partials, and k_spec_merge, one workgroup per row:
// logits_merge_partials into the row's greedy token and log-sum-exp) or tail.hpp's logits_tail_rows_launch (k_logits_stats and
// k_logits_finish: all log-probabilities and the rows' argmaxes) give the rows' tokens, in 2 launches each; spec_row_record and
// spec_rearm_header make a row's sampler record and re-arm its workspace row; window_span is a row's penalty window; SpecBlock,
// spec_count_accepted and spec_commit are one sequence's block, spec_segment and spec_accept_seq a segment of a batched pass.
//
// pie_ngram_draft(_rows), 2 launches, deterministic (no atomics, nothing depends on arrival order):
//   1. k_ngram_search over a grid sized from `cap` (one workgroup per 2048 ids, at most 1024, grid-stride beyond) x the sequences: a thread
//      takes END positions e of candidate matches.  A match of length n that ends at e -- ids[e - n : e] == ids[len - n : len] -- contains
//      the matches of every shorter length ending there, so one backwards comparison of at most ngram_max ids gives e's longest match, and
//      "the largest start of the largest n" is the largest key (length << 27 | e): a max reduction, one partial per workgroup;
//   2. k_ngram_pick, one workgroup per sequence: the maximum of the partials, then ONE thread copies k ids from e on, reading its own draft
//      once the copy runs past the sequence's end (LZ77's overlapped copy: a period-3 tail drafts k ids, not 3).
// pie_spec_verify, 3 launches:
//   1. spec_greedy_rows (2);
//   2. k_spec_accept over (TAIL_FINISH_BLOCKS, rows): every workgroup counts the accepted drafts from the rows' tokens (at most 31
//      comparisons); a row behind them leaves at once, the others write their slice of the log-probabilities as k_logits_finish does;
//      workgroup (0, 0) commits (1).
// pie_spec_verify_rows, 3 launches: spec_greedy_rows over every row (2); k_spec_accept_rows, one thread per sequence (1).
// pie_spec_verify_sampled, 3 launches under the greedy sampler, 9 with a sampler (10 with an XTC record):
//   1. logits_tail_rows_launch (2);
//   2. k_spec_fill_rows, one workgroup: the call's first stream position c = counter[0], read on the device, and row r's record at
//      calls = c + r (and the shared XTC record once per row), in the workspace (1);
//   3. pie_sample_rows(_xtc)'s launches (sample_rows_launch): row r drawn as the one-row pie_sample call number c + r of the seed (5 or 6);
//   4. k_spec_accept_sampled, ONE thread: the accepted run against the drawn tokens, the commit and counter = {c + n, 0} (1).
//   The greedy sampler leaves 2 and 3 out.  pie_decoder_spec_step_dfa masks 1's partials; its k_spec_accept_dfa moves the automaton.
// pie_spec_verify_draft, 19 launches: speculative sampling over a block a draft MODEL proposed
//   1. logits_tail_rows_launch (2);
//   2. k_spec_draft_fill, one workgroup: c = counter[0] and the records of BOTH filters -- target row r at calls = c + r, the drafter's rows
//      at any position (their draws are discarded) -- and the sampler workspaces' re-armed headers (1);
//   3. sample_rows_launch over the target's log-probabilities with a mask output: the kept sets K of P, and the rows' ordinary draws --
//      the bonus token and the fallback come from them (5); the same over q_logprobs: the kept sets of Q (5);
//   4. k_spec_dist_stats over (ceil(V / 512), 2 rows - 1): a tile's largest kept log-probability and sum of exp((lp - m) * inv_temp), fp64;
//      k_spec_dist_merge, one workgroup per row: the tiles' shares in a fixed order (2);
//   5. k_spec_draft_residual over ceil(V / 512) tiles (x rows - 1 with the residual diagnostic): every workgroup decides the drafts --
//      thread i draft i: P_i(d), Q_i(d), u_i from the Philox block {0xFFFFFFFE, 0, c + i} -- takes n_acc as the first refusal and
//      writes its tile of R_j = log(max(0, P_j - Q_j)), j = n_acc, with a per-tile "has a finite entry" flag (1);
//   6. sample_launch(CATEGORICAL, temp 1) on R_j at {c + j, 0}: pie_sample itself (2);
//   7. k_spec_draft_commit, one workgroup: the accepted drafts, then the residual's token (the row's ordinary draw when no tile had a
//      finite entry, or behind a fully accepted block), through spec_commit; counter = {c + n, 0} (1).
//   No floating-point atomics; every reduction has a fixed order; n_acc stays on the device.
// pie_spec_verify_rows_sampled, 10 launches and a fill (11 with XTC records): pie_spec_verify_sampled's rule per segment of a batched pass
//   1. k_spec_edit_seg_rows over (8, B): workgroup (j, s) applies seat s's repetition penalty -- the window from the seat's ring below
//      the segment's first position and from the pass's own inputs from it on -- and the seat's bias entries to row j of segment s (1);
//   2. logits_tail_rows_launch (2);
//   3. the rows' records filled with the greedy mode, then k_spec_fill_seg_rows, one workgroup per segment: row j's record = the seat's
//      with calls + j (and the seat's XTC record), in the workspace (1 + the fill);
//   4. pie_sample_rows(_xtc)'s launches over the N rows (5 or 6);
//   5. k_spec_commit_rows, one thread per sequence: k_spec_accept_rows' part over the drawn tokens, then the seat's calls and ring (1).
// pie_decoder_spec_step* (spec_step) put k_spec_edit_rows in front of the verify: one workgroup per row applies the decoder's repetition
// penalty over the row's own window (ids_by_pos below the offset, the fed token at it, the drafts behind it) and its logit bias.
#include "speculative.hpp"

#include "decoder.hpp"
#include "tail.hpp"

namespace {

// ---------------------------------------------------------------- the prompt-lookup drafter
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

// blockIdx.y (pie_ngram_draft_rows; 0 for the one-sequence op): the sequence -- its row of ids [B, cap], its len, its row of the partials
__global__ void __launch_bounds__(NGRAM_T) k_ngram_search(const int *ids, const int *len, int cap, int nmax, int nmin, unsigned *partials) {
    __shared__ unsigned s_best[NGRAM_T / 64];
    ids += (size_t)blockIdx.y * cap, len += blockIdx.y, partials += (size_t)blockIdx.y * gridDim.x;
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
    // blockIdx.x: the sequence (pie_ngram_draft_rows; one workgroup for the one-sequence op)
    ids += (size_t)blockIdx.x * cap, len += blockIdx.x, partials += (size_t)blockIdx.x * n_partials, out_ids += (size_t)blockIdx.x * k, out_count += blockIdx.x;
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

// ---------------------------------------------------------------- the parts every verify shares
// The verify head, which every verify's workspace begins with: the tail's partials of `rows` rows (at offset 0), then the rows' tokens in
// `tok_slots` slots, whose offset it returns.
size_t verify_head(Carve &c, int rows, int tok_slots) {
    c.take(sizeof(LogitStat) * TAIL_STAT_TILES * (size_t)rows);
    return c.take(sizeof(int) * (size_t)tok_slots);
}

__global__ void __launch_bounds__(256) k_spec_merge(const LogitStat *stats, int *tok, float *lse) {
    int t;
    const float v = logits_merge_partials(stats + (size_t)blockIdx.x * TAIL_STAT_TILES, TAIL_STAT_TILES, t);
    if (threadIdx.x == 0) tok[blockIdx.x] = t, lse[blockIdx.x] = v;
}

// The rows' greedy tokens and log-sum-exps, the head of both greedy verifies: the tail's partials, then their merge (2 launches).
template <class T>
void spec_greedy_rows(const u16 *logits, int rows, int V, LogitStat *stats, int *tok, float *lse, hipStream_t st) {
    hipLaunchKernelGGL(k_logits_stats<T>, dim3(TAIL_STAT_TILES, (unsigned)rows), dim3(256), 0, st, logits, V, stats);
    hipLaunchKernelGGL(k_spec_merge, dim3((unsigned)rows), dim3(256), 0, st, (const LogitStat *)stats, tok, lse);
}

// Row r of a block (or of a segment) draws as its base record's one-row call number calls + r -- the position a plain loop's draw number r
// from here would have -- with no penalty of its own (an edit launch in front has applied it).  The sampler advances the ROW's calls.
__device__ __forceinline__ pie_row_tail spec_row_record(pie_row_tail base, int r) {
    base.calls += (unsigned long long)r, base.penalty = 1.0f, base.context_size = 1;
    return base;
}

// A workspace's parts lie where the call's row count puts them, so a sampler-workspace row's header may hold what a pass of another size
// left there: the two words the sampler expects to be zero are zeroed in front of its launches.
__device__ __forceinline__ void spec_rearm_header(unsigned long long *row) { row[SMP_WS_MAXKEY_WORD] = 0ull, row[SMP_WS_XTC_WORD] = 0ull; }

// The penalty window of a row at position pos: the n = pos + 1 - lo positions lo .. pos, lo = max(0, pos + 1 - context).  Returns this
// thread's position p = lo + threadIdx.x, which lies inside the window iff threadIdx.x < n.
__device__ __forceinline__ int window_span(int pos, int context, int &n) {
    const int lo = pos + 1 - context > 0 ? pos + 1 - context : 0;
    n = pos + 1 - lo;
    return lo + (int)threadIdx.x;
}

// ---------------------------------------------------------------- one sequence's block: the accepted run and the commit
struct SpecBlock {  // what the three one-sequence verifies are given and leave
    int rows, V;
    const int *draft;  // [rows - 1]
    const int *tok;    // [rows]: the rows' tokens (greedy, or drawn)
    int *out_tokens, *out_n;
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

// ---------------------------------------------------------------- pie_spec_verify
// Both greedy verifies' workspace: the verify head, then the rows' log-sum-exps -- 32 slots for one sequence, one per row for a batched pass
struct SpecGreedyLayout {
    size_t tok, lse, bytes;
    SpecGreedyLayout(int rows, int slots) {
        Carve c;
        tok = verify_head(c, rows, slots);
        lse = c.take(sizeof(float) * (size_t)slots);
        bytes = align16(c.at);
    }
};

struct SpecArgs {
    const u16 *logits;
    SpecBlock b;
    const float *lse;  // [rows]
    float *logprobs;   // nullable
};

template <class T>
__global__ void __launch_bounds__(256) k_spec_accept(const SpecArgs a) {
    __shared__ int s_acc;
    if (threadIdx.x == 0) s_acc = spec_count_accepted(a.b.draft, a.b.tok, a.b.rows, a.b.V);
    __syncthreads();
    const int n_acc = s_acc, r = blockIdx.y;
    if (r > n_acc) return;  // block-uniform: a row behind the accepted run is not written
    if (a.logprobs) logits_write_logprobs<T>(a.logits + (size_t)r * a.b.V, a.b.V, a.lse[r], a.logprobs + (size_t)r * a.b.V);
    if (r != 0 || blockIdx.x != 0 || threadIdx.x != 0) return;
    spec_commit(a.b.s, a.b.tok, a.b.rows, n_acc, a.b.out_tokens, a.b.out_n);
}

// ---------------------------------------------------------------- the segmented verify of a batched pass
struct SpecRowsArgs {
    int N, B, V;
    const int *seg_first;  // [B + 1]
    const int *draft;      // [B, draft_stride]: sequence s's drafts, as many as it has rows behind its first
    int draft_stride;
    const int *tok;        // [N]: the rows' greedy tokens
    int *out_tokens;       // [B, SPEC_SEG_ROWS]
    int *out_n;            // [B]
    int *ids;              // nullable, [B, cap]: the sequences' ids, the drafter's input
    int *len;              // [B]
    int cap;
};

// Segment s of seg_first [B + 1] as every kernel of a batched pass reads it: its first row, and how many rows it has (0: an idle slot).
// seg_first is device memory: the rows are clamped into [0, N] and to 8 before anything is read.
__device__ __forceinline__ int spec_segment(const int *seg_first, int s, int N, int &r0) {
    int r1 = seg_first[s + 1];
    r0 = seg_first[s];
    r0 = r0 < 0 ? 0 : (r0 > N ? N : r0);
    r1 = r1 < r0 ? r0 : (r1 > N ? N : r1);
    return r1 - r0 > SPEC_SEG_ROWS ? SPEC_SEG_ROWS : r1 - r0;
}

// What k_spec_accept_rows does for sequence s, for the kernels that end in it: pie_spec_verify's rule on its own rows (spec_count_accepted,
// at most 7 comparisons), then its tokens behind its ids.  An idle slot (no rows): out_n = 0.  Returns out_n[s] and the segment's first row.
__device__ __forceinline__ int spec_accept_seq(const SpecRowsArgs &a, int s, int &r0) {
    const int rows = spec_segment(a.seg_first, s, a.N, r0);
    int *out = a.out_tokens + (size_t)s * SPEC_SEG_ROWS;
    if (rows == 0) {
        for (int i = 0; i < SPEC_SEG_ROWS; ++i) out[i] = -1;
        a.out_n[s] = 0;
        return 0;
    }
    const int *tok = a.tok + r0;
    // (a row behind the drafts the stride holds has no draft: it ends the run like a refused one)
    const int n_acc = spec_count_accepted(a.draft + (size_t)s * a.draft_stride, tok, rows > a.draft_stride + 1 ? a.draft_stride + 1 : rows, a.V);
    for (int i = 0; i < SPEC_SEG_ROWS; ++i) out[i] = i <= n_acc ? tok[i] : -1;
    a.out_n[s] = n_acc + 1;
    if (!a.ids) return n_acc + 1;
    // ids[s, len - 1] is the token this pass was fed; the chosen tokens follow it, the last of them being the next pass's input
    int L = a.len[s];
    L = L < 0 ? 0 : (L > a.cap ? a.cap : L);
    for (int i = 0; i <= n_acc && L + i < a.cap; ++i) a.ids[(size_t)s * a.cap + L + i] = tok[i];
    a.len[s] = L + n_acc + 1 > a.cap ? a.cap : L + n_acc + 1;
    return n_acc + 1;
}

__global__ void __launch_bounds__(64) k_spec_accept_rows(const SpecRowsArgs a) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.B) return;
    int r0;
    spec_accept_seq(a, s, r0);
}

// pie_decoder_spec_step_batch's input rows: sequence s's first row is its fed token, the rows behind it its drafts; an id the embedding
// could not index is fed as id 0 (the verify reads the caller's draft, where such an id ends the accepted run)
__global__ void __launch_bounds__(64) k_spec_gather_rows(const int *tokens, const int *draft, int draft_stride, const int *seg_first, int B, int N, int vocab,
                                                         int *fed) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= B) return;
    int r0;
    const int rows = spec_segment(seg_first, s, N, r0);
    for (int i = 0; i < rows; ++i) {
        const int id = i == 0 ? tokens[s] : (i - 1 < draft_stride ? draft[(size_t)s * draft_stride + i - 1] : 0);
        fed[r0 + i] = id >= 0 && id < vocab ? id : 0;
    }
}

// ---------------------------------------------------------------- the segmented verify under per-seat tails
// pie_spec_verify_rows_sampled's workspace: the verify head of every row | one pie_row_tail and one pie_xtc per ROW (the seats' records
// expanded over their segments) | pie_sample_rows' workspace (the part that has to be zeroed once).
struct SpecRowsSampledLayout {
    size_t tok, table, xtc, smp, bytes;
    SpecRowsSampledLayout(int n_rows, int V) {
        Carve c;
        tok = verify_head(c, n_rows, n_rows);
        table = c.take16(sizeof(pie_row_tail) * (size_t)n_rows);
        xtc = c.take(sizeof(pie_xtc) * (size_t)n_rows);
        smp = c.take16(pie_sample_workspace_bytes(n_rows, V));
        bytes = c.at;
    }
};

struct SpecSeatsArgs {
    SpecSeats q;  // what the seats own (speculative.hpp): record, ring, bias entries and XTC record s belong to segment s
    u16 *logits;
    int N, B, V;
    const int *seg_first, *fed;
    pie_row_tail *table_rows;  // [N], the workspace's
    pie_xtc *xtc_rows;
    unsigned long long *smp_ws;
    size_t smp_row_words;
};

// the position of segment s's first row: pos0[s], or row_ctx[its first row] - 1
__device__ __forceinline__ int spec_seat_pos0(const SpecSeats &q, int s, int r0) { return q.pos0 ? q.pos0[s] : q.row_ctx[r0] - 1; }

// Segment window: this thread's entry of the window of row j of a segment that starts at pos0 (position pos0 + j), -1 beyond it: the seat's
// ring below pos0, the pass's own inputs fed[0 .. j] from pos0 on.  NOTHING is recorded here, unlike
// ring_window_id: slot (pos0 + j) & 1023 still holds position pos0 + j - 1024, which lies inside row 0's window whenever context_size >=
// 1025 - j, so a row that stored its own input would race with its segment's earlier rows, which run in other workgroups.  The commit
// launch, behind every draw, is the ring's one writer.
__device__ __forceinline__ int seg_window_id(const int *ring, const int *fed, int context, int pos0, int j) {
    context = context < 1 ? 1 : (context > PEN_MAX_IDS ? PEN_MAX_IDS : context);
    int n;  // 1 <= n <= context
    const int p = window_span(pos0 + j, context, n);
    if ((int)threadIdx.x >= n) return -1;
    return p < pos0 ? ring[p & (PEN_MAX_IDS - 1)] : fed[p - pos0];  // p - pos0 <= j
}

// Workgroup (j, s) is row j of segment s: the seat's repetition penalty over the row's own window, then the seat's bias entries
// (tail.hpp's phases).  Every exit and every skipped phase is block-uniform: a launch argument, or a value every thread reads from one
// address that no launch of this sequence has written yet.
template <class T>
__global__ void __launch_bounds__(PEN_MAX_IDS) k_spec_edit_seg_rows(const SpecSeatsArgs a) {
    __shared__ alignas(8) int s_ids[PEN_MAX_IDS];
    const int j = blockIdx.x, s = blockIdx.y;
    int r0;
    if (j >= spec_segment(a.seg_first, s, a.N, r0)) return;
    const SpecSeats &q = a.q;
    const int pos0 = spec_seat_pos0(q, s, r0);
    if (pos0 < 0) return;
    u16 *logits = a.logits + (size_t)(r0 + j) * a.V;
    const float penalty = q.table[s].penalty;
    if (penalty != 1.0f)
        penalise_phase<T>(logits, a.V, penalty, seg_window_id(q.recent + (size_t)s * PEN_MAX_IDS, a.fed + r0, q.table[s].context_size, pos0, j), s_ids);
    if (!q.bias_ids) return;
    const int n = q.bias_n[s];
    bias_phase<T>(logits, a.V, q.bias_ids, q.bias_vals, n < 0 ? 0 : (n > q.bias_cap ? q.bias_cap : n), (size_t)s * q.bias_cap, s_ids);
}

// Thread j of workgroup s: row j of segment s draws with the seat's record at calls_s + j, in the workspace; the seat's own record is read
// only until the commit launch.
__global__ void __launch_bounds__(64) k_spec_fill_seg_rows(const SpecSeatsArgs a) {
    const int j = threadIdx.x, s = blockIdx.x;
    int r0;
    if (j >= spec_segment(a.seg_first, s, a.N, r0)) return;
    a.table_rows[r0 + j] = spec_row_record(a.q.table[s], j);
    if (a.q.xtc) a.xtc_rows[r0 + j] = a.q.xtc[s];
    spec_rearm_header(a.smp_ws + (size_t)(r0 + j) * a.smp_row_words);
}

// Thread s is sequence s, behind every draw: k_spec_accept_rows' part over the drawn tokens, then the seat's state moves by the n tokens
// the pass chose -- calls for a seat that draws (a greedy seat's record is not written), and the ring's slots of the n positions the pass
// has fed for good: its fed token and the n - 1 accepted drafts.  No other slot is written.
__global__ void __launch_bounds__(64) k_spec_commit_rows(const SpecRowsArgs a, const SpecSeats q, const int *fed) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.B) return;
    int r0;
    const int n = spec_accept_seq(a, s, r0);
    if (n == 0) return;
    const int pos0 = spec_seat_pos0(q, s, r0);
    if (pos0 < 0) return;
    if (sample_mode_draws(q.table[s].mode)) q.table[s].calls += (unsigned long long)n;
    for (int i = 0; i < n; ++i) q.recent[(size_t)s * PEN_MAX_IDS + ((pos0 + i) & (PEN_MAX_IDS - 1))] = fed[r0 + i];
}

// ---------------------------------------------------------------- the verify under a sampler
// pie_spec_verify_sampled's workspace: the verify head | the call's first stream position | one pie_row_tail and one pie_xtc per row |
// pie_sample_rows' workspace (the part that has to be zeroed once).
struct SpecSampledLayout {
    size_t tok, base, table, xtc, smp, bytes;
    SpecSampledLayout(int rows, int V) {
        Carve c;
        tok = verify_head(c, rows, SPEC_MAX_ROWS);
        base = c.take(16);
        table = c.take(sizeof(pie_row_tail) * SPEC_MAX_ROWS);
        xtc = c.take(sizeof(pie_xtc) * SPEC_MAX_ROWS);
        smp = c.take16(pie_sample_workspace_bytes(rows, V));
        bytes = c.at;
    }
};

struct SpecFillArgs {
    int rows;
    pie_row_tail record;  // the sampler's, at stream position 0
    const unsigned long long *counter;
    const pie_xtc *xtc;  // nullable: the one record every row shares
    unsigned long long *base;
    pie_row_tail *table;
    pie_xtc *xtc_rows;
    unsigned long long *smp_ws;  // pie_sample_rows' workspace, row stride smp_row_words 64-bit words
    size_t smp_row_words;
};

// Row r draws at stream position counter[0] + r.  The position is device memory (a replayed step advances it without the host), so the
// records are made here and not by the caller.
__global__ void __launch_bounds__(SPEC_MAX_ROWS) k_spec_fill_rows(const SpecFillArgs a) {
    const int r = threadIdx.x;
    if (r >= a.rows) return;
    pie_row_tail t = a.record;
    t.calls = a.counter[0];
    if (r == 0) *a.base = t.calls;
    a.table[r] = spec_row_record(t, r);
    if (a.xtc) a.xtc_rows[r] = *a.xtc;
    spec_rearm_header(a.smp_ws + (size_t)r * a.smp_row_words);
}

struct SpecSampledArgs {
    SpecBlock b;                     // tok: the rows' drawn tokens (their argmaxes under the greedy sampler)
    const unsigned long long *base;  // the call's first stream position
    unsigned long long *counter;     // nullable (the greedy sampler): {base + n, 0} afterwards
};

// The log-probabilities of every row are already written (the draws read them): one thread does what is left.
__device__ __forceinline__ int spec_accept_sampled(const SpecSampledArgs &a) {
    const int n_acc = spec_count_accepted(a.b.draft, a.b.tok, a.b.rows, a.b.V);
    spec_commit(a.b.s, a.b.tok, a.b.rows, n_acc, a.b.out_tokens, a.b.out_n);
    if (a.counter) a.counter[0] = *a.base + (unsigned long long)(n_acc + 1), a.counter[1] = 0ull;  // the rejected rows' positions are not consumed
    return n_acc;
}

__global__ void k_spec_accept_sampled(const SpecSampledArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    spec_accept_sampled(a);
}

// pie_decoder_spec_step_dfa's part of the verify, all of it in the workspace but the decoder's own record, state and arena:
// states [rows] = the automaton's state in front of every row (the walk along the draft), records [rows] = the record once per row,
// masks [rows, mask_words] and mask_on [rows] = what the mask op derives from them and the masked partials read.
struct SpecDfa {
    const pie_row_dfa *record;
    int *state;
    const int *tables;
    int tables_len;
    int *states, *mask_on;
    pie_row_dfa *records;
    unsigned *masks;
    int mask_words;
};

struct SpecDfaLayout {  // pie_decoder_spec_step_dfa's part of the workspace, behind the `head` bytes of pie_decoder_spec_step_tail's
    size_t states, mask_on, records, masks, bytes;
    int mask_words;
    SpecDfaLayout(size_t head, int V) {
        mask_words = (V + 31) / 32;
        Carve c;
        c.take(head);
        states = c.take16(sizeof(int) * SPEC_MAX_ROWS);
        mask_on = c.take(sizeof(int) * SPEC_MAX_ROWS);
        records = c.take(sizeof(pie_row_dfa) * SPEC_MAX_ROWS);
        masks = c.take(sizeof(unsigned) * SPEC_MAX_ROWS * (size_t)mask_words);
        bytes = align16(c.at);
    }
};

// The accept launch under an automaton: what k_spec_accept_sampled leaves, and the decoder's automaton state where out_n configured steps
// would have left it -- the state in front of row n_acc (every draft before it was accepted: the plain loop's state) advanced by that
// row's token, by pie_token_dfa_advance's rule.
__global__ void k_spec_accept_dfa(const SpecSampledArgs a, const SpecDfa f) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int n_acc = spec_accept_sampled(a);
    const pie_row_dfa r = *f.record;
    if (!dfa_armed(r, a.b.V, f.tables_len)) return;
    const int s = f.states[n_acc];
    *f.state = s >= 0 && s < r.n_states ? dfa_next(r, f.tables, a.b.V, s, a.b.tok[n_acc]) : s;
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

// Row window: this thread's entry of the window of row r (position o + r), -1 beyond it: ids_by_pos below o, the fed token
// at o -- recorded there, as the step's tail records its input (every row that sees o stores the same value; no row reads it back) -- and
// draft[q - o - 1] behind it (q <= o + r: an index below rows - 1).  Every position is checked against ids_cap, as step_window_id's are.
__device__ __forceinline__ int spec_window_id(const SpecEditArgs &a, int r) {
    const int o = a.state->pos - a.rows;
    int n;
    const int p = window_span(o + r, a.context, n);
    if (o < 0 || (int)threadIdx.x >= n || p < 0 || p >= a.ids_cap) return -1;
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

// ---------------------------------------------------------------- the verify of a draft MODEL's block
constexpr int DIST_T = 256, DIST_SLICE = 512;  // the sampler's partition of a row: 512 ids per workgroup, two adjacent ids per thread
constexpr unsigned SPEC_U_IDX4 = 0xFFFFFFFEu;  // the accept test's index word: the coin's is 0xFFFFFFFF, a vocabulary index's <= V / 4

struct DistPart {  // a tile's, then a row's, share of dist's normaliser: the largest kept log-probability and sum exp((lp - m) * inv_temp) over the kept ids
    double m, s;   // no kept id: m = -inf, s = 0
};

struct SpecDraftMeta {
    unsigned long long base;        // c = counter[0] at entry
    unsigned long long rcounter[2];  // the residual draw's stream position {c + n_acc, 0}: pie_sample's counter
    int n_acc, res_tok;
};

// pie_spec_verify_draft's workspace: the verify head | the drafter rows' tokens | the composed tokens | the meta record | both filters'
// records | the rows' and the tiles' normaliser shares | the tiles' flags | the residual row | the kept sets | the residual draw's sampler
// workspace | the filters'.  P rows are 0 .. rows - 1, Q rows rows .. 2 rows - 2 wherever both share an array.
struct SpecDraftLayout {
    int tiles;
    size_t tok, qtok, comp, meta, table, norms, parts, flags, resrow, mask, smp_res, smp, bytes;
    SpecDraftLayout(int rows, int V) {
        tiles = (V + DIST_SLICE - 1) / DIST_SLICE;
        const size_t dist_rows = 2 * (size_t)rows - 1;
        Carve c;
        tok = verify_head(c, rows, SPEC_MAX_ROWS);
        qtok = c.take(sizeof(int) * SPEC_MAX_ROWS);
        comp = c.take(sizeof(int) * SPEC_MAX_ROWS);
        meta = c.take(sizeof(SpecDraftMeta));
        table = c.take16(sizeof(pie_row_tail) * 2 * SPEC_MAX_ROWS);
        norms = c.take(sizeof(DistPart) * 2 * SPEC_MAX_ROWS);
        parts = c.take(sizeof(DistPart) * dist_rows * tiles);
        flags = c.take(sizeof(int) * tiles);
        resrow = c.take16(sizeof(float) * (size_t)V);
        mask = c.take16(dist_rows * (size_t)V);
        smp_res = c.take16(pie_sample_workspace_bytes(1, V));
        smp = c.take(pie_sample_workspace_bytes((int)dist_rows, V));
        bytes = c.at;
    }
};

struct SpecDraftArgs {
    SpecBlock b;                 // tok: the rows' ordinary draws
    pie_row_tail record;         // the sampler's, at stream position 0
    unsigned long long *counter;
    const float *logprobs;       // [rows, V]: the target's
    const float *q_logprobs;     // [rows - 1, V]: the drafter's
    const unsigned char *mask;   // [2 rows - 1, V]: the sampler's kept sets
    pie_row_tail *table;         // [2 rows - 1]
    unsigned long long *smp_ws;  // the filters' sampler workspaces, [2 rows - 1] rows, then ...
    unsigned long long *smp_res;  // ... the residual draw's one row (laid out in front of them)
    size_t smp_row_words;
    DistPart *parts, *norms;
    int tiles;
    int *flags;                  // [tiles]: the drawn residual row has a finite entry in the tile
    float *resrow;               // [V]: the residual row the last token is drawn from
    float *accept_rec, *residual;  // nullable diagnostics
    SpecDraftMeta *meta;
    int *comp;                   // [rows]: the accepted drafts, then the last token
};

__device__ __forceinline__ const float *dist_row_lp(const SpecDraftArgs &a, int r) {
    return r < a.b.rows ? a.logprobs + (size_t)r * a.b.V : a.q_logprobs + (size_t)(r - a.b.rows) * a.b.V;
}

// Both filters' records and the workspaces' re-armed headers: P row r draws at c + r -- its token is the row's ordinary draw --, a Q row
// is only filtered (its draw is discarded: any stream position does).
__global__ void __launch_bounds__(2 * SPEC_MAX_ROWS) k_spec_draft_fill(const SpecDraftArgs a) {
    const int r = threadIdx.x;
    pie_row_tail t = a.record;
    t.calls = a.counter[0];
    if (r == 0) {
        a.meta->base = t.calls;
        spec_rearm_header(a.smp_res);
    }
    if (r >= 2 * a.b.rows - 1) return;
    a.table[r] = spec_row_record(t, r < a.b.rows ? r : 0);
    spec_rearm_header(a.smp_ws + (size_t)r * a.smp_row_words);
}

// A block's sum and maximum in a fixed order: the butterfly inside a wave, then the four waves in turn.  Every thread gets the result.
__device__ __forceinline__ double dist_block_sum(double v, double *s_w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}
__device__ __forceinline__ double dist_block_max(double v, double *s_w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(s_w[0], s_w[1]), fmax(s_w[2], s_w[3]));
}

// Launch 1 of dist, over (tiles, 2 rows - 1): a tile's share of its row's normaliser.  The arithmetic is fp64 -- 2 x 63 x V exponentials
// are nothing beside the pass -- so that the residual's difference of two normalised rows keeps its digits where P and Q are close.
__global__ void __launch_bounds__(DIST_T) k_spec_dist_stats(const SpecDraftArgs a) {
    __shared__ double s_w[DIST_T / 64];
    const int r = blockIdx.y, base = blockIdx.x * DIST_SLICE + 2 * threadIdx.x, V = a.b.V;
    const float *lp = dist_row_lp(a, r);
    const unsigned char *mask = a.mask + (size_t)r * V;
    double x[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) x[j] = base + j < V && mask[base + j] ? (double)lp[base + j] : -INFINITY;
    const double m = dist_block_max(fmax(x[0], x[1]), s_w);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (x[j] != -INFINITY) s += exp((x[j] - m) * (double)a.record.inv_temp);
    s = dist_block_sum(s, s_w);
    if (threadIdx.x == 0) a.parts[(size_t)r * a.tiles + blockIdx.x] = DistPart{m, s};
}

// Launch 2 of dist, one workgroup per row: the tiles' shares in a fixed order (thread t takes tiles t, t + 256, ...; then the block's tree).
__global__ void __launch_bounds__(DIST_T) k_spec_dist_merge(const SpecDraftArgs a) {
    __shared__ double s_w[DIST_T / 64];
    const DistPart *p = a.parts + (size_t)blockIdx.x * a.tiles;
    double m = -INFINITY;
    for (int t = threadIdx.x; t < a.tiles; t += DIST_T) m = fmax(m, p[t].m);
    m = dist_block_max(m, s_w);
    double s = 0.0;
    for (int t = threadIdx.x; t < a.tiles; t += DIST_T)
        if (p[t].s > 0.0) s += p[t].s * exp((p[t].m - m) * (double)a.record.inv_temp);
    s = dist_block_sum(s, s_w);
    if (threadIdx.x == 0) a.norms[blockIdx.x] = DistPart{m, s};
}

// dist(x) of row r (0 <= x < V): 0 outside the kept set, and everywhere when the filter kept nothing
__device__ __forceinline__ double dist_at(const SpecDraftArgs &a, int r, int x) {
    const DistPart n = a.norms[r];
    if (!(n.s > 0.0) || !a.mask[(size_t)r * a.b.V + x]) return 0.0;
    return exp(((double)dist_row_lp(a, r)[x] - n.m) * (double)a.record.inv_temp) / n.s;
}

// u_i: XTC's coin construction (sampler.hip: k_smp_xtc) on the index word no coin and no vocabulary index uses.  The Philox block is
// restated here because sampler.hip keeps its own file-local.
__device__ __forceinline__ float spec_accept_u(unsigned long long seed, unsigned long long call) {
    unsigned c[4] = {SPEC_U_IDX4, 0u, (unsigned)call, (unsigned)(call >> 32)};
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return ((float)(c[0] >> 8) + 0.5f) * 0x1p-24f;
}

// Launch 3, over (tiles, 1) -- (tiles, rows - 1) with the residual diagnostic: every workgroup decides the drafts (thread i draft i, at
// most 31 in parallel: two dist values and one Philox block each), takes n_acc as the first refusal, and writes its tile of the residual
// row R_j, j = n_acc (and of every R_i into the diagnostic).  All drafts accepted: nothing is drawn from, nothing is written.
__global__ void __launch_bounds__(DIST_T) k_spec_draft_residual(const SpecDraftArgs a) {
    __shared__ int s_ok[SPEC_MAX_ROWS];
    __shared__ int s_acc;
    const int t = threadIdx.x, rows = a.b.rows, V = a.b.V, m = rows - 1;
    const unsigned long long c = a.meta->base;
    if (t < m) {
        const int d = a.b.draft[t];
        const bool in = d >= 0 && d < V;  // an id outside the vocabulary indexes nothing
        const float p = in ? (float)dist_at(a, t, d) : 0.0f, q = in ? (float)dist_at(a, rows + t, d) : 0.0f;
        const float u = spec_accept_u(a.record.seed, c + (unsigned long long)t);
        s_ok[t] = in && q > 0.0f && __fmul_rn(u, q) < p;
        if (a.accept_rec && blockIdx.x == 0 && blockIdx.y == 0) a.accept_rec[3 * t] = p, a.accept_rec[3 * t + 1] = q, a.accept_rec[3 * t + 2] = u;
    }
    __syncthreads();
    if (t == 0) {
        int n = 0;
        while (n < m && s_ok[n]) ++n;
        s_acc = n;
        if (blockIdx.x == 0 && blockIdx.y == 0) a.meta->n_acc = n, a.meta->rcounter[0] = c + (unsigned long long)n, a.meta->rcounter[1] = 0ull;
    }
    __syncthreads();
    const int j = s_acc, r = a.residual ? (int)blockIdx.y : j;
    if (r >= m) return;  // block-uniform
    const int base = blockIdx.x * DIST_SLICE + 2 * t;
    bool finite = false;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int x = base + e;
        if (x >= V) continue;
        const double diff = dist_at(a, r, x) - dist_at(a, rows + r, x);
        const float v = diff > 0.0 ? (float)log(diff) : -INFINITY;
        finite = finite || diff > 0.0;
        if (a.residual) a.residual[(size_t)r * V + x] = v;
        if (r == j) a.resrow[x] = v;
    }
    const int any = __syncthreads_or(finite ? 1 : 0);
    if (r == j && t == 0) a.flags[blockIdx.x] = any;
}

// The last launch, one workgroup: whether the drawn residual row had a finite entry (an OR over the tiles' flags), then one thread composes
// the tokens and commits through the function both other verifies end in.
__global__ void __launch_bounds__(DIST_T) k_spec_draft_commit(const SpecDraftArgs a) {
    int any = 0;
    for (int t = threadIdx.x; t < a.tiles; t += DIST_T) any |= a.flags[t];
    any = __syncthreads_or(any);
    if (threadIdx.x != 0) return;
    const int n_acc = a.meta->n_acc;
    for (int i = 0; i < n_acc; ++i) a.comp[i] = a.b.draft[i];
    // the bonus token behind a fully accepted block, the residual's draw behind a refusal, the row's ordinary draw when the residual is empty
    a.comp[n_acc] = n_acc < a.b.rows - 1 && any ? a.meta->res_tok : a.b.tok[n_acc];
    spec_commit(a.b.s, a.comp, a.b.rows, n_acc, a.b.out_tokens, a.b.out_n);
    a.counter[0] = a.meta->base + (unsigned long long)(n_acc + 1), a.counter[1] = 0ull;
}

}  // namespace

int spec_verify_launch(const u16 *logits, int rows, int V, int dtype, const int *draft, int *out_tokens, int *out_n, float *logprobs, void *workspace,
                       const SpecState &s, hipStream_t st) {
    const SpecGreedyLayout lay(rows, SPEC_MAX_ROWS);
    char *ws = (char *)workspace;
    int *tok = (int *)(ws + lay.tok);
    float *lse = (float *)(ws + lay.lse);
    const SpecArgs a = {logits, SpecBlock{rows, V, draft, tok, out_tokens, out_n, s}, lse, logprobs};
    return launch_for_dtype(dtype, "spec verify:", [&](auto t) {
        using T = decltype(t);
        spec_greedy_rows<T>(logits, rows, V, (LogitStat *)ws, tok, lse, st);
        hipLaunchKernelGGL(k_spec_accept<T>, dim3(TAIL_FINISH_BLOCKS, (unsigned)rows), dim3(256), 0, st, a);
    });
}

// The sampler's record at stream position 0, as sample_launch derives it: the fill kernels put the call's position in.
static pie_row_tail spec_sampler_record(int mode, double temp, double p, int k, unsigned long long seed) {
    pie_row_tail t = {};
    t.mode = mode, t.seed = seed;
    sample_derive(mode, temp, p, k, &t.inv_temp, &t.thr, &t.k);
    return t;
}

// pie_spec_verify_sampled's launches behind whatever made the logits.  mode PIE_SAMPLE_GREEDY (the decoder's penalty- or bias-only tails):
// the rows' tokens are their argmaxes, nothing is drawn and the counter is not touched.
static int spec_verify_sampled_launch(u16 *logits, int rows, int V, int dtype, const int *draft, int mode, double temp, double p, int k, unsigned long long seed,
                                      unsigned long long *counter, const pie_xtc *xtc, int *out_tokens, int *out_n, float *logprobs, void *workspace,
                                      const SpecState &s, hipStream_t st, const SpecDfa *dfa = nullptr) {
    const SpecSampledLayout lay(rows, V);
    char *ws = (char *)workspace;
    int *tok = (int *)(ws + lay.tok);
    unsigned long long *base = (unsigned long long *)(ws + lay.base);
    // dfa (pie_decoder_spec_step_dfa): every row's partials are masked with the row's own words, and the accept launch moves the automaton
    if (int rc = logits_tail_rows_launch(dtype, logits, V, rows, (LogitStat *)ws, logprobs, tok, st, dfa ? dfa->masks : nullptr, dfa ? dfa->mask_words : 0,
                                         dfa ? dfa->mask_on : nullptr))
        return rc;
    const bool draws = mode != PIE_SAMPLE_GREEDY;
    if (draws) {
        SpecFillArgs f = {};
        f.rows = rows, f.record = spec_sampler_record(mode, temp, p, k, seed), f.counter = counter, f.xtc = xtc, f.base = base;
        f.table = (pie_row_tail *)(ws + lay.table), f.xtc_rows = (pie_xtc *)(ws + lay.xtc);
        f.smp_ws = (unsigned long long *)(ws + lay.smp), f.smp_row_words = pie_sample_workspace_bytes(1, V) / sizeof(unsigned long long);
        hipLaunchKernelGGL(k_spec_fill_rows, dim3(1), dim3(SPEC_MAX_ROWS), 0, st, f);
        PIE_LAUNCH_CHECK();
        if (int rc = sample_rows_launch(logprobs, rows, V, f.table, ws + lay.smp, tok, nullptr, nullptr, st, SampleXtc{xtc ? f.xtc_rows : nullptr, nullptr})) return rc;
    }
    const SpecSampledArgs a = {SpecBlock{rows, V, draft, tok, out_tokens, out_n, s}, base, draws ? counter : nullptr};
    if (dfa) hipLaunchKernelGGL(k_spec_accept_dfa, dim3(1), dim3(64), 0, st, a, *dfa);
    else hipLaunchKernelGGL(k_spec_accept_sampled, dim3(1), dim3(64), 0, st, a);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

int spec_verify_rows_launch(const u16 *logits, int N, int V, int dtype, const int *seg_first, int B, const int *draft, int draft_stride, int *out_tokens,
                            int *out_n, int *ids, int *len, int cap, void *workspace, hipStream_t st) {
    const SpecGreedyLayout lay(N, N);
    char *ws = (char *)workspace;
    int *tok = (int *)(ws + lay.tok);
    const SpecRowsArgs a = {N, B, V, seg_first, draft, draft_stride, tok, out_tokens, out_n, ids, len, cap};
    return launch_for_dtype(dtype, "spec verify rows:", [&](auto t) {
        spec_greedy_rows<decltype(t)>(logits, N, V, (LogitStat *)ws, tok, (float *)(ws + lay.lse), st);
        hipLaunchKernelGGL(k_spec_accept_rows, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, a);
    });
}

// The records are filled with the greedy mode first: a row no segment covers draws nothing.
int spec_verify_rows_sampled_launch(const SpecSeats &q, u16 *logits, int N, int V, int dtype, const int *seg_first, int B, const int *fed, const int *draft,
                                    int draft_stride, int *out_tokens, int *out_n, float *logprobs, int *ids, int *len, int cap, void *workspace, hipStream_t st) {
    const SpecRowsSampledLayout lay(N, V);
    char *ws = (char *)workspace;
    int *tok = (int *)(ws + lay.tok);
    SpecSeatsArgs a = {};
    a.q = q, a.logits = logits, a.N = N, a.B = B, a.V = V, a.seg_first = seg_first, a.fed = fed;
    a.table_rows = (pie_row_tail *)(ws + lay.table), a.xtc_rows = (pie_xtc *)(ws + lay.xtc);
    a.smp_ws = (unsigned long long *)(ws + lay.smp), a.smp_row_words = pie_sample_workspace_bytes(1, V) / sizeof(unsigned long long);
    if (int rc = launch_for_dtype(dtype, "spec verify rows sampled:", [&](auto t) {
            hipLaunchKernelGGL(k_spec_edit_seg_rows<decltype(t)>, dim3(SPEC_SEG_ROWS, (unsigned)B), dim3(PEN_MAX_IDS), 0, st, a);
        }))
        return rc;
    if (int rc = logits_tail_rows_launch(dtype, logits, V, N, (LogitStat *)ws, logprobs, tok, st)) return rc;
    PIE_HIP_TRY(hipMemsetAsync(a.table_rows, 0xFF, sizeof(pie_row_tail) * (size_t)N, st));  // mode = PIE_SAMPLE_GREEDY in every record
    hipLaunchKernelGGL(k_spec_fill_seg_rows, dim3((unsigned)B), dim3(64), 0, st, a);
    PIE_LAUNCH_CHECK();
    if (int rc = sample_rows_launch(logprobs, N, V, a.table_rows, ws + lay.smp, tok, nullptr, nullptr, st, SampleXtc{q.xtc ? a.xtc_rows : nullptr, nullptr})) return rc;
    const SpecRowsArgs r = {N, B, V, seg_first, draft, draft_stride, tok, out_tokens, out_n, ids, len, cap};
    hipLaunchKernelGGL(k_spec_commit_rows, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, r, q, fed);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

int spec_gather_rows_launch(const int *tokens, const int *draft, int draft_stride, const int *seg_first, int B, int N, int vocab, int *fed, hipStream_t st) {
    hipLaunchKernelGGL(k_spec_gather_rows, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, tokens, draft, draft_stride, seg_first, B, N, vocab, fed);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// pie_spec_verify_draft's launches behind whatever made the logits
static int spec_verify_draft_launch(u16 *logits, int rows, int V, int dtype, const int *draft, const float *q_logprobs, int mode, double temp, double p, int k,
                                    unsigned long long seed, unsigned long long *counter, int *out_tokens, int *out_n, float *logprobs, float *accept_rec,
                                    float *residual, void *workspace, const SpecState &s, hipStream_t st) {
    const SpecDraftLayout lay(rows, V);
    char *ws = (char *)workspace;
    const int dist_rows = 2 * rows - 1;
    unsigned char *mask = (unsigned char *)(ws + lay.mask);
    int *tok = (int *)(ws + lay.tok), *qtok = (int *)(ws + lay.qtok);
    SpecDraftArgs a = {};
    a.b = SpecBlock{rows, V, draft, tok, out_tokens, out_n, s}, a.record = spec_sampler_record(mode, temp, p, k, seed), a.counter = counter;
    a.logprobs = logprobs, a.q_logprobs = q_logprobs;
    a.mask = mask, a.table = (pie_row_tail *)(ws + lay.table), a.smp_ws = (unsigned long long *)(ws + lay.smp), a.smp_res = (unsigned long long *)(ws + lay.smp_res);
    a.smp_row_words = pie_sample_workspace_bytes(1, V) / sizeof(unsigned long long);
    a.parts = (DistPart *)(ws + lay.parts), a.norms = (DistPart *)(ws + lay.norms), a.tiles = lay.tiles, a.flags = (int *)(ws + lay.flags);
    a.resrow = (float *)(ws + lay.resrow), a.accept_rec = accept_rec, a.residual = residual, a.meta = (SpecDraftMeta *)(ws + lay.meta);
    a.comp = (int *)(ws + lay.comp);
    if (int rc = logits_tail_rows_launch(dtype, logits, V, rows, (LogitStat *)ws, logprobs, tok, st)) return rc;
    hipLaunchKernelGGL(k_spec_draft_fill, dim3(1), dim3(2 * SPEC_MAX_ROWS), 0, st, a);
    PIE_LAUNCH_CHECK();
    // the kept sets are the sampler's own: its filter launches with a mask output, over the target's rows (whose draws are the rows' ordinary
    // tokens) and over the drafter's (whose draws are discarded)
    if (int rc = sample_rows_launch(logprobs, rows, V, a.table, a.smp_ws, tok, nullptr, mask, st)) return rc;
    if (int rc = sample_rows_launch(q_logprobs, rows - 1, V, a.table + rows, a.smp_ws + (size_t)rows * a.smp_row_words, qtok, nullptr, mask + (size_t)rows * V, st)) return rc;
    hipLaunchKernelGGL(k_spec_dist_stats, dim3((unsigned)lay.tiles, (unsigned)dist_rows), dim3(DIST_T), 0, st, a);
    hipLaunchKernelGGL(k_spec_dist_merge, dim3((unsigned)dist_rows), dim3(DIST_T), 0, st, a);
    hipLaunchKernelGGL(k_spec_draft_residual, dim3((unsigned)lay.tiles, residual ? (unsigned)(rows - 1) : 1u), dim3(DIST_T), 0, st, a);
    PIE_LAUNCH_CHECK();
    // the residual's draw IS pie_sample(CATEGORICAL, temp = 1) on that row at {c + n_acc, 0}; behind a fully accepted block it draws from
    // whatever the row holds and nobody reads the token
    SampleFeed none = {};
    if (int rc = sample_launch(a.resrow, 1, V, PIE_SAMPLE_CATEGORICAL, 1.0, 0.0, 0, seed, a.meta->rcounter, a.smp_res, &a.meta->res_tok, nullptr, nullptr, none, st)) return rc;
    hipLaunchKernelGGL(k_spec_draft_commit, dim3(1), dim3(DIST_T), 0, st, a);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// ---------------------------------------------------------------- the op entries' checks
// The drafter over B sequences, checked (rows: pie_ngram_draft_rows, which also bounds B; pie_ngram_draft is B = 1)
static int ngram_draft_checked(const char *entry, bool rows, const int32_t *ids, const int32_t *len, int B, int cap, int ngram_max, int ngram_min, int k,
                               int32_t *out_ids, int32_t *out_count, void *workspace, void *stream) {
    const std::string who = std::string(entry) + ": ";
    PIE_REQUIRE(ngram_min >= 1 && ngram_min <= ngram_max && ngram_max <= SPEC_MAX_NGRAM, PIE_E_ARG, who + "need 1 <= ngram_min <= ngram_max <= 8");
    PIE_REQUIRE(k >= 1 && k <= SPEC_MAX_ROWS - 1, PIE_E_ARG, who + "k must be 1..31");
    PIE_REQUIRE(ids && len && out_ids && out_count && workspace, PIE_E_ARG, who + "null pointer");
    PIE_REQUIRE(!rows || (B >= 1 && B <= SPEC_MAX_SEQS), PIE_E_SHAPE, who + "B must be 1..4096");
    PIE_REQUIRE(cap >= 1 && cap <= SPEC_MAX_IDS, PIE_E_SHAPE, who + "cap must be 1..2^27");
    PIE_REQUIRE(pie_aligned(ids, 4) && pie_aligned(len, 4) && pie_aligned(out_ids, 4) && pie_aligned(out_count, 4) && pie_aligned(workspace, 4), PIE_E_ALIGN,
                who + "4-byte alignment required");
    hipStream_t st = (hipStream_t)stream;
    const int wgs = (cap + NGRAM_IDS_PER_WG - 1) / NGRAM_IDS_PER_WG;  // the grid per sequence: the same partials, the same maximum, whatever B
    const int G = wgs < 1 ? 1 : (wgs > NGRAM_MAX_WGS ? NGRAM_MAX_WGS : wgs);
    hipLaunchKernelGGL(k_ngram_search, dim3((unsigned)G, (unsigned)B), dim3(NGRAM_T), 0, st, ids, len, cap, ngram_max, ngram_min, (unsigned *)workspace);
    PIE_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ngram_pick, dim3((unsigned)B), dim3(NGRAM_T), 0, st, ids, len, cap, (const unsigned *)workspace, G, k, out_ids, out_count);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

// What pie_spec_verify, pie_spec_verify_sampled and pie_spec_verify_draft check of their block.  others / others_aligned: the entry's
// further required pointers are there / its further arrays are 4-byte aligned; aligned_words: the entry's own wording of that refusal.
static int spec_block_check(const char *entry, const void *logits, int rows, int V, int dtype, const int32_t *draft, const int32_t *out_tokens, const int32_t *out_n,
                            const float *logprobs, const void *workspace, bool others, bool others_aligned, const char *aligned_words) {
    const std::string who = std::string(entry) + ": ";
    PIE_REQUIRE(logits && draft && out_tokens && out_n && workspace && others, PIE_E_ARG, who + "null pointer");
    PIE_REQUIRE(rows >= 2 && rows <= SPEC_MAX_ROWS && V >= 1, PIE_E_SHAPE, who + "need 2 <= rows <= 32 and V >= 1");
    PIE_REQUIRE(pie_aligned(logits, 2) && pie_aligned(draft, 4) && pie_aligned(out_tokens, 4) && pie_aligned(out_n, 4) && pie_aligned(logprobs, 4) && others_aligned,
                PIE_E_ALIGN, who + aligned_words);
    PIE_REQUIRE(pie_aligned(workspace, 16), PIE_E_ALIGN, who + "workspace needs 16-byte alignment");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, who + "dtype must be PIE_BF16 or PIE_F16");
    return PIE_OK;
}

// What pie_spec_verify_rows and pie_spec_verify_rows_sampled check of their segmented block.  others, others_aligned, aligned_words: as
// above; v_ok and shape_words: the entry's own bound on V and its wording of the shape refusal.
static int spec_rows_check(const char *entry, const void *logits, int n_rows, bool v_ok, int dtype, const int32_t *seg_first, int B, const int32_t *draft_ids,
                           int draft_stride, const int32_t *out_tokens, const int32_t *out_n, const int32_t *ids, const int32_t *len, int cap, const void *workspace,
                           bool others, const char *shape_words, bool others_aligned, const char *aligned_words) {
    const std::string who = std::string(entry) + ": ";
    PIE_REQUIRE(logits && seg_first && draft_ids && out_tokens && out_n && workspace && others, PIE_E_ARG, who + "null pointer");
    PIE_REQUIRE((ids == nullptr) == (len == nullptr) && (ids || cap == 0) && (!ids || cap >= 1), PIE_E_ARG, who + "ids [B, cap >= 1] and len come together or not at all");
    PIE_REQUIRE(dtype == PIE_BF16 || dtype == PIE_F16, PIE_E_ARG, who + "dtype must be PIE_BF16 or PIE_F16");
    PIE_REQUIRE(n_rows >= 1 && n_rows <= 65535 && v_ok && B >= 1 && B <= SPEC_MAX_SEQS && draft_stride >= 1, PIE_E_SHAPE, who + shape_words);
    PIE_REQUIRE(pie_aligned(logits, 2) && pie_aligned(seg_first, 4) && pie_aligned(draft_ids, 4) && pie_aligned(out_tokens, 4) && pie_aligned(out_n, 4) &&
                    pie_aligned(ids, 4) && pie_aligned(len, 4) && others_aligned, PIE_E_ALIGN, who + aligned_words);
    PIE_REQUIRE(pie_aligned(workspace, 16), PIE_E_ALIGN, who + "workspace needs 16-byte alignment");
    return PIE_OK;
}

extern "C" {

size_t pie_ngram_draft_workspace_bytes(void) { return sizeof(unsigned) * NGRAM_MAX_WGS; }

int pie_ngram_draft(const int32_t *ids, const int32_t *len, int cap, int ngram_max, int ngram_min, int k, int32_t *out_ids, int32_t *out_count,
                    void *workspace, void *stream) {
    return ngram_draft_checked("pie_ngram_draft", false, ids, len, 1, cap, ngram_max, ngram_min, k, out_ids, out_count, workspace, stream);
}

size_t pie_ngram_draft_rows_workspace_bytes(int B) { return B < 1 || B > SPEC_MAX_SEQS ? 0 : sizeof(unsigned) * NGRAM_MAX_WGS * (size_t)B; }

int pie_ngram_draft_rows(const int32_t *ids, const int32_t *len, int B, int cap, int ngram_max, int ngram_min, int k, int32_t *out_ids, int32_t *out_count,
                         void *workspace, void *stream) {
    return ngram_draft_checked("pie_ngram_draft_rows", true, ids, len, B, cap, ngram_max, ngram_min, k, out_ids, out_count, workspace, stream);
}

size_t pie_spec_verify_workspace_bytes(int rows) { return rows < 2 || rows > SPEC_MAX_ROWS ? 0 : SpecGreedyLayout(rows, SPEC_MAX_ROWS).bytes; }

int pie_spec_verify(const void *logits, int rows, int V, int dtype, const int32_t *draft, int32_t *out_tokens, int32_t *out_n, float *logprobs,
                    void *workspace, void *stream) {
    if (int rc = spec_block_check("pie_spec_verify", logits, rows, V, dtype, draft, out_tokens, out_n, logprobs, workspace, true, true,
                                  "logits need 2-byte, the draft and the outputs 4-byte alignment"))
        return rc;
    return spec_verify_launch((const u16 *)logits, rows, V, dtype, draft, out_tokens, out_n, logprobs, workspace, SpecState(), (hipStream_t)stream);
}

size_t pie_spec_verify_rows_workspace_bytes(int n_rows) { return n_rows < 1 || n_rows > 65535 ? 0 : SpecGreedyLayout(n_rows, n_rows).bytes; }

int pie_spec_verify_rows(const void *logits, int n_rows, int V, int dtype, const int32_t *seg_first, int B, const int32_t *draft_ids, int draft_stride,
                         int32_t *out_tokens, int32_t *out_n, int32_t *ids, int32_t *len, int cap, void *workspace, void *stream) {
    if (int rc = spec_rows_check("pie_spec_verify_rows", logits, n_rows, V >= 1, dtype, seg_first, B, draft_ids, draft_stride, out_tokens, out_n, ids, len, cap, workspace, true,
                                 "need 1 <= n_rows <= 65535, V >= 1, 1 <= B <= 4096 and draft_stride >= 1", true,
                                 "logits need 2-byte, the index arrays and the outputs 4-byte alignment"))
        return rc;
    return spec_verify_rows_launch((const u16 *)logits, n_rows, V, dtype, seg_first, B, draft_ids, draft_stride, out_tokens, out_n, ids, len, cap, workspace,
                                   (hipStream_t)stream);
}

size_t pie_spec_verify_rows_sampled_workspace_bytes(int n_rows, int V) {
    return n_rows < 1 || n_rows > 65535 || pie_sample_workspace_bytes(n_rows, V) == 0 ? 0 : SpecRowsSampledLayout(n_rows, V).bytes;
}

int pie_spec_verify_rows_sampled(void *logits, int n_rows, int V, int dtype, const int32_t *seg_first, int B, const int32_t *fed, const int32_t *draft_ids,
                                 int draft_stride, const int32_t *pos0, pie_row_tail *table, int32_t *recent_ids, const int32_t *bias_ids, const float *bias_vals,
                                 const int32_t *bias_n, int bias_cap, const pie_xtc *xtc, int32_t *out_tokens, int32_t *out_n, float *logprobs, int32_t *ids,
                                 int32_t *len, int cap, void *workspace, void *stream) {
    const std::string who = "pie_spec_verify_rows_sampled: ";
    if (int rc = spec_rows_check("pie_spec_verify_rows_sampled", logits, n_rows, pie_sample_workspace_bytes(n_rows, V) != 0, dtype, seg_first, B, draft_ids, draft_stride,
                                 out_tokens, out_n, ids, len, cap, workspace, fed && pos0 && table && recent_ids && logprobs,
                                 "need 1 <= n_rows <= 65535, 1 <= V <= 524288, 1 <= B <= 4096 and draft_stride >= 1",
                                 pie_aligned(fed, 4) && pie_aligned(pos0, 4) && pie_aligned(recent_ids, 4) && pie_aligned(bias_ids, 4) && pie_aligned(bias_vals, 4) &&
                                     pie_aligned(bias_n, 4) && pie_aligned(xtc, 4) && pie_aligned(logprobs, 4),
                                 "logits need 2-byte, the index arrays, the seats' state and the outputs 4-byte alignment"))
        return rc;
    PIE_REQUIRE(bias_ids ? (bias_vals && bias_n && bias_cap >= 1 && bias_cap <= PEN_MAX_IDS) : (!bias_vals && !bias_n && bias_cap == 0), PIE_E_ARG,
                who + "bias_ids, bias_vals [B, 1 <= bias_cap <= 1024] and bias_n come together or not at all");
    PIE_REQUIRE(pie_aligned(table, 8), PIE_E_ALIGN, who + "the table needs 8-byte alignment");
    SpecSeats q;
    q.table = table, q.recent = recent_ids, q.pos0 = pos0, q.bias_ids = bias_ids, q.bias_vals = bias_vals, q.bias_n = bias_n, q.bias_cap = bias_cap, q.xtc = xtc;
    return spec_verify_rows_sampled_launch(q, (u16 *)logits, n_rows, V, dtype, seg_first, B, fed, draft_ids, draft_stride, out_tokens, out_n, logprobs, ids, len, cap,
                                           workspace, (hipStream_t)stream);
}

size_t pie_spec_verify_sampled_workspace_bytes(int rows, int V) {
    if (rows < 2 || rows > SPEC_MAX_ROWS || pie_sample_workspace_bytes(rows, V) == 0) return 0;
    return SpecSampledLayout(rows, V).bytes;
}

int pie_spec_verify_sampled(const void *logits, int rows, int V, int dtype, const int32_t *draft, int mode, double temp, double p, int k, unsigned long long seed,
                            unsigned long long *counter, const pie_xtc *xtc, int32_t *out_tokens, int32_t *out_n, float *logprobs, void *workspace, void *stream) {
    if (int rc = spec_block_check("pie_spec_verify_sampled", logits, rows, V, dtype, draft, out_tokens, out_n, logprobs, workspace, counter && logprobs, pie_aligned(xtc, 4),
                                  "logits need 2-byte, the draft, the XTC record and the outputs 4-byte alignment"))
        return rc;
    PIE_REQUIRE(mode != PIE_SAMPLE_GREEDY, PIE_E_ARG, "pie_spec_verify_sampled: the greedy sampler draws nothing (use pie_spec_verify)");
    PIE_REQUIRE(pie_aligned(counter, 8), PIE_E_ALIGN, "pie_spec_verify_sampled: the counter needs 8-byte alignment");
    if (int rc = sample_check("pie_spec_verify_sampled", V, mode, temp, p, k, workspace)) return rc;
    return spec_verify_sampled_launch((u16 *)const_cast<void *>(logits), rows, V, dtype, draft, mode, temp, p, k, seed, counter, xtc, out_tokens, out_n, logprobs,
                                      workspace, SpecState(), (hipStream_t)stream);
}

size_t pie_spec_verify_draft_workspace_bytes(int rows, int V) {
    if (rows < 2 || rows > SPEC_MAX_ROWS || pie_sample_workspace_bytes(rows, V) == 0) return 0;
    return SpecDraftLayout(rows, V).bytes;
}

int pie_spec_verify_draft(const void *logits, int rows, int V, int dtype, const int32_t *draft, const float *q_logprobs, int mode, double temp, double p, int k,
                          unsigned long long seed, unsigned long long *counter, int32_t *out_tokens, int32_t *out_n, float *logprobs, float *accept_rec, float *residual,
                          void *workspace, void *stream) {
    if (int rc = spec_block_check("pie_spec_verify_draft", logits, rows, V, dtype, draft, out_tokens, out_n, logprobs, workspace, q_logprobs && counter && logprobs,
                                  pie_aligned(q_logprobs, 4) && pie_aligned(accept_rec, 4) && pie_aligned(residual, 4),
                                  "logits need 2-byte, the draft, its log-probabilities and the outputs 4-byte alignment"))
        return rc;
    PIE_REQUIRE(mode != PIE_SAMPLE_GREEDY, PIE_E_ARG, "pie_spec_verify_draft: a greedy draft is a point mass (use pie_spec_verify)");
    PIE_REQUIRE(pie_aligned(counter, 8), PIE_E_ALIGN, "pie_spec_verify_draft: the counter needs 8-byte alignment");
    if (int rc = sample_check("pie_spec_verify_draft", V, mode, temp, p, k, workspace)) return rc;
    return spec_verify_draft_launch((u16 *)const_cast<void *>(logits), rows, V, dtype, draft, q_logprobs, mode, temp, p, k, seed, counter, out_tokens, out_n, logprobs,
                                    accept_rec, residual, workspace, SpecState(), (hipStream_t)stream);
}

// The pass workspace (SpecPassLayout) over the logits block [rows, vocab] and 32 fed ids, with the kind's verify workspace behind it (for
// _dfa, behind pie_spec_verify_sampled's: the states in front of the rows [32] | mask_on [32] | the record per row [32] | the rows' mask words)
static size_t spec_pass_bytes(const pie_decoder *d, int rows, size_t verify_bytes) { return SpecPassLayout(rows, SPEC_MAX_ROWS, d->cfg.vocab).bytes(verify_bytes); }

size_t pie_decoder_spec_workspace_bytes(const pie_decoder *d, int rows) { return d ? spec_pass_bytes(d, rows, pie_spec_verify_workspace_bytes(rows)) : 0; }

size_t pie_decoder_spec_tail_workspace_bytes(const pie_decoder *d, int rows) {
    return d ? spec_pass_bytes(d, rows, pie_spec_verify_sampled_workspace_bytes(rows, d->cfg.vocab)) : 0;
}

size_t pie_decoder_spec_dfa_workspace_bytes(const pie_decoder *d, int rows) {
    const size_t head = pie_decoder_spec_tail_workspace_bytes(d, rows);
    return head ? SpecDfaLayout(head, d->cfg.vocab).bytes : 0;
}

size_t pie_decoder_spec_draft_workspace_bytes(const pie_decoder *d, int rows) {
    return d ? spec_pass_bytes(d, rows, pie_spec_verify_draft_workspace_bytes(rows, d->cfg.vocab)) : 0;
}

}  // extern "C"

// ---------------------------------------------------------------- the decoder's pass entries
enum SpecKind { SPEC_RAW = 0, SPEC_TAIL = 1, SPEC_DRAFT = 2, SPEC_DFA = 3 };  // pie_decoder_spec_step, _spec_step_tail, _spec_step_draft, _spec_step_dfa

// The rows' edits behind the pass, in the step tail's order: penalty, then bias (one launch, none when neither is set); with a penalty the
// accept launch keeps ids_by_pos whole.
static int spec_edit_launch(pie_decoder *d, const int32_t *draft_ids, int rows, void *workspace, SpecState *s, hipStream_t st) {
    const pie_decoder_config &c = d->cfg;
    const StepTail &t = d->tail;
    if (t.penalty.on()) s->ids_by_pos = t.penalty.ids_by_pos, s->ids_cap = t.penalty.ids_cap;
    if (!t.penalty.on() && !t.bias.on()) return PIE_OK;
    SpecEditArgs e = {};
    e.logits = (u16 *)workspace, e.V = c.vocab, e.rows = rows, e.penalty = (float)t.penalty.value, e.context = t.penalty.context, e.ids_by_pos = t.penalty.ids_by_pos, e.ids_cap = t.penalty.ids_cap;
    e.state = d->state, e.fed = s->fed, e.draft = draft_ids;
    e.b = BiasArgs{t.bias.ids, t.bias.vals, t.bias.n, t.penalty.on()};
    return launch_for_dtype(c.dtype, "spec edit:", [&](auto ty) { hipLaunchKernelGGL(k_spec_edit_rows<decltype(ty)>, dim3((unsigned)rows), dim3(PEN_MAX_IDS), 0, st, e); });
}

// The four pie_decoder_spec_step* entries, one speculative pass of kind `kind`.  The prologue: the kind's refusals -- which parts of the
// step's tail the pass admits is StepTail's answer (decoder.hpp) --, the shape and alignment checks, the workspace's carve-up
// (SpecPassLayout), the gather of the input rows, the SpecState fill and the many-row pass itself, raw logits on every row.  Then, for
// SPEC_DFA, the automaton's walk and the rows' masks; the edit (every kind but the raw one); the kind's verify.  q_logprobs: SPEC_DRAFT's.
static int spec_step(const char *entry, SpecKind kind, pie_decoder *d, const int32_t *draft_ids, int n_draft, const float *q_logprobs, int32_t *out_tokens,
                     int32_t *out_n, float *logprobs_rows, void *workspace, int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream) {
    const std::string who = std::string(entry) + ": ";
    const bool with_tail = kind != SPEC_RAW;
    PIE_REQUIRE(d && draft_ids && out_tokens && out_n && (logprobs_rows || !with_tail) && workspace, PIE_E_ARG, who + "null pointer");
    PIE_REQUIRE(!d->tp(), PIE_E_STATE, who + "not available on a tensor-parallel shard");
    PIE_REQUIRE(!d->kv_quant && !d->ring, PIE_E_STATE, who + "not available on a quantized or rotating KV cache");
    PIE_REQUIRE(!d->kv_i8, PIE_E_STATE, who + "not available on int8 KV pages");
    const StepTail &t = d->tail;
    if (!with_tail) {
        PIE_REQUIRE(!t.configured() && !d->prompt.n, PIE_E_STATE,
                    who + "speculation is greedy and raw: no sampler, penalty, mask, bias, top-logprobs, counts or prompt scoring may be set");
        PIE_REQUIRE(!t.xtc.on(), PIE_E_STATE, who + "speculation is greedy: no XTC record may be set");
    } else if (kind == SPEC_DFA) {  // the tail's pass plus the automaton, which alone is enough
        const char *part = t.spec_dfa_refused();
        PIE_REQUIRE(!part, PIE_E_STATE, who + "not available with " + part);
        PIE_REQUIRE(!d->prompt.n, PIE_E_STATE, who + "not available with prompt scoring");
        PIE_REQUIRE(t.dfa.on(), PIE_E_STATE, who + "no token automaton is set (the pass without one is pie_decoder_spec_step_tail)");
    } else {
        const char *part = t.spec_tail_refused();
        PIE_REQUIRE(!part, PIE_E_STATE, who + "not available with " + part);
        PIE_REQUIRE(!d->prompt.n, PIE_E_STATE, who + "not available with prompt scoring");
        // XTC's coin changes the target's distribution from call to call: the acceptance test would need the coin of every row's own call
        PIE_REQUIRE(kind != SPEC_DRAFT || !t.xtc.on(), PIE_E_STATE, who + "not available with an XTC record");
        PIE_REQUIRE(kind != SPEC_DRAFT || t.sampler.on(), PIE_E_STATE,
                    who + "no stochastic sampler is set (a greedy draft is a point mass: pie_decoder_spec_step or pie_decoder_spec_step_tail)");
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
    const SpecPassLayout lay(rows, SPEC_MAX_ROWS, V);
    int *fed = (int *)((char *)workspace + lay.fed);
    void *verify_ws = (char *)workspace + lay.verify;
    PIE_REQUIRE(d->glob_set && d->kv_set && d->out_set, PIE_E_STATE, "pie_decoder: set_globals, set_kv and bind_outputs must be called before stepping");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_spec_gather, dim3(1), dim3(SPEC_MAX_ROWS), 0, st, (const DecState *)d->state, draft_ids, n_draft, d->embed_vocab(), fed);
    PIE_LAUNCH_CHECK();
    SpecState s;
    s.state = d->state, s.history = d->history, s.hist_cap = d->hist_cap, s.fed = fed;
    s.seq_ids = seq_ids, s.seq_cap = seq_cap, s.seq_len = seq_len, s.token_out = d->token_out;
    // Raw logits on every row: logits_all != nullptr makes the pass's own last-row tail raw and greedy (pie_decoder::tail_raw), which leaves
    // pos = o + rows; a configured sampler draws nothing there and its counter stays where it is.
    if (int rc = pie_decoder_prefill(d, fed, rows, workspace, stream)) return rc;
    const int dtype = d->cfg.dtype;
    u16 *logits = (u16 *)workspace;
    if (kind == SPEC_RAW) return spec_verify_launch(logits, rows, V, dtype, draft_ids, out_tokens, out_n, logprobs_rows, verify_ws, s, st);
    SpecDfa f = {};
    if (kind == SPEC_DFA) {
        const StepTail::Dfa &a = d->tail.dfa;
        const SpecDfaLayout lay(pie_decoder_spec_tail_workspace_bytes(d, rows), V);
        char *ws = (char *)workspace;
        f = {a.record, a.state, a.tables, a.tables_len, (int *)(ws + lay.states), (int *)(ws + lay.mask_on), (pie_row_dfa *)(ws + lay.records),
             (unsigned *)(ws + lay.masks), lay.mask_words};
        // the state in front of every row, from the caller's draft (an id the grammar forbids leaves the automaton: the rows behind it are
        // unmasked, and never accepted -- the forbidden id's own row is masked in the state before it), then the rows' masks
        if (int rc = token_dfa_walk_launch(a.record, a.state, a.tables, a.tables_len, V, draft_ids, n_draft, f.states, f.records, f.mask_on, st)) return rc;
        if (int rc = token_dfa_mask_launch(f.records, f.states, a.tables, a.tables_len, rows, V, f.masks, f.mask_words, f.mask_on, st)) return rc;
    }
    if (int rc = spec_edit_launch(d, draft_ids, rows, workspace, &s, st)) return rc;
    const StepTail::Sampler &m = d->tail.sampler;
    if (kind == SPEC_DRAFT)
        return spec_verify_draft_launch(logits, rows, V, dtype, draft_ids, q_logprobs, m.mode, m.temp, m.p, m.k, m.seed, m.counter, out_tokens, out_n, logprobs_rows, nullptr,
                                        nullptr, verify_ws, s, st);
    return spec_verify_sampled_launch(logits, rows, V, dtype, draft_ids, m.mode, m.temp, m.p, m.k, m.seed, m.counter, m.on() ? d->tail.xtc.record : nullptr, out_tokens, out_n,
                                      logprobs_rows, verify_ws, s, st, kind == SPEC_DFA ? &f : nullptr);
}

extern "C" {

int pie_decoder_spec_step(pie_decoder *d, const int32_t *draft_ids, int n_draft, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows, void *workspace,
                          int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream) {
    return spec_step("pie_decoder_spec_step", SPEC_RAW, d, draft_ids, n_draft, nullptr, out_tokens, out_n, logprobs_rows, workspace, seq_ids, seq_cap, seq_len, stream);
}

int pie_decoder_spec_step_tail(pie_decoder *d, const int32_t *draft_ids, int n_draft, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows, void *workspace,
                               int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream) {
    return spec_step("pie_decoder_spec_step_tail", SPEC_TAIL, d, draft_ids, n_draft, nullptr, out_tokens, out_n, logprobs_rows, workspace, seq_ids, seq_cap, seq_len, stream);
}

int pie_decoder_spec_step_dfa(pie_decoder *d, const int32_t *draft_ids, int n_draft, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows, void *workspace,
                              int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream) {
    return spec_step("pie_decoder_spec_step_dfa", SPEC_DFA, d, draft_ids, n_draft, nullptr, out_tokens, out_n, logprobs_rows, workspace, seq_ids, seq_cap, seq_len, stream);
}

int pie_decoder_spec_step_draft(pie_decoder *d, const int32_t *draft_ids, int n_draft, const float *q_logprobs, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows,
                                void *workspace, int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream) {
    PIE_REQUIRE(q_logprobs, PIE_E_ARG, "pie_decoder_spec_step_draft: null pointer");
    PIE_REQUIRE(pie_aligned(q_logprobs, 4), PIE_E_ALIGN, "pie_decoder_spec_step_draft: 4-byte alignment required");
    return spec_step("pie_decoder_spec_step_draft", SPEC_DRAFT, d, draft_ids, n_draft, q_logprobs, out_tokens, out_n, logprobs_rows, workspace, seq_ids, seq_cap, seq_len, stream);
}

}  // extern "C"
