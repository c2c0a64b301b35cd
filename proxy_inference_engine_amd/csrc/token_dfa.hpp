// token_dfa.hpp -- the device-side token automaton (include/pie_hip.h, "token automaton"): a grammar as a token-level DFA
// compressed by token classes.  An automaton is V + S * C consecutive int32 words inside a caller-owned arena `tables` [tables_len]:
// cls [V] (token id -> class), then trans [S, C] (next state, -1: not allowed).  Two ops over rows of (record, state):
//   mask     the row's token mask in the tail's bit layout (token i = bit i & 31 of word i >> 5), derived from its state
//   advance  the row's state moved by the token that was drawn
// The record, the state, the class array and the table are device memory that the host rewrites between launches and are NOT trusted:
// a record is armed only when both of its ranges lie inside the arena (dfa_armed), a class is used only inside [0, C), a state only inside
// [0, S) -- so every index below is bounded by tables_len whatever the memory holds.
#pragma once
#include "common.hpp"

__device__ __forceinline__ bool dfa_armed(const pie_row_dfa &r, int V, int tables_len) {
    return r.n_states > 0 && r.n_classes > 0 && r.cls_off >= 0 && r.trans_off >= 0 && (long long)r.cls_off + V <= (long long)tables_len &&
           (long long)r.trans_off + (long long)r.n_states * (long long)r.n_classes <= (long long)tables_len;
}

enum { DFA_UNARMED = 0, DFA_MASKED = 1, DFA_LEFT = 2 };

// Workgroup (blockIdx.x, row blockIdx.y) tests ids blockIdx.x * 256 .. + 255, a wave 64 consecutive ids from a multiple of 64: a coalesced
// cls load, a gather from the state's one trans row, one 64-bit ballot whose two words lanes 0 and 32 store -- each only below
// ceil(V / 32), so a canary behind the row's words survives, and with the bits at or beyond V zero.  One thread reads the record and the
// state and the workgroup takes them from LDS: what it does is block-uniform by construction (tail.hpp: k_logits_stats_rows_masked).
static __global__ void __launch_bounds__(256) k_token_dfa_mask(const pie_row_dfa *records, const int *states, const int *tables, int tables_len, int V,
                                                        unsigned *masks, int mask_words, int *mask_on) {
    __shared__ int s_kind, s_cls_off, s_row_off, s_C;
    const int row = blockIdx.y;
    if (threadIdx.x == 0) {
        const pie_row_dfa r = records[row];
        const int s = states[row];
        int kind = DFA_UNARMED;
        if (dfa_armed(r, V, tables_len)) {
            kind = s >= 0 && s < r.n_states ? DFA_MASKED : DFA_LEFT;
            s_cls_off = r.cls_off, s_C = r.n_classes;
            s_row_off = kind == DFA_MASKED ? r.trans_off + s * r.n_classes : 0;  // < trans_off + S * C <= tables_len: fits an int
            if (mask_on && blockIdx.x == 0) mask_on[row] = kind == DFA_MASKED;
        }
        s_kind = kind;
    }
    __syncthreads();
    const int kind = s_kind;
    if (kind == DFA_UNARMED || (kind == DFA_LEFT && mask_on)) return;  // nothing of the row's words is written
    const int id = blockIdx.x * 256 + threadIdx.x;
    bool ok = id < V;
    if (ok && kind == DFA_MASKED) {
        const int c = tables[s_cls_off + id];
        ok = c >= 0 && c < s_C && tables[s_row_off + c] >= 0;
    }
    const unsigned long long bits = __ballot(ok);
    const int lane = threadIdx.x & 63, word = (id >> 5);  // lane 0: the wave's first word, lane 32: its second
    if ((lane & 31) == 0 && word < (V + 31) / 32) masks[(size_t)row * mask_words + word] = (unsigned)(lane ? bits >> 32 : bits);
}

// One thread per row.
static __global__ void __launch_bounds__(64) k_token_dfa_advance(const pie_row_dfa *records, int *states, const int *tables, int tables_len, int rows, int V,
                                                          const int *tokens) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    const pie_row_dfa r = records[row];
    if (!dfa_armed(r, V, tables_len)) return;
    const int s = states[row];
    if (s < 0 || s >= r.n_states) return;  // left or finished: stays what it is
    const int t = tokens[row];
    int next = -1;
    if (t >= 0 && t < V) {
        const int c = tables[r.cls_off + t];
        if (c >= 0 && c < r.n_classes) next = tables[r.trans_off + s * r.n_classes + c];
    }
    states[row] = next;
}

// ---------------------------------------------------------------- the automaton along a draft
constexpr int DFA_MAX_DRAFT = 31;  // a speculative pass's drafts (speculative.hpp: SPEC_MAX_ROWS - 1)

// pie_token_dfa_advance's rule for one armed record: the state after `t`, from state s in [0, S)
__device__ __forceinline__ int dfa_next(const pie_row_dfa &r, const int *tables, int V, int s, int t) {
    if (t < 0 || t >= V) return -1;
    const int c = tables[r.cls_off + t];
    return c >= 0 && c < r.n_classes ? tables[r.trans_off + s * r.n_classes + c] : -1;
}

// The class of id t under an armed record, -1 for an id outside [0, V) or a class outside [0, C)
__device__ __forceinline__ int dfa_class(const pie_row_dfa &r, const int *tables, int V, int t) {
    if (t < 0 || t >= V) return -1;
    const int c = tables[r.cls_off + t];
    return c >= 0 && c < r.n_classes ? c : -1;
}

// One wave.  Lane i loads the class of tokens[i] -- n independent loads -- and lane 0 then walks: one dependent trans load per position.
// out_states[0] = *state, out_states[i + 1] = the advance op's result for out_states[i] and tokens[i]; a state outside [0, S) stays what
// it is and an unarmed record copies *state to every slot.  rep / mask_on (nullable, the speculative pass's): the record once per state
// for the mask op's per-row form, and mask_on zeroed in front of it -- the mask op writes only an armed row's entry.
static __global__ void __launch_bounds__(64) k_token_dfa_walk(const pie_row_dfa *record, const int *state, const int *tables, int tables_len, int V,
                                                       const int *tokens, int n, int *out_states, pie_row_dfa *rep, int *mask_on) {
    __shared__ int s_cls[DFA_MAX_DRAFT];
    const int lane = threadIdx.x;
    const pie_row_dfa r = *record;
    const bool armed = dfa_armed(r, V, tables_len);
    if (lane < n) s_cls[lane] = armed ? dfa_class(r, tables, V, tokens[lane]) : -1;
    if (lane <= n) {
        if (rep) rep[lane] = r;
        if (mask_on) mask_on[lane] = 0;
    }
    __syncthreads();
    if (lane != 0) return;
    int s = *state;
    out_states[0] = s;
    for (int i = 0; i < n; ++i) {
        if (armed && s >= 0 && s < r.n_states) s = s_cls[i] >= 0 ? tables[r.trans_off + s * r.n_classes + s_cls[i]] : -1;
        out_states[i + 1] = s;
    }
}

// The grammar-aware drafter (include/pie_hip.h: pie_token_dfa_draft has the rule).  One wave: lane i holds candidate i and its class --
// loaded before anything is stored, so out_ids may be cand and out_count cand_count -- and lane 0 then walks.  `forced` is a hint: an
// entry is used only when the tables re-derive it (0 <= f < V, trans[s, cls[f]] == next >= 0), so whatever it holds, every id written is
// allowed in the state the ids before it lead to.  forced[next] is requested before the re-derivation of forced[s] is waited for: a forced
// step's dependent chain is cls[f] -> trans[s, .], not forced[s] -> cls[f] -> trans[s, .].
static __global__ void __launch_bounds__(64) k_token_dfa_draft(const pie_row_dfa *record, const int *state, const int *tables, int tables_len, const int *forced,
                                                        int forced_states, int V, const int *cand, const int *cand_count, int k, int *out_ids, int *out_count) {
    __shared__ int s_cand[DFA_MAX_DRAFT], s_ccls[DFA_MAX_DRAFT];
    const int lane = threadIdx.x;
    const pie_row_dfa r = *record;
    const bool armed = dfa_armed(r, V, tables_len);
    int cc = *cand_count;
    cc = cc < 0 ? 0 : (cc > DFA_MAX_DRAFT ? DFA_MAX_DRAFT : cc);
    if (lane < DFA_MAX_DRAFT) {
        const int id = lane < cc ? cand[lane] : -1;
        s_cand[lane] = id, s_ccls[lane] = armed ? dfa_class(r, tables, V, id) : -1;
    }
    __syncthreads();  // every candidate is in LDS before the first store below
    if (lane != 0) return;
    const int s0 = *state, S = r.n_states, C = r.n_classes;
    if (!armed || s0 < 0 || s0 >= S) {  // an unconstrained request drafts as before
        const int n = cc < k ? cc : k;
        for (int i = 0; i < n; ++i) out_ids[i] = s_cand[i];
        *out_count = n;
        return;
    }
    const int2 *hint = reinterpret_cast<const int2 *>(forced);
    const int2 none = make_int2(-1, -1);
    int s = s0, j = 0, n = 0;
    bool live = true;
    int2 f = s < forced_states ? hint[s] : none;
    while (n < k) {
        const int row = r.trans_off + s * C;  // s in [0, S): below trans_off + S * C <= tables_len
        const bool hinted = f.x >= 0 && f.x < V && f.y >= 0;
        const int fc = hinted ? tables[r.cls_off + f.x] : -1;
        const int2 ahead = hinted && f.y < S && f.y < forced_states ? hint[f.y] : none;  // in flight while the hint is re-derived
        const bool has = live && j < cc && s_ccls[j] >= 0;
        const int cnext = has ? tables[row + s_ccls[j]] : -1;
        const bool ok = hinted && fc >= 0 && fc < C && tables[row + fc] == f.y;
        int t, nxt;
        if (ok) {
            t = f.x, nxt = f.y;
            if (live && j < cc && s_cand[j] == t) ++j;
            else live = false;
        } else if (cnext >= 0) {
            t = s_cand[j], nxt = cnext, ++j;
        } else {
            break;
        }
        out_ids[n++] = t, s = nxt;
        if (s < 0 || s >= S) break;
        f = ok ? ahead : (s < forced_states ? hint[s] : none);
    }
    *out_count = n;
}

// ---------------------------------------------------------------- checks and launchers (the ops of ops.hip and the passes' tails)
static inline int token_dfa_check(const char *who, const void *records, const void *states, const void *tables, int tables_len, int rows, int V) {
    const std::string w(who);
    PIE_REQUIRE(records && states && tables, PIE_E_ARG, w + ": null pointer");
    PIE_REQUIRE(rows >= 1 && rows <= 65535 && V >= 1 && tables_len >= 1, PIE_E_SHAPE, w + ": 1 <= rows <= 65535, V >= 1 and a non-empty arena");
    PIE_REQUIRE(pie_aligned(records, 4) && pie_aligned(states, 4) && pie_aligned(tables, 4), PIE_E_ALIGN, w + ": records, states and tables need 4-byte alignment");
    return PIE_OK;
}

static inline int token_dfa_mask_launch(const pie_row_dfa *records, const int *states, const int *tables, int tables_len, int rows, int V, unsigned *masks,
                                        int mask_words, int *mask_on, hipStream_t st) {
    hipLaunchKernelGGL(k_token_dfa_mask, dim3((V + 255) / 256, rows), dim3(256), 0, st, records, states, tables, tables_len, V, masks, mask_words, mask_on);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

static inline int token_dfa_walk_launch(const pie_row_dfa *record, const int *state, const int *tables, int tables_len, int V, const int *tokens, int n,
                                        int *out_states, pie_row_dfa *rep, int *mask_on, hipStream_t st) {
    hipLaunchKernelGGL(k_token_dfa_walk, dim3(1), dim3(64), 0, st, record, state, tables, tables_len, V, tokens, n, out_states, rep, mask_on);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

static inline int token_dfa_draft_launch(const pie_row_dfa *record, const int *state, const int *tables, int tables_len, const int *forced, int forced_states,
                                         int V, const int *cand, const int *cand_count, int k, int *out_ids, int *out_count, hipStream_t st) {
    hipLaunchKernelGGL(k_token_dfa_draft, dim3(1), dim3(64), 0, st, record, state, tables, tables_len, forced, forced_states, V, cand, cand_count, k, out_ids,
                       out_count);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

static inline int token_dfa_advance_launch(const pie_row_dfa *records, int *states, const int *tables, int tables_len, int rows, int V, const int *tokens,
                                           hipStream_t st) {
    hipLaunchKernelGGL(k_token_dfa_advance, dim3((rows + 63) / 64), dim3(64), 0, st, records, states, tables, tables_len, rows, V, tokens);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}
