// speculative.hpp -- what speculative.hip shares with callers inside the library (prefill.hip's batched passes): the limits, the carve
// helper every speculative workspace is laid out with, the pass workspace, the decoder-side commit target and the verifies' launchers.
// The shared parts are described once at the head of speculative.hip.
#pragma once
#include "attention.hpp"  // DecState
#include "common.hpp"

constexpr int SPEC_MAX_ROWS = 32;   // rows of one verify pass: the fed token and up to 31 drafts
constexpr int SPEC_MAX_NGRAM = 8;   // the drafter's longest suffix
constexpr int SPEC_MAX_IDS = 1 << 27;  // the drafter's search key packs (match length, end position) into 32 bits
constexpr int SPEC_SEG_ROWS = 8;    // rows of one sequence in a batched pass: the fed token and up to 7 drafts
constexpr int SPEC_MAX_SEQS = 4096;  // sequences of one pie_ngram_draft_rows / pie_spec_verify_rows call
constexpr int SPEC_BATCH_ROWS = 256;  // rows of one batched pass: one tile of the streaming GEMM

// A bump allocator over a workspace: take() returns the offset of the next part, take16() of the next part on a 16-byte boundary.
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += bytes;
        return o;
    }
    size_t take16(size_t bytes) {
        at = align16(at);
        return take(bytes);
    }
};

// The workspace of every pass entry (pie_decoder_spec_step*, pie_decoder_spec_step_batch*): the logits block [logit_rows, V] T at its head |
// the pass's input ids [fed_slots] | the verify's own workspace.
struct SpecPassLayout {
    size_t fed, verify;
    SpecPassLayout(int logit_rows, int fed_slots, int V) {
        Carve c;
        c.take((size_t)logit_rows * V * 2);
        fed = c.take16(sizeof(int) * (size_t)fed_slots);
        verify = c.take16(0);
    }
    // the whole workspace with `verify_bytes` behind it; 0 when the verify refuses the block (verify_bytes == 0)
    size_t bytes(size_t verify_bytes) const { return verify_bytes ? verify + verify_bytes : 0; }
};

// What the accept launch does besides the op's outputs when the block came from the decoder's own pass (all device memory; state == nullptr:
// the op alone).  Before the launch state->pos = o + rows and the pass's tail has run; after it the decoder is where `n` greedy steps from
// position o would have left it: pos = o + n, token = the last accepted token, history[o + 1 + i] = accepted token i.  seq_ids (nullable,
// [seq_cap]) = the sequence's ids by position, made whole here: seq_ids[o] = fed[0] (the fed-back token of row 0) and seq_ids[o + 1 + i] =
// accepted token i; seq_len (nullable) = o + n + 1, the drafter's `len` for the next draft.  token_out (nullable): the bound token output.
// ids_by_pos (nullable, [ids_cap]; pie_decoder_spec_step_tail and pie_decoder_spec_step_draft): the repetition penalty's ids by position, ids_by_pos[o + 1 + i] = accepted
// token i, so that the plain step that follows finds its window whole.
struct SpecState {
    DecState *state = nullptr;
    int *history = nullptr;
    int hist_cap = 0;
    const int *fed = nullptr;
    int *seq_ids = nullptr;
    int seq_cap = 0;
    int *seq_len = nullptr;
    int *token_out = nullptr;
    int *ids_by_pos = nullptr;
    int ids_cap = 0;
};

// the op's three launches (arguments already checked)
int spec_verify_launch(const u16 *logits, int rows, int V, int dtype, const int *draft, int *out_tokens, int *out_n, float *logprobs, void *workspace,
                       const SpecState &s, hipStream_t st);

// The batched pass (pie_decoder_spec_step_batch in prefill.hip).  pie_spec_verify_rows' three launches (arguments already
// checked): segment s = rows seg_first[s] .. seg_first[s + 1] - 1 of logits [N, V] against draft [B, draft_stride]; ids / len nullable.
int spec_verify_rows_launch(const u16 *logits, int N, int V, int dtype, const int *seg_first, int B, const int *draft, int draft_stride, int *out_tokens,
                            int *out_n, int *ids, int *len, int cap, void *workspace, hipStream_t st);
// The batched pass under per-seat tails (pie_decoder_spec_step_batch_tail in prefill.hip).  What the seats own, all device
// memory: record, ring, bias entries and XTC record s belong to segment s.  Exactly one of pos0 [B] (the op) and row_ctx [N] (the decoder's
// row_context_lens: segment s starts at position row_ctx[its first row] - 1) is given; the bias part and xtc are nullable.
struct SpecSeats {
    pie_row_tail *table = nullptr;
    int *recent = nullptr;
    const int *pos0 = nullptr, *row_ctx = nullptr;
    const int *bias_ids = nullptr;
    const float *bias_vals = nullptr;
    const int *bias_n = nullptr;
    int bias_cap = 0;
    const pie_xtc *xtc = nullptr;
};
// pie_spec_verify_rows_sampled's launches (arguments already checked); logits are edited in place, logprobs [N, V] are required
int spec_verify_rows_sampled_launch(const SpecSeats &q, u16 *logits, int N, int V, int dtype, const int *seg_first, int B, const int *fed, const int *draft,
                                    int draft_stride, int *out_tokens, int *out_n, float *logprobs, int *ids, int *len, int cap, void *workspace, hipStream_t st);
// fed [N] = the pass's input ids: every segment's fed token (tokens [B]), then its drafts
int spec_gather_rows_launch(const int *tokens, const int *draft, int draft_stride, const int *seg_first, int B, int N, int vocab, int *fed, hipStream_t st);
