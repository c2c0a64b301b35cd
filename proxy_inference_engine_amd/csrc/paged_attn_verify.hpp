// paged_attn_verify.hpp -- the attention of a batched speculative pass: every speculating sequence's 1..8 consecutive query
// rows against that sequence's own pages, in ONE launch per layer (plus one merge launch when the positions are split).  For callers
// inside the library (prefill.hip: pie_decoder_spec_step_batch); the op-level entry is pie_paged_attn_verify (paged_attn_verify.hip).
#pragma once
#include "attention.hpp"
#include "common.hpp"

constexpr int VERIFY_MAX_SEG_ROWS = 8;  // rows of one sequence in a pass: the fed token and up to 7 drafts

struct VerifyAttnArgs {
    const u16 *q;            // [N, Hq, D]
    const u16 *slab;         // the layer's T pages: K block then V block per page, each [Hkv, 64, D]
    const int *block_table;  // [B, bt_stride]
    const int *row_seq;      // [N]: the block-table row of row r's sequence
    const int *row_ctx;      // [N]: the positions row r attends, its own included
    const int *seg_first;    // [B + 1]: segment s = rows seg_first[s] .. seg_first[s + 1] - 1 (at most 8; none: an idle slot)
    int N, B, Hq, Hkv, bt_stride, n_pages, splits;
    float scale;
    float *part_acc;  // [N, Hq, splits, D]   (splits > 1)
    float *part_ml;   // [N, Hq, splits, 2]
    u16 *out;         // [N, Hq, D]
};

// splits for B segments over tables of max_blocks pages: enough workgroups for two per CU, never more than pages per sequence
int paged_attn_verify_splits(int B, int Hkv, int max_blocks);
// arguments already checked; D 64 / 128, Hq / Hkv 1..8
int paged_attn_verify_launch(int dtype, int D, const VerifyAttnArgs &a, hipStream_t st);
