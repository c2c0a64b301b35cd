// prefill_attn_paged.hpp -- the launch of prefill_attn_paged.hip: prompt chunks that continue a cached prefix, on T pages, all chunks of a
// pass in one split-KV launch.
#pragma once
#include "common.hpp"

constexpr int PREFILL_PAGED_MAX_CHUNKS = 32;  // chunk descriptors one launch carries by value in its kernel arguments (640 bytes)
constexpr int PREFILL_PAGED_TARGET_WGS = 256;  // workgroups the split rule fills a launch up to: one per CU (DESIGN.md 30 has the measurement against 512 and 1024)
constexpr int PREFILL_PAGED_MIN_SPLIT_PAGES = 2;  // the rule leaves a split at least this many pages of the longest chunk (one-page splits lose to no split, measured)
constexpr size_t PREFILL_PAGED_WS_CAP = (size_t)64 << 20;  // the rule (and the decoder's knob) never asks for more partials than this

struct PrefillPagedArgs {
    const u16 *q;             // [N, Hq, D]
    const u16 *slab;          // a layer's T pages: K block then V block, each [Hkv, 64, D]
    const int *block_tables;  // [n_seqs, bt_stride]
    u16 *out;                 // [N, Hq, D]: the chunks' rows are written, no other
    int Hq, Hkv, bt_stride, n_pages;
    float scale;
    int splits;               // >= 1: contiguous runs of whole pages of the keys a query tile sees
    float *part_acc;          // splits > 1: [chunk rows, Hq, splits, D] fp32, the chunks' rows only, in the order of the chunk array ...
    float *part_ml;           // ... and [chunk rows, Hq, splits, 2] = (max, sum)
};

// chunks: HOST int32 [n_chunks][4] = {first row, rows M, cached positions P, block-table row}, checked by the caller.
// The rule: 1 split while the launch's query tiles x Hkv reach PREFILL_PAGED_TARGET_WGS, else enough to reach it; never more than ATTN_MAX_SPLITS,
// than the pages of the longest chunk over PREFILL_PAGED_MIN_SPLIT_PAGES, or than PREFILL_PAGED_WS_CAP of partials holds at head_dim 128.
// force > 0 (PIE_KNOB_CHUNK_SPLITS): that count, at most ATTN_MAX_SPLITS, the pages of the longest chunk and what PREFILL_PAGED_WS_CAP holds.
int prefill_attn_paged_splits(const int32_t *chunks, int n_chunks, int Hkv, int rep, int force = 0);
size_t prefill_attn_paged_workspace_bytes(const int32_t *chunks, int n_chunks, int Hq, int D, int splits);  // 0 for one split
// One launch per 32 chunks, and the merge of their rows when a.splits > 1 (a.part_acc / a.part_ml: the whole call's partials).
int prefill_attn_paged_launch(int dtype, int D, const PrefillPagedArgs &a, const int32_t *chunks, int n_chunks, hipStream_t st);
