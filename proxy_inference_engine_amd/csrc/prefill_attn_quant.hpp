// prefill_attn_quant.hpp -- the launch of prefill_attn_quant.hip: causal attention of M query rows straight from the quantized KV cache
// (QuantizedKVCache, kv_quant.hpp), on the MFMA units, split over keys where the launch has too few query tiles.
#pragma once
#include "kv_quant.hpp"

constexpr int PREFILL_QUANT_TARGET_WGS = 256;     // workgroups the split rule fills a launch up to: one per CU (DESIGN.md 30's measurement on T pages)
constexpr int PREFILL_QUANT_MIN_SPLIT_BLOCKS = 4;  // the rule leaves a split at least this many 32-key blocks (two 64-key pages)
constexpr size_t PREFILL_QUANT_WS_CAP = (size_t)64 << 20;  // the rule never asks for more partials than this

struct PrefillQuantArgs {
    const u16 *q;           // [M, Hq, D] T
    QKvLayer kv;            // codes u32 [Hkv, cap, D*bits/32], scales / biases T [Hkv, cap, D/gs]; rows [0, offset + M) are attended
    const DecState *state;  // nullable: offset = state->pos (decoder); the capacity stays the host's `cap`
    int offset, cap, gs;
    int M, Hq, Hkv;
    float scale;
    int splits;             // >= 1: contiguous runs of whole 32-key blocks of the keys a query tile sees
    u16 *out;               // [M, Hq, D] T
    float *part_acc;        // splits > 1: [M, Hq, splits, D] fp32 ...
    float *part_ml;         // ... and [M, Hq, splits, 2] = (max, sum)
};

// The rule: 1 split while the query tiles x Hkv reach PREFILL_QUANT_TARGET_WGS, else enough to reach it; never more than
// ATTN_MAX_SPLITS, than the 32-key blocks of offset + M over PREFILL_QUANT_MIN_SPLIT_BLOCKS, or than PREFILL_QUANT_WS_CAP holds at head_dim 128.
int prefill_attn_quant_splits(int M, int offset, int Hq, int Hkv);
size_t prefill_attn_quant_workspace_bytes(int M, int Hq, int D, int splits);  // 0 for one split
// The attention launch, and the merge of its rows when a.splits > 1.
int prefill_attn_quant_launch(int dtype, int D, int bits, const PrefillQuantArgs &a, hipStream_t st);
