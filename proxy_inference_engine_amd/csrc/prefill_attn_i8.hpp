// prefill_attn_i8.hpp -- the launch of prefill_attn_i8.hip: prompt chunks that continue a cached prefix, on int8 pages.
#pragma once
#include "common.hpp"

constexpr int PREFILL_I8_MAX_CHUNKS = 32;  // chunk descriptors one launch carries by value in its kernel arguments (512 bytes)

struct PrefillI8Chunk {
    int first, rows, cached, seq;  // first row of the batch, rows M >= 1, cached positions P >= 1, block-table row
};

struct PrefillI8Args {
    const u16 *q;             // [N, Hq, D]
    const void *slab;         // a layer's int8 pages (pie_page_i8_bytes each)
    const int *block_tables;  // [n_seqs, bt_stride]
    u16 *out;                 // [N, Hq, D]: the chunks' rows are written, no other
    int Hq, Hkv, bt_stride, n_pages;
    float scale;
};

// chunks: HOST int32 [n_chunks][4], checked by the caller (varlen_batch's chunk checks): rows inside [0, N), pages inside the block table,
// sequence inside block_tables.  One launch per 32 chunks.
int prefill_attn_i8_launch(int dtype, int D, const PrefillI8Args &a, const int32_t *chunks, int n_chunks, hipStream_t st);
