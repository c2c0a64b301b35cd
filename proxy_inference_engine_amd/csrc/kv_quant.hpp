// kv_quant.hpp -- the quantized KV cache's decode attention arguments and launchers (kv_quant.hip), shared with the decoder.
#pragma once
#include "attention.hpp"

// Arguments of the quantized decode attention (one query row; GQA: q-head h reads kv-head h / REP).
struct QAttnArgs {
    const u16 *q;  // [Hq, D] T
    const u32 *kc, *vc;  // [Hkv, cap, D*BITS/32]
    const u16 *ks, *kb, *vs, *vb;  // [Hkv, cap, D/gs] T
    const DecState *state;  // nullable: T = state->pos + 1, cap = state->cap (decoder)
    int T, cap, gs;
    int Hq, Hkv, splits;
    float scale;
    float *part_acc, *part_ml;  // [Hq, splits, D], [Hq, splits, 2] -- the k_attn_decode partial format
    // decoder: staging block of the q|k|v epilogue, K [Hkv, 64, D] then V [Hkv, 64, D] T; the new position's row sits at slot pos % 64.
    // nullptr = the cache already holds every attended row (op level)
    const u16 *stage;
};

// The formats this path takes (bits 4 / 8, group 32 / 64 / 128 dividing head_dim 64 / 128, bf16 / f16): PIE_OK or a refusal with pie_last_error.
int kv_quant_check(const char *who, int dtype, int D, int group_size, int bits);
// combine = false leaves the partials for the o_proj prologue (decoder, short caches); true merges them into `out` (k_attn_combine).
int attn_decode_quant_launch(int dtype, int D, int bits, const QAttnArgs &a, bool combine, u16 *out, hipStream_t st);

// One layer's quantized K / V buffers (the six pointers of pie_decoder_set_kv_quant).
struct QKvLayer {
    const u32 *kc;
    const u16 *ks, *kb;
    const u32 *vc;
    const u16 *vs, *vb;
};
// The prompt path's two steps on a quantized layer (prefill.hip): dequant = rows [0, state->pos) of every kv-head into the T scratch
// sk / sv [Hkv, cap, D]; otherwise rows [pos, pos + M) of the scratch -> codes, and their dequantized values back into the scratch.
int kv_quant_prefill_launch(int dtype, int D, int bits, bool dequant, const QKvLayer &lay, const DecState *state, int Hkv, int cap, int M, int gs,
                            u16 *sk, u16 *sv, hipStream_t st);
