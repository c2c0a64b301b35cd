// count_penalty.hpp -- frequency and presence penalties over the counts of a request's generated tokens (include/pie_hip.h, "frequency and
// presence penalties"): logits[v] = T(f32(logits[v]) - (freq * (float)counts[v] + pres)) wherever counts[v] > 0.
//
// One kernel for the multi-sequence passes (a row per blockIdx.y, its source row, position and input id found as k_logits_penalty_rows
// finds them), the op (the same, or ctx == nullptr: every row live, nothing counted) and the single-sequence step (rows == 1, position and
// input id from the decoder's DecState).
//
// Geometry: 128 threads x 4 elements = 512 elements per workgroup.  A one-row launch at V = 128256 is then 251 workgroups, one per CU of a
// 256-CU device; 256 threads x 8 elements (a 16-byte logits access per thread) would make it 63.  Chosen by that reasoning -- the row is
// 0.77 MB, so the one-row launch should sit at the launch floor either way -- and NOT by measurement: no other chunk size was timed, and
// neither was storing only the changed elements against storing the whole slot (a slot is stored when any of its elements changed).
// What is measured is this geometry alone (3.4 us at 1 and 8 rows, 6.1 us at 32).
// A thread's slot is 4 consecutive elements starting at a multiple of 4 PAST the row's head h (the 0..3 elements in front of the first
// 8-byte-aligned logit; s * V * 2 bytes is 8-aligned for V = 128256 and is not for odd V).  The counts row starts s * V * 4 bytes in: its
// element h is 16-byte aligned exactly when the logits' is 8-byte aligned, given aligned bases -- checked, not assumed: otherwise the whole row
// runs on the scalar body.  Slot 0 is the head, the last slot the tail; both run the scalar body.
#pragma once
#include "common.hpp"
#include "attention.hpp"  // DecState

constexpr int CNT_THREADS = 128, CNT_VEC = 4;

struct CountPenArgs {
    u16 *logits;  // [rows, V]
    int V, n_src;
    pie_count_penalty *records;  // [rows]
    int *counts;                 // [rows, V]
    const int *ids, *ctx, *out_rows;  // the passes' form; ctx == nullptr: every row live, nothing counted
    const DecState *state;            // the step's form (rows == 1): pos and the input id
    int count;                        // the step's form: the row's input is the state's token (a step, not a prompt pass)
};

template <class T>
__device__ __forceinline__ u16 count_penalty_value(u16 x, int c, float freq, float pres) {
    return T::from_f32(__fsub_rn(T::to_f32(x), __fadd_rn(__fmul_rn(freq, (float)c), pres)));
}

template <class T>
__global__ void __launch_bounds__(CNT_THREADS) k_logits_count_penalty_rows(const CountPenArgs a) {
    const int s = blockIdx.y;
    int pos = 0, id = -1;
    bool counting = false;
    if (a.state) {
        pos = a.state->pos, id = a.state->token, counting = a.count != 0;
        if (pos < 0) return;  // block-uniform, like every return down to the slot's bounds
    } else if (a.ctx) {
        const int i = a.out_rows ? a.out_rows[s] : s;
        if (i < 0 || i >= a.n_src) return;
        pos = a.ctx[i] - 1;
        if (pos < 0) return;  // an idle slot
        id = a.ids[i], counting = true;
    }
    pie_count_penalty *rec = a.records + s;
    const float freq = rec->freq, pres = rec->pres;
    if (freq == 0.0f && pres == 0.0f) return;
    const int V = a.V;
    u16 *lg = a.logits + (size_t)s * V;
    int *cn = a.counts + (size_t)s * V;
    int h = (int)(((8u - (unsigned)(reinterpret_cast<uintptr_t>(lg) & 7u)) & 7u) >> 1);  // elements in front of the first 8-byte-aligned logit
    const bool vec = (reinterpret_cast<uintptr_t>(lg) & 1u) == 0 && (reinterpret_cast<uintptr_t>(cn + h) & 15u) == 0;
    if (!vec) h = 0;
    const int j = blockIdx.x * CNT_THREADS + threadIdx.x;  // slot 0: the head [0, h); slot j >= 1: [h + 4 (j - 1), h + 4 j)
    if (j > (V + CNT_VEC - 1) / CNT_VEC) return;           // (also keeps 4 * j inside int)
    const int lo = j == 0 ? 0 : h + CNT_VEC * (j - 1);
    const int hi = min(V, j == 0 ? h : lo + CNT_VEC);
    if (lo >= hi) return;
    // the one thread of the launch whose slot holds element `id` counts the row's input id (and is the only one to touch counted_pos)
    const bool bump = counting && id >= lo && id < hi && pos >= rec->start && pos > rec->counted_pos;
    if (vec && j > 0 && hi - lo == CNT_VEC) {
        const uint2 x = *reinterpret_cast<const uint2 *>(lg + lo);
        const int4 c4 = *reinterpret_cast<const int4 *>(cn + lo);
        int c[CNT_VEC] = {c4.x, c4.y, c4.z, c4.w};
        u16 e[CNT_VEC] = {(u16)(x.x & 0xffffu), (u16)(x.x >> 16), (u16)(x.y & 0xffffu), (u16)(x.y >> 16)};
        bool changed = false;
#pragma unroll
        for (int k = 0; k < CNT_VEC; ++k) {
            if (bump && lo + k == id) {
                c[k] = (int)((unsigned)c[k] + 1u);
                cn[id] = c[k];
            }
            if (c[k] > 0) e[k] = count_penalty_value<T>(e[k], c[k], freq, pres), changed = true;
        }
        if (changed) *reinterpret_cast<uint2 *>(lg + lo) = make_uint2((u32)e[0] | ((u32)e[1] << 16), (u32)e[2] | ((u32)e[3] << 16));
    } else {
        for (int v = lo; v < hi; ++v) {
            int c = cn[v];
            if (bump && v == id) c = (int)((unsigned)c + 1u), cn[v] = c;
            if (c > 0) lg[v] = count_penalty_value<T>(lg[v], c, freq, pres);
        }
    }
    if (bump) rec->counted_pos = pos;
}

static inline int logits_count_penalty_rows_launch(int dtype, const CountPenArgs &a, int rows, hipStream_t st) {
    const int slots = (a.V + CNT_VEC - 1) / CNT_VEC + 1;
    const dim3 grid((slots + CNT_THREADS - 1) / CNT_THREADS, rows);
    return launch_for_dtype(dtype, "logits count penalty:", [&](auto t) { hipLaunchKernelGGL(k_logits_count_penalty_rows<decltype(t)>, grid, dim3(CNT_THREADS), 0, st, a); });
}
