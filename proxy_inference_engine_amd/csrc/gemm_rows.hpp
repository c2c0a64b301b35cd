// gemm_rows.hpp -- what the many-row GEMM family of w4m_gemm.hip and its callers (prefill.hip, vision.hip, tools/*_bench) declare for each
// other: the types that cross the translation units and the prototypes.  Declarations only, no kernels.
#pragma once

#include "prefill_attn.hpp"  // u16, DecState

// Arguments of the q|k|v epilogue: RoPE on the q and k pairs and the cache append, exactly k_rope_append_rows (prefill.hip).  Passed by value
// into k_w4m_gemm / k_w4r_gemm and filled in by the many-row passes of prefill.hip.
struct W4mRope {
    const float *rope_cs;               // [M, HD / 2, 2] (cos, sin) of every row's position (k_rope_cs_rows)
    const DecState *state;              // single sequence: row m sits at state->pos + m, cache capacity state->cap ...
    const int *ctx_len;                 // ... or a batch of sequences: row m at ctx_len[m] - 1 (< 0: idle slot)
    const unsigned long long *kv_table; // per-layer K / V buffer (or slab) bases ...
    u16 *slab;                          // ... or this layer's slab directly (batch)
    const int *block_table;             // paged KV (nullable): table row m * bt_stride
    int bt_stride, n_pages, layer, n_layers, n_heads, n_kv_heads, HD, traditional;
    u16 *q_out;                         // [M, n_heads, HD]
    const u16 *bias;                    // the Linear's bias (packed order), nullable: filled in by the launch that takes the epilogue
    size_t i8_page_bytes;               // != 0 (with slab): the pages are int8 with per-head fp16 scales (paged_i8.hip): K / V are quantised on the way in
};

// A K-split many-row GEMM leaves S fp32 partial slabs [S][M][N]; its consumer can form the Linear's output itself -- the slabs summed in
// slab order, then the one rounding to T: exactly k_w4l_reduce's arithmetic -- which saves that launch and the round trip of y through
// memory (prompts of 33..~700 rows split K; a launch is ~5 us of a 150-300 us layer there).
struct W4lSlabs {
    const float *part = nullptr;
    int S = 0;
    size_t MN = 0;
};

// The epilogues of the int4 kernels, as a caller wishes them and as a launch reports them.  (The W4R_ names: k_w4r_gemm switches on all four at
// run time; k_w4m_gemm takes the first three as its `swiglu` argument.)
enum W4Epi {
    W4R_STORE = 0,   // y [M, N] = T(x . W^T)
    W4R_SWIGLU = 1,  // the packed gate|up matrix: act [M, N / 2] = T(T(silu(g)) * u), no y
    W4R_ROPE = 2,    // the packed q|k|v matrix: q rotated into W4mRope::q_out, k / v rotated and appended to the cache, no y
    W4R_SLAB = 3     // kernel-side only: un-rounded fp32 slabs of a K split
};

// What an int4 launch did.
struct W4Outcome {
    int epi = W4R_STORE;     // the epilogue that ran: the wish, or W4R_STORE where the route declined it (y holds the product then)
    int slabs = 0;           // > 1: y was NOT written, the workspace holds that many fp32 slabs [slabs][M][N]; 0: y (or act, or the cache) was written
    bool bias_done = false;  // the Linear's bias is already in the result; otherwise it is the caller's (bias_rows) or, with slabs, the consumer's
};

// One many-row int4 g=64 Linear on its W4M tiles: y [M, N] = x [M, K] . W^T (+ bias); N % 32 == 0, K % 64 == 0.
struct W4Rows {
    int dtype;
    const void *w4m, *x;
    int M, N, K;
    void *y;
    const void *bias = nullptr;  // the Linear's (nullable)
    int wish = W4R_STORE;        // W4R_SWIGLU into `act`, W4R_ROPE with `rope`; a route may decline (W4Outcome::epi)
    void *act = nullptr;
    W4mRope *rope = nullptr;     // (its bias field is set here when the epilogue is taken)
    bool take_slabs = false;     // the caller's consumer sums the fp32 slabs of a K split (and adds the bias) itself
    bool few_rows = false;       // the few-row kernel may serve the rows k_w4r_gemm does not take (up to PIE_KNOB_SMALL_M of them)
    bool abi_rows = false;       // pie_qgemm_w4m's rule instead: the few-row kernel up to 32 rows, whatever the knob says
};
size_t w4_rows_workspace_bytes(const W4Rows &q);  // of device scratch for w4_rows_launch (0: none needed)
int w4_rows_launch(const W4Rows &q, void *workspace, hipStream_t st, W4Outcome *done);

// The three kernel families behind that entry (w4m_gemm.hip; the bench tools call them one by one).  y / act / rope by epilogue as above.
int w4m_gemm_launch(int dtype, const void *w4m, const void *x, int M, int N, int K, void *y, hipStream_t st, int epi, const void *bias, const W4mRope *rope);
int w4l_gemm_launch(int dtype, const void *w4m, const void *x, int M, int N, int K, void *y, void *workspace, hipStream_t st, void *act, bool take_slabs,
                    W4Outcome *done);
int w4r_gemm_launch(int dtype, const void *w4m, const void *x, int M, int N, int K, void *y, void *workspace, hipStream_t st, int epi, const void *bias,
                    const W4mRope *rope, bool take_slabs, W4Outcome *done, bool wide_scales);
size_t w4l_workspace_bytes(int M, int N, int K);
bool w4r_serves(int M, int N, int K);
int w4r_splits(int M, int N, int K);
size_t w4r_workspace_bytes(int M, int N, int K);

// W4M tiles (32 rows x 64 columns, 0.5625 B per weight) from the W4S stream
size_t w4m_bytes(int N, int K);
int w4m_repack_launch(const void *w4s, int N, int K, void *w4m, hipStream_t st);
bool w4m_wide_scales(const void *w4m);

// The 16-bit many-row MFMA GEMM on W16M tiles (w16_gemm.hpp; weights in MFMA A-fragment order)
size_t w16m_size(int N, int K);
int w16m_from_rows_launch(const void *w, int N, int K, void *w16m, hipStream_t st);
int w16m_from_w16s_launch(const void *w16s, int N, int K, void *w16m, hipStream_t st);
size_t w16l_workspace_bytes(int M, int N, int K);
int w16l_gemm_launch(int dtype, const void *w16m, const void *x, int ldx, int M, int N, int K, void *y, void *workspace, hipStream_t st, const void *bias,
                     void *swiglu_act, bool *fused, int ldy);

int bias_any_launch(int dtype, void *y, const void *bias, int M, int N, hipStream_t st);  // vision.hip: y += bias, any N
