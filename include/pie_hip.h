/*
 * pie_hip.h -- C ABI of libpie_hip.so: the MI355X (gfx950) implementation of PIE's decode hot path.
 *
 * The reference (TheProxyCompany/proxy-inference-engine @ 2025-05-09) has no FFI for this path: its seam
 * is the set of MLX op call sites inside `proxy_inference_engine` (all tensor math is `import mlx.core as
 * mx`, engine/inference_engine.py:6) plus the one-symbol native module `pie_core` (hello(),
 * src/pie_core/src/bindings.cpp:6-9).  Each entry point below replaces exactly one of those call sites (or a
 * fused run of them) and cites it.  Paths are relative to /root/reference/src/proxy_inference_engine/.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch/HIP C++ types in signatures (hipStream_t travels as void*).
 *   - All data pointers are DEVICE pointers owned by the caller.  The library never allocates or frees
 *     caller tensors and keeps no reference after return, except pie_decoder_* which records the weight /
 *     KV pointers it is given (the caller keeps those alive until pie_decoder_destroy).
 *   - Every launch is asynchronous on `stream`; nothing synchronises the device.
 *   - Return value: 0 = PIE_OK, negative = PIE_E_*.  Nothing throws across the ABI.
 *     pie_last_error() returns a thread-local description of the last failure on the calling thread.
 *   - `dtype`: activation / parameter float type, PIE_BF16 or PIE_F16 (16-bit storage, fp32 accumulate).
 *   - Threading: thread-compatible (no global mutable state besides the thread-local error string); one
 *     host thread drives one decoder, like the reference's single non re-entrant InferenceEngine
 *     (server/app.py:23,35).
 */
#ifndef PIE_HIP_H
#define PIE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PIE_OK = 0, PIE_E_ARG = -1, PIE_E_SHAPE = -2, PIE_E_ALIGN = -3, PIE_E_HIP = -4, PIE_E_STATE = -5, PIE_E_ARCH = -6, PIE_E_RANGE = -7,
       PIE_EXHAUSTED = 1 /* pie_page_alloc: no free page (the reference's std::nullopt); not an error */ };
enum { PIE_BF16 = 1, PIE_F16 = 2, PIE_I8 = 3 /* KV page storage only: int8 rows + per-head fp16 scales (page pool, pie_paged_*_i8) */ };

/* pie_core.hello()  (src/pie_core/src/bindings.cpp:8; asserted by tests/python/test_basic.py:16). */
const char *pie_hello(void);
const char *pie_version(void);
const char *pie_last_error(void);
/* Fills name (<= name_len bytes, NUL-terminated gcnArchName), CU count, bytes of device memory. */
int pie_device_info(char *name, int name_len, int *n_cus, size_t *hbm_bytes);

/* Test / tuning switches (no reference counterpart).  One process-wide table; value PIE_KNOB_DEFAULT restores the built-in default.  Every knob is
 * exercised by a test (tests/test_gpu_decode.py, test_gpu_ops.py, test_gpu_paged.py compare the forms they select); none changes a result beyond
 * what its comment says.  Nothing in the library reads the environment. */
enum {
    PIE_KNOB_PREFILL_MIN = 0,        /* prompts shorter than this run as iterated decode steps (MLX's qmv regime); default 6, min 2 */
    PIE_KNOB_PREFILL_CHUNK = 1,      /* rows per prompt chunk; default 4096 (16..8192) */
    PIE_KNOB_PREFILL_RESIDENT = 2,   /* GiB budget for resident dequantised layer matrices; default: half of the free HBM; 0 = none */
    PIE_KNOB_SMALL_M = 3,            /* rows up to which int4 Linears that k_w4r_gemm does not take use the few-row kernel; default 32; 0 = the many-row tile kernel takes them */
    PIE_KNOB_W4L_SLABS = 4,          /* 0: K-split products of the int4 GEMMs reduced by their own launch instead of by their consumers (bit-equal) */
    PIE_KNOB_PREFILL_ATTN_VALU = 5,  /* 1: the VALU prompt attention instead of the MFMA flash kernel (the tests' cross-check) */
    PIE_KNOB_PREFILL_QT = 6,         /* 1 / 2: one / two 32-row query tiles per prompt-attention workgroup */
    PIE_KNOB_ATTN_MERGE_MAX_CAP = 7, /* cache capacity up to which o_proj merges the split-KV partials (read at pie_decoder_create); default 1024 */
    PIE_KNOB_ATTN_WARM_MAX_MB = 8,   /* the attention launch's idle CUs warm the Infinity Cache with at most this many MB of o_proj's weights; 0 = off (read per step enqueue / graph capture) */
    PIE_KNOB_W4R = 9,                /* 0: int4 Linears of 6..256 rows on the round-2 kernels (k_w4m_gemm, k_w4l2_gemm) instead of the weight-streaming k_w4r_gemm (the tests' cross-check) */
    PIE_KNOB_FUSE_ATTN = 10,         /* 0: the step's attention as its own launch instead of behind the q|k|v launch's XCD-local seam (32 / 8 / 128 heads; bit-identical; read per step enqueue / graph capture) */
    PIE_KNOB_ATTN_MERGE_IN_LAUNCH = 11, /* 0: the fused launch leaves the split-KV partials to o_proj's merging prologue instead of finishing every query head itself (bit-identical; read where the q|k|v launch is enqueued / captured) */
    PIE_KNOB_PREFILL_RESIDENT_KB = 12, /* the PIE_KNOB_PREFILL_RESIDENT budget in KiB; set (>= 0) it takes precedence.  It exists so that tests can admit some matrices of a small model and refuse others */
    PIE_KNOB_COUNT = 13
};
#define PIE_KNOB_DEFAULT (-1)
int pie_set_knob(int knob, int value);
int pie_get_knob(int knob); /* the value set, or PIE_KNOB_DEFAULT */

/* ---------------------------------------------------------------- mx.quantize / mx.dequantize (K10)
 * Call sites: cache/kv_cache/cache.py:144-147, quantized.py:91-96; defines the checkpoint triplet
 * models/utils.py:96-111 consumes.  w [N,K] T -> codes uint32 [N,K/8], scales/biases T [N,K/64].
 * Bit-exact with the published algorithm: integer codes, T-rounded affine params. */
int pie_quantize_w4g64(const void *w, int N, int K, int dtype, uint32_t *codes, void *scales, void *biases, void *stream);
int pie_dequantize_w4g64(const uint32_t *codes, const void *scales, const void *biases, int N, int K, int dtype,
                         void *w_out, void *stream);

/* ---------------------------------------------------------------- weight streaming layout ("W4S")
 * Load-time repack of one MLX-quantised Linear (weight/scales/biases triplet, models/utils.py:96-111) into
 * the layout the GEMV streams: units of 2304 B = one ROW PAIR x one 2048-wide K slice
 * (2 x [64 lanes x 16 B] nibble-reordered codes + [64 lanes x 4 B] {scale,bias}); unit index = pair*n_slices + slice.
 * row_map (device int32 [N_out], may be NULL = identity) gives, per packed row, the source row of
 * `codes`; N_out must be even.  This is how q|k|v are concatenated with RoPE partners adjacent and
 * gate|up interleaved.  pie_w4s_bytes() is the size of `packed`. */
size_t pie_w4s_bytes(int N_out, int K);
int pie_repack_w4g64(const uint32_t *codes, const void *scales, const void *biases, int N_src, int K,
                     const int32_t *row_map, int N_out, void *packed, void *stream);

/* ---------------------------------------------------------------- mx.quantized_matmul(x, w, scales, biases,
 * transpose=True, group_size=64, bits=4) via nn.QuantizedLinear.__call__ (K1).
 * Call sites: models/llama/language.py:83 (q,k,v), :108 (o), :127 (gate,up,down), :207/:209 (lm_head).
 * x [M,K] T, packed = W4S of a [N,K] weight, lin_bias T [N] or NULL (nn.QuantizedLinear bias), y [M,N] T.
 * Row-by-row exact-fp32 arithmetic (MLX's qmv regime) for every M; the weights are streamed once per up to 5 rows of x
 * (k_w4s_gemv_rows), each row bit-identical to that row multiplied alone. */
int pie_qgemv_w4g64(const void *x, int M, const void *packed, int N, int K, const void *lin_bias, void *y,
                    int dtype, void *stream);

/* ---------------------------------------------------------------- MLX int8 group-64 checkpoints (config "quantization":
 * {"group_size": 64, "bits": 8}): weight uint32 [N, K/4] (byte i of word w = code 4w+i), scales/biases T [N, K/64].
 * Same call sites and kernel as the int4 path on "W8S" units of 4352 B (row pair x 2048-wide K slice, four 16-byte code
 * pieces per lane).  pie_quantize_g64 (bits = 2 | 4 | 6 | 8) / pie_dequantize_g64 / pie_embedding_g64 (bits = 4 | 8) are the bits-generic forms
 * of the w4g64 entry points above. */
size_t pie_w8s_bytes(int N_out, int K);
int pie_repack_w8g64(const uint32_t *codes, const void *scales, const void *biases, int N_src, int K, const int32_t *row_map,
                     int N_out, void *packed, void *stream);
int pie_qgemv_w8g64(const void *x, int M, const void *packed, int N, int K, const void *lin_bias, void *y, int dtype, void *stream);
int pie_quantize_g64(const void *w, int N, int K, int bits, int dtype, uint32_t *codes, void *scales, void *biases, void *stream);
int pie_dequantize_g64(const uint32_t *codes, const void *scales, const void *biases, int N, int K, int bits, int dtype, void *w_out,
                       void *stream);
int pie_embedding_g64(const int32_t *ids, int L, const uint32_t *codes, const void *scales, const void *biases, int V, int H,
                      int bits, int dtype, void *out, void *stream);

/* ---------------------------------------------------------------- MLX int2 group-64 checkpoints (config "quantization": {"group_size": 64 | 128,
 * "bits": 2}; models/utils.py:96-111 forwards any bits nn.quantize takes): weight uint32 [N, K/16] (code k of a word at bits [2k, 2k+2)),
 * scales / biases T [N, K/64].  Same call sites and streaming kernel on "W2S" units of 1280 B (row pair x 2048-wide K slice, ONE 16-byte code
 * piece per lane + its {scale | bias << 16}): 0.3125 B per weight in HBM, the checkpoint's own figure (round 4 streamed these as 4-bit codes,
 * 0.5625 B).  The embedding TABLE of such a checkpoint is handed to the decoder as 4-bit codes (one row per step); W2S is a Linear format. */
size_t pie_w2s_bytes(int N_out, int K);
int pie_repack_w2g64(const uint32_t *codes, const void *scales, const void *biases, int N_src, int K, const int32_t *row_map, int N_out,
                     void *packed, void *stream);
int pie_qgemv_w2g64(const void *x, int M, const void *packed, int N, int K, const void *lin_bias, void *y, int dtype, void *stream);

/* ---------------------------------------------------------------- MLX int6 group-64 checkpoints (config "quantization": {"group_size": 64 | 128,
 * "bits": 6}): weight uint32 [N, 3K/16] -- MLX's little-endian bit stream, code k of a row at bits [6k, 6k+6) -- scales / biases T [N, K/64].
 * "W6S" units of 3328 B (row pair x 2048-wide K slice): the low nibbles as the W4S unit's two code pieces, the high two bits as the W2S unit's one
 * piece, then {scale | bias << 16} per lane: 0.8125 B per weight in HBM, the checkpoint's own figure (round 4 streamed these as bytes, 1.0625 B).
 * A group's dot product = the W4S dot of the low plane + 16 x the W2S dot of the high plane.  The embedding table is handed over as 8-bit codes. */
size_t pie_w6s_bytes(int N_out, int K);
int pie_repack_w6g64(const uint32_t *codes, const void *scales, const void *biases, int N_src, int K, const int32_t *row_map, int N_out,
                     void *packed, void *stream);
int pie_qgemv_w6g64(const void *x, int M, const void *packed, int N, int K, const void *lin_bias, void *y, int dtype, void *stream);

/* ---------------------------------------------------------------- MLX group-32 checkpoints (config "quantization": {"group_size": 32,
 * "bits": 4 | 8}; nn.quantize takes any group_size in {32, 64, 128}, models/utils.py:96-111): weight uint32 [N, K*bits/32], scales / biases
 * T [N, K/32].  Same call sites and streaming kernel as the group-64 paths on "W4S32" units of 2560 B / "W8S32" units of 4608 B: the W4S / W8S
 * unit with TWO {scale | bias << 16} words per lane (its code pieces are two consecutive 32-wide groups).  Decode steps and prompts below 6
 * rows multiply in the exact-fp32 regime (one pass over the weights per row); longer prompts dequantise to a W16M copy for k_w16l_gemm. */
size_t pie_w4s32_bytes(int N_out, int K);
int pie_repack_w4g32(const uint32_t *codes, const void *scales, const void *biases, int N_src, int K, const int32_t *row_map, int N_out,
                     void *packed, void *stream);
int pie_qgemv_w4g32(const void *x, int M, const void *packed, int N, int K, const void *lin_bias, void *y, int dtype, void *stream);
size_t pie_w8s32_bytes(int N_out, int K);
int pie_repack_w8g32(const uint32_t *codes, const void *scales, const void *biases, int N_src, int K, const int32_t *row_map, int N_out,
                     void *packed, void *stream);
int pie_qgemv_w8g32(const void *x, int M, const void *packed, int N, int K, const void *lin_bias, void *y, int dtype, void *stream);
int pie_embedding_g32(const int32_t *ids, int L, const uint32_t *codes, const void *scales, const void *biases, int V, int H, int bits, int dtype, void *out,
                      void *stream);

/* ---------------------------------------------------------------- dense checkpoints (no "quantization" entry in
 * config.json, models/utils.py:96-97): nn.Linear / nn.Embedding with 16-bit weights.  Same streaming kernel as the int4
 * path on "W16S" units of 2048 B = one ROW PAIR x one 512-wide K slice (2 x [64 lanes x 16 B]); row_map as for
 * pie_repack_w4g64.  pie_gemv_dense: y[M,N] = x[M,K] @ W.T (+ bias), fp32 accumulate, one rounding
 * (call sites models/llama/language.py:83,108,127,209).  pie_embedding_dense: row gather (language.py:176). */
size_t pie_w16s_bytes(int N_out, int K);
int pie_repack_dense(const void *w, int N_src, int K, const int32_t *row_map, int N_out, void *packed, void *stream);
int pie_gemv_dense(const void *x, int M, const void *packed, int N, int K, const void *lin_bias, void *y, int dtype, void *stream);
int pie_embedding_dense(const int32_t *ids, int L, const void *table, int V, int H, int dtype, void *out, void *stream);

/* The same product WITHOUT the final rounding: y fp32 [M,N] = the fp32 row sums.  For the row-parallel Linears (o_proj,
 * down_proj) of a tensor-parallel shard, whose partial sums are all-reduced over the ranks before the one rounding to T
 * (proxy_inference_engine_amd/tp.py; the reference has no parallelism). */
int pie_qgemv_w4g64_f32(const void *x, int M, const void *packed, int N, int K, float *y, int dtype, void *stream);

/* nn.QuantizedEmbedding.__call__ (models/llama/language.py:176): dequantise gathered rows of the
 * MLX-layout table.  ids device int32 [L] -> out [L,H] T. */
int pie_embedding_w4g64(const int32_t *ids, int L, const uint32_t *codes, const void *scales, const void *biases,
                        int V, int H, int dtype, void *out, void *stream);

/* ---------------------------------------------------------------- mx.fast.rms_norm(x, w, eps) (K3)
 * Call sites: nn.RMSNorm at models/llama/language.py:137-141, :168.  x,y [rows,H] T, w [H] T. */
int pie_rms_norm(const void *x, const void *w, float eps, int rows, int H, int dtype, void *y, void *stream);

/* ---------------------------------------------------------------- mx.fast.rope(x, D, traditional=False,
 * base=None, scale=1.0, offset, freqs) (K4).  Call site: models/llama/utils.py:42-50.
 * x,y [heads,L,D] T; freqs device fp32 [D/2]; position of row l = offset + l. */
int pie_rope(const void *x, int heads, int L, int D, const float *freqs, int offset, int dtype, void *y, void *stream);
/* the same with mx.fast.rope's `traditional` flag: non-zero rotates the interleaved pairs (2i, 2i+1) */
int pie_rope_ex(const void *x, int heads, int L, int D, const float *freqs, int offset, int traditional, int dtype, void *y,
                void *stream);

/* ---------------------------------------------------------------- mx.fast.scaled_dot_product_attention (K2)
 * Call site: models/base.py:111-113 <- models/llama/language.py:98-105.  Decode form (L = 1, mask = None):
 * q [Hq,1,D] T; k,v [Hkv,cap,D] T of which the first T positions are attended (the strided view
 * cache/kv_cache/reusable.py:142 returns); out [Hq,1,D] T.  GQA: q-head h uses kv-head h / (Hq/Hkv).
 * fp32 scores / softmax / PV, one rounding at the end (MLX fused-kernel contract).
 * workspace: device scratch of pie_sdpa_decode_workspace_bytes(Hq, D) bytes. */
size_t pie_sdpa_decode_workspace_bytes(int Hq, int D);
int pie_sdpa_decode(const void *q, const void *k, const void *v, int Hq, int Hkv, int T, int cap, int D, float scale,
                    int dtype, void *out, void *workspace, void *stream);

/* The same call site at L > 1 with the causal mask of models/base.py:37-53 (query row l at absolute position offset + l sees
 * keys 0 .. offset + l): q, out [L, Hq, D] T (the [B, L, h, D] order of language.py:86 before its transpose); k, v
 * [Hkv, cap, D] with rows [0, offset + L) valid.  MFMA flash kernel; P kept as hi + lo halves of T (~fp32 contract). */
int pie_sdpa_prefill(const void *q, const void *k, const void *v, int Hq, int Hkv, int L, int offset, int cap, int D,
                     float scale, int dtype, void *out, void *stream);

/* nn.silu(a) * b (models/llama/language.py:127) and the residual adds (:151,:153) (K6, K7). */
int pie_silu_mul(const void *a, const void *b, size_t n, int dtype, void *y, void *stream);
int pie_add(const void *a, const void *b, size_t n, int dtype, void *y, void *stream);

/* ---------------------------------------------------------------- logits tail (K9)
 * engine/inference_engine.py:268-271 + samplers/__init__.py:37-38: logprobs = f32(logits) - logsumexp,
 * token = first argmax.  logits [V] T, logprobs fp32 [V], token device int32 [1]. */
int pie_logprobs_argmax(const void *logits, int V, int dtype, float *logprobs, int32_t *token, void *stream);
/* The repetition penalty (logits_processors/repetition.py:11-22) on logits [V] T, in place: for every DISTINCT id among ids[0..n) (device
 * int32), x = f32(logits[id]), logits[id] = T(x < 0 ? x * (float)penalty : x / (float)penalty) -- one IEEE fp32 multiplication or division,
 * then one round-to-nearest-even to T.  An id that occurs several times is penalised once (the reference gathers, computes and scatters);
 * ids outside [0, V) are skipped and never indexed; -0.0 is not < 0 and is divided.  One launch of one workgroup.
 * penalty < 0 or not finite, n outside 1..1024: PIE_E_ARG; V < 1: PIE_E_SHAPE -- each before any launch. */
int pie_logits_penalty(void *logits, int V, int dtype, const int32_t *ids, int n, double penalty, void *stream);
/* The token mask of structured decoding (the reference's first processor, structuring_engine.process_logits, inference_engine.py:319-335,
 * leaves only the allowed ids finite) fused into the log-softmax: mask is DEVICE uint32 [mask_words >= ceil(V / 32)], token i is allowed
 * iff bit i & 31 of word i >> 5 is set (LSB first, the layout grammar engines export); bits at or beyond V are ignored.  logits [V] T are
 * masked IN PLACE -- a disallowed id becomes -inf, an allowed id keeps its bits -- then logprobs and token are written exactly as
 * pie_logprobs_argmax of the masked logits writes them (same 256-tile partition, same first-argmax rule).  Two launches: the masked
 * partials pass, then the finish.  An all-zero mask is the caller's error: token 0 and NaN logprobs, like pie_logprobs_argmax of an
 * all -inf row.  mask_words < ceil(V / 32): PIE_E_SHAPE; a mask not 4-byte aligned: PIE_E_ALIGN -- each before any launch. */
int pie_logprobs_argmax_masked(void *logits, int V, int dtype, const uint32_t *mask, int mask_words, float *logprobs, int32_t *token,
                               void *stream);
/* logit_bias (logits_params.hpp; logit_processor_factory.cpp) on logits [V] T, in place: ids DEVICE int32 [n], bias DEVICE float [n]; for
 * every entry t whose id is in [0, V) and not held by an earlier entry, logits[id] = T(f32(logits[id]) + bias[t]) -- one IEEE fp32
 * addition, one round-to-nearest-even to T.  The first of duplicate ids owns the id (pie_logits_penalty's rule); ids out of range are
 * skipped and never indexed.  One launch of one workgroup.  n outside 1..1024: PIE_E_ARG; V < 1: PIE_E_SHAPE; ids or bias not
 * 4-byte aligned: PIE_E_ALIGN -- each before any launch. */
int pie_logits_bias(void *logits, int V, int dtype, const int32_t *ids, const float *bias, int n, void *stream);
/* Measurement aid (no reference counterpart; SURVEY.md 8d "fraction of a measured device-copy bandwidth"): a bare streaming read of `bytes`
 * shaped like the weight GEMV's stream (one 8-wave workgroup per CU, non-temporal 16-byte loads, nothing computed).  bench.py times it for
 * roofline.stream_peak. */
int pie_stream_read(const void *p, size_t bytes, void *stream);

/* The stochastic branches of make_sampler (samplers/__init__.py:39-46) over fp32 log-probabilities [rows, V], one kernel, no sort:
 * every branch scales by 1 / temp, filters, and draws argmax(x + Gumbel) like mx.random.categorical.
 *   mode PIE_SAMPLE_CATEGORICAL  categorical_sampling (categorical.py:6-8)
 *        PIE_SAMPLE_TOP_K        top_k_sampling(k)                        (top_k.py:14-29; k in (0, V), else PIE_E_ARG like its ValueError)
 *        PIE_SAMPLE_TOP_P        top_p_sampling(p)                        (top_p.py:18-33; kept: ascending cumulative probability > 1 - p)
 *        PIE_SAMPLE_MIN_P        min_p_sampling(p, min_tokens_to_keep=k)  (min_p.py:30-60)
 * seed + counter: the random stream (Philox-4x32-10; the library's own, not MLX's).  counter = DEVICE uint64[2], zeroed by the caller when
 * it (re)seeds; the last workgroup advances it, so a captured graph keeps drawing fresh numbers.  workspace: pie_sample_workspace_bytes(rows, V)
 * bytes of device memory, ZEROED once by the caller and then reused from call to call (the kernels leave it ready for the next one).
 * tokens int32 [rows]; kept_count (nullable) int32 [rows] = number of drawable ids; kept_mask (nullable) uint8 [rows, V] = which ids the
 * filter keeps (tests compare it with the reference's sort-based definition).  2 launches (categorical, min-p) or 5 (top-k, top-p), a row
 * spread over V / 512 workgroups; V <= 524288. */
enum { PIE_SAMPLE_CATEGORICAL = 0, PIE_SAMPLE_TOP_K = 1, PIE_SAMPLE_TOP_P = 2, PIE_SAMPLE_MIN_P = 3 };
size_t pie_sample_workspace_bytes(int rows, int V);
int pie_sample(const float *logprobs, int rows, int V, int mode, double temp, double p, int k, unsigned long long seed, unsigned long long *counter,
               void *workspace, int32_t *tokens, int32_t *kept_count, unsigned char *kept_mask, void *stream);

/* ---------------------------------------------------------------- per-row tails
 * One record per output row of a multi-sequence pass, in DEVICE memory: everything about a row's penalty and sampler that pie_sample and
 * pie_logits_penalty take as arguments.  Nothing of it is a launch argument, so a captured graph keeps replaying while requests with
 * different parameters come and go in its rows.
 *   mode          PIE_SAMPLE_GREEDY (the row keeps the argmax already in tokens[r]) or one of the four PIE_SAMPLE_*
 *   inv_temp, thr pie_sample's derived fp32 values: (float)(1 / temp); (float)(1 - top_p) or (float)log(min_p)
 *   k             top_k, or min_tokens_to_keep
 *   seed, calls   the row's own random stream: draw number `calls` of `seed`; the row's last draw workgroup advances `calls`
 *   penalty       the repetition penalty as fp32; exactly 1.0: none
 *   context_size  its window, 1..1024 positions
 * pie_row_tail_pack fills a record in HOST memory from the arguments of pie_sample (mode, temp, p, k, seed) and pie_logits_penalty
 * (penalty) with their argument rules (no vocabulary is known here: top_k > 0, min_tokens_to_keep >= 1; mode PIE_SAMPLE_GREEDY ignores
 * temp, p and k), context_size 1..1024: PIE_E_ARG otherwise, nothing touches a device.  The kernels do not trust the bytes they read: an
 * unknown mode acts as greedy, k is clamped to [1, V], context_size to [1, 1024], and every index is checked. */
enum { PIE_SAMPLE_GREEDY = -1 };
typedef struct pie_row_tail {
    int32_t mode;
    float inv_temp, thr;
    int32_t k;
    unsigned long long seed, calls;
    float penalty;
    int32_t context_size;
} pie_row_tail;
size_t pie_row_tail_bytes(void); /* sizeof(pie_row_tail), for bindings */
int pie_row_tail_pack(int mode, double temp, double p, int k, unsigned long long seed, unsigned long long calls, double penalty, int context_size,
                      pie_row_tail *out);
/* pie_sample with per-row parameters: row r of logprobs [rows, V] is filtered and drawn exactly as pie_sample(logprobs + r * V, rows = 1, ...)
 * with table[r]'s mode, temperature, p, k and seed and a counter of {table[r].calls, 0} -- the same token and kept mask, bit for bit; a
 * request's stream depends on neither its row nor its neighbours.  table: DEVICE pie_row_tail [rows], 8-byte aligned; a drawn row's `calls`
 * is advanced by one.  A greedy (or unknown-mode) row is left alone: its workspace, tokens[r], kept_count[r] and kept_mask row are not
 * written.  Always 5 launches over a (V / 512, rows) grid; a workgroup whose row does not need a launch returns at once.  workspace:
 * pie_sample_workspace_bytes(rows, V) bytes, zeroed once, reusable from call to call whatever the rows' modes become. */
int pie_sample_rows(const float *logprobs, int rows, int V, pie_row_tail *table, void *workspace, int32_t *tokens, int32_t *kept_count,
                    unsigned char *kept_mask, void *stream);
/* XTC, "exclude top choices" (mlx-lm's apply_xtc): with a coin's probability, every id more probable than the LEAST
 * probable one above a threshold is hidden from the draw, so the sampler takes a plausible continuation other than the obvious one.
 * It runs over the unscaled fp32 log-probabilities lp[0..V) of a row, before the division by the temperature:
 *   COIN        u = ((r >> 8) + 0.5) * 2^-24, r = word 0 of the Philox-4x32-10 block with key seed and counter {0xFFFFFFFF, row, call}
 *               (row and call as for the draw: row 0 and the record's `calls` in the table form).  No vocabulary index reaches that block
 *               (V <= 524288), so the draw's Gumbel stream is untouched.  XTC applies to this call iff u < probability.
 *   CANDIDATES  A = { i : lp[i] > log_threshold } (fp32 compare; special ids are members like any other).  |A| < 2: nothing is removed.
 *   CUT         m = min over A of lp[i]; removed R = { i : lp[i] > m, i not special }.  Ids tied at m stay, special ids stay.
 *   DRAW        exactly as if lp[i] were -inf for i in R, in every mode; top-p's weights and min-p's threshold refer to the survivors' maximum.
 * The token is bit for bit pie_sample's over a copy of logprobs with R set to -inf on the same seed and counter; kept_mask is 0 on R and
 * that call's mask elsewhere, kept_count that call's count without the members of R it counts; the call counter advances as ever.  A greedy
 * row ignores XTC; probability == 0 is off.  logprobs are only read.
 * pie_xtc is one record in DEVICE memory (4-byte aligned); pie_xtc_pack fills it in HOST memory: probability in [0, 1], threshold in
 * (0, 0.5] (log_threshold = (float)log(threshold)), n_special 0..PIE_XTC_SPECIAL_MAX ids never removed (end of sequence, newline):
 * PIE_E_ARG otherwise, nothing touches a device.  The kernels do not trust the bytes they read: n_special is clamped to 0..16, a special id
 * outside [0, V) matches nothing, probability and log_threshold only enter comparisons (NaN: nothing is removed).
 * pie_sample_xtc / pie_sample_rows_xtc: pie_sample / pie_sample_rows plus xtc -- ONE record shared by the rows, or DEVICE [rows] in the
 * table form -- and removed (nullable) DEVICE int32 [rows] = |R| of the call (0 when the coin says no; a greedy row's is not written).
 * xtc == NULL: exactly the old op.  One launch more than the same call without (a grid-wide integer atomic min finds the cut and leaves
 * it in a word of the row's workspace header: pie_sample_workspace_bytes is unchanged, and nothing depends on arrival order). */
enum { PIE_XTC_SPECIAL_MAX = 16 };
typedef struct pie_xtc {
    float log_threshold, probability;
    int32_t n_special, reserved;
    int32_t special[PIE_XTC_SPECIAL_MAX];
} pie_xtc;
size_t pie_xtc_bytes(void); /* sizeof(pie_xtc) = 80, for bindings */
int pie_xtc_pack(double probability, double threshold, const int32_t *special, int n_special, pie_xtc *out);
int pie_sample_xtc(const float *logprobs, int rows, int V, int mode, double temp, double p, int k, unsigned long long seed, unsigned long long *counter,
                   void *workspace, int32_t *tokens, int32_t *kept_count, unsigned char *kept_mask, const pie_xtc *xtc, int32_t *removed, void *stream);
int pie_sample_rows_xtc(const float *logprobs, int rows, int V, pie_row_tail *table, void *workspace, int32_t *tokens, int32_t *kept_count,
                        unsigned char *kept_mask, const pie_xtc *xtc, int32_t *removed, void *stream);
/* pie_logits_penalty with per-row windows, one launch, one workgroup per row of logits [rows, V] T.  recent_ids: caller-owned DEVICE int32
 * [rows, 1024], a ring per row: the id fed at position q lives at recent_ids[r][q & 1023].  ids / ctx: the pass's input ids and context
 * lengths [n_src]; out_rows (nullable) [rows]: output row s reads source row i = out_rows ? out_rows[s] : s.  With pos = ctx[i] - 1 the
 * kernel records ids[i] at recent_ids[s][pos & 1023], then penalises the distinct ids of positions max(0, pos + 1 - context_size) .. pos
 * with pie_logits_penalty's arithmetic (the row's own input is inside the window, the token about to be chosen is not).  A row with
 * pos < 0 (an idle slot) or i outside [0, n_src) is skipped; a row whose penalty is exactly 1.0 is recorded and not penalised. */
int pie_logits_penalty_rows(void *logits, int rows, int V, int dtype, const pie_row_tail *table, int32_t *recent_ids, const int32_t *ids,
                            const int32_t *ctx, const int32_t *out_rows, int n_src, void *stream);

/* Per-row forms of the token mask and of logit_bias: what the multi-sequence passes run with pie_decoder_set_batch_logits_edits.
 * pie_logprobs_argmax_rows_masked: logits [rows, V] T, masks DEVICE uint32 [rows, mask_words >= ceil(V / 32)] in pie_logprobs_argmax_masked's
 *   bit layout, mask_on DEVICE int32 [rows], read on the device: nonzero = row r is masked in place with its own words and logprobs [rows, V],
 *   tokens [rows] are written -- bit for bit what pie_logprobs_argmax_masked(logits + r * V, ..., masks + r * mask_words, ...) gives that row
 *   alone; zero = the row's words are not read, every logit keeps its bits and the row is pie_logprobs_argmax's.  Two launches over a
 *   (256, rows) and a (64, rows) grid; the partials live in stream-ordered scratch.  An all-zero mask on an armed row is the caller's error.
 *   rows < 1, a null pointer: PIE_E_ARG; rows > 65535, V < 1, mask_words < ceil(V / 32): PIE_E_SHAPE; masks or mask_on not 4-byte aligned:
 *   PIE_E_ALIGN -- each before any launch.
 * pie_logits_bias_rows: logits [rows, V] T in place; ids DEVICE int32 [rows, cap], bias DEVICE float [rows, cap], n DEVICE int32 [rows], cap
 *   1..1024.  Row r takes its first min(max(n[r], 0), cap) entries under pie_logits_bias's rule (id in [0, V), the first of duplicate ids
 *   owns the id, one fp32 addition, one rounding to T): bit for bit pie_logits_bias of that row with that table; n[r] == 0 keeps every bit.
 *   One launch, one workgroup per row.  rows < 1, cap outside 1..1024: PIE_E_ARG; V < 1: PIE_E_SHAPE; ids, bias or n not 4-byte aligned:
 *   PIE_E_ALIGN -- each before any launch. */
int pie_logprobs_argmax_rows_masked(void *logits, int rows, int V, int dtype, const uint32_t *masks, int mask_words, const int32_t *mask_on,
                                    float *logprobs, int32_t *tokens, void *stream);
int pie_logits_bias_rows(void *logits, int rows, int V, int dtype, const int32_t *ids, const float *bias, const int32_t *n, int cap, void *stream);

/* ---------------------------------------------------------------- frequency and presence penalties
 * The two OpenAI-style logits parameters, on counts of a request's GENERATED tokens: with c[v] = how often id v occurs among the tokens
 * generated so far for the request (prompt tokens do not count, neither does the token about to be chosen),
 *   c[v] == 0 :  x'[v] = x[v]                                             (the stored T value is not rewritten)
 *   c[v] >  0 :  x'[v] = T( f32(x[v]) - ( f32(freq) * (float)c[v] + f32(pres) ) )
 * with one fp32 multiplication, one fp32 addition and one fp32 subtraction in that association (no fma), and one round-to-nearest-even
 * to T.  -inf stays -inf, +-inf and NaN follow IEEE, an f16 result beyond 65504 is inf.  freq and pres may be negative.
 * ORDER inside a tail: (1) token mask (physically last: a masked id is -inf whatever else is configured), (2) repetition penalty,
 * (3) logit_bias, (4) frequency / presence; then the unchanged log-softmax + argmax, the sampler and the top-n record.
 * State per output row, caller-owned DEVICE memory: counts int32 [rows_cap, V] (exact beyond 65535) and one pie_count_penalty record:
 *   freq, pres    the two parameters as fp32; both exactly 0: the row is left alone, bit for bit, and nothing is counted
 *   start         the first position that holds a generated token (= the prompt's length): an input id at a position below it is a
 *                 prompt token and is not counted
 *   counted_pos   the last position whose input id has been counted (start - 1 when none has): a position is counted once, however
 *                 often a pass over it is run
 * pie_count_penalty_pack fills a record in HOST memory: freq and pres finite, start >= 0, counted_pos >= -1, PIE_E_ARG otherwise; nothing
 * touches a device.  The kernel does not trust the bytes it reads: every index is checked, freq and pres only enter arithmetic.
 * pie_logits_count_penalty_rows: logits [rows, V] T in place, one launch over a (ceil((ceil(V / 4) + 1) / 128), rows) grid of 128-thread
 *   workgroups, four elements per thread (8-byte logits and 16-byte counts accesses where the row's base allows, scalar heads and tails
 *   where it does not).  Row s reads source row i = out_rows ? out_rows[s] : s of ids / ctx [n_src] (pie_logits_penalty_rows' rule): its
 *   input id ids[i] sits at position pos = ctx[i] - 1; pos < 0 (an idle slot) or i outside [0, n_src): the row is skipped.  COUNTING: when
 *   pos >= start, pos > counted_pos and 0 <= ids[i] < V, the one thread that covers element ids[i] increments counts[s][ids[i]], stores
 *   counted_pos = pos and uses the incremented count; no other thread reads or writes either, so there is no atomic and no ordering
 *   between workgroups.  Then the formula over the row.  ctx == NULL (ids and out_rows are then ignored): every row is live and nothing
 *   is counted -- the counts are used as they are.  rows < 1, a null pointer: PIE_E_ARG; rows > 65535, V < 1, n_src < 1, fewer source rows
 *   than rows without out_rows: PIE_E_SHAPE; records or counts not 4-byte aligned, logits not 2-byte aligned: PIE_E_ALIGN -- each before
 *   any launch. */
typedef struct pie_count_penalty {
    float freq, pres;
    int32_t start, counted_pos;
} pie_count_penalty;
size_t pie_count_penalty_bytes(void); /* sizeof(pie_count_penalty) = 16, for bindings */
int pie_count_penalty_pack(double freq, double pres, int start, int counted_pos, pie_count_penalty *out);
int pie_logits_count_penalty_rows(void *logits, int rows, int V, int dtype, pie_count_penalty *records, int32_t *counts, const int32_t *ids,
                                  const int32_t *ctx, const int32_t *out_rows, int n_src, void *stream);

/* ---------------------------------------------------------------- DRY penalty
 * DRY ("don't repeat yourself"), the sequence-repetition penalty of text-generation-webui, llama.cpp, koboldcpp and exllama: only the token
 * that would extend a verbatim repeat of the sequence's tail is penalised, exponentially in the length of that repeat.
 * PARAMETERS  multiplier: finite, >= 0; exactly 0 means off and the row keeps every bit.  base: finite, > 0.  allowed_length: 1..64.
 *   range: 1..1024 window positions.  breakers: up to PIE_DRY_BREAKERS_MAX token ids ("sequence breakers"; the caller passes ids).
 * WINDOW  c[0..n) are the ids at positions max(0, pos + 1 - range) .. pos, pos = the position of the row's input id, so c[n-1] is the input
 *   id; the token about to be chosen is not in the window (the repetition penalty's window rule).
 * No penalty if n < 2 or c[n-1] is a breaker.
 * CANDIDATES  every i in 0 .. n-2 with c[i] == c[n-1].  Let t = c[i+1].  Position i is skipped if t is a breaker or lies outside [0, V);
 *   such a t is never used as an index.
 * MATCH LENGTH  L_i is the largest L with 1 <= L <= min(i + 1, PIE_DRY_MAX_MATCH) such that for every 1 <= m < L: c[i-m] == c[n-1-m], and
 *   c[n-1-m] is not a breaker.  The two runs may overlap, so a period-3 tail matches to the cap.  A match never reaches before the window's
 *   first position.
 * PENALTY  M[t] = max L_i over the positions i with c[i+1] == t.  For every t with M[t] >= allowed_length: p = f32(multiplier), then
 *   p = p * f32(base) exactly M[t] - allowed_length times, each one fp32 round-to-nearest multiplication (no powf, no fma); then
 *   x'[t] = T( f32(x[t]) - p ): one fp32 subtraction and one rounding to T.  Every other element keeps its stored bits and is not rewritten.
 *   -inf stays -inf; infinities, NaN and f16 overflow follow IEEE, as for the count penalties.
 * ORDER inside a tail: (1) token mask (physically last: a masked id stays -inf), (2) repetition penalty, (3) logit_bias, (4) frequency /
 *   presence, (5) DRY; then the unchanged log-softmax + argmax, the sampler and the top-n record.
 * DETERMINISM  M[t] is a maximum: among the candidates of one id the one with the larger L, then the lower i, owns the id (decided through
 *   LDS) and does the one read-modify-write; nothing depends on arrival order.  One workgroup of 1024 threads per logit vector, one thread
 *   per window position; breaker membership is computed once per window position.
 * pie_dry_penalty is one row's record; pie_dry_penalty_pack fills it in HOST memory under the parameter rules above (n_breakers
 *   0..PIE_DRY_BREAKERS_MAX), PIE_E_ARG otherwise; nothing touches a device.  The kernels do not trust the bytes they read: allowed_length
 *   is clamped to 1..64, range to 1..1024, n_breakers to 0..64; multiplier and base only enter arithmetic.
 * pie_logits_dry_penalty: logits [V] T in place, the window is ids[0..n) (DEVICE int32, n 1..1024, ids[n-1] = the input id; the range is
 *   n), breakers DEVICE int32 [n_breakers] (may be NULL when n_breakers == 0).  One launch.
 * pie_logits_dry_penalty_rows: logits [rows, V] T in place, one launch, one workgroup per row.  Row s reads source row i = out_rows ?
 *   out_rows[s] : s of ids / ctx [n_src] (pie_logits_penalty_rows' rule): its input id ids[i] sits at position pos = ctx[i] - 1; pos < 0
 *   (an idle slot) or i outside [0, n_src): the row is skipped.  Every live row first records its input id in its ring
 *   recent_ids[s][pos & 1023] -- a zero record too -- then takes its window from the ring.  records DEVICE [rows], breakers DEVICE int32
 *   [rows, PIE_DRY_BREAKERS_MAX], recent_ids DEVICE int32 [rows, 1024].
 * A null pointer, an argument outside the parameter rules, n outside 1..1024, a dtype other than PIE_BF16 / PIE_F16: PIE_E_ARG; V < 1, rows
 *   outside 1..65535, n_src < 1, fewer source rows than rows without out_rows: PIE_E_SHAPE; an int32 array or the records not 4-byte
 *   aligned, logits not 2-byte aligned: PIE_E_ALIGN -- each before any launch. */
enum { PIE_DRY_MAX_MATCH = 64, PIE_DRY_BREAKERS_MAX = 64 };
typedef struct pie_dry_penalty {
    float multiplier, base;
    int32_t allowed_length, range, n_breakers, reserved;
} pie_dry_penalty;
size_t pie_dry_penalty_bytes(void); /* sizeof(pie_dry_penalty) = 24, for bindings */
int pie_dry_penalty_pack(double multiplier, double base, int allowed_length, int range, int n_breakers, pie_dry_penalty *out);
int pie_logits_dry_penalty(void *logits, int V, int dtype, const int32_t *ids, int n, double multiplier, double base, int allowed_length,
                           const int32_t *breakers, int n_breakers, void *stream);
int pie_logits_dry_penalty_rows(void *logits, int rows, int V, int dtype, const pie_dry_penalty *records, const int32_t *breakers,
                                int32_t *recent_ids, const int32_t *ids, const int32_t *ctx, const int32_t *out_rows, int n_src, void *stream);

/* ---------------------------------------------------------------- top-n log-probabilities
 * get_top_logprobs (engine/utils.py:4-48) on the device, sort-free: for every row of fp32 log-probabilities [rows, V] the n best
 * (id, value) pairs and the chosen token's own, n 1..PIE_TOP_LOGPROBS_MAX.  tokens (nullable) DEVICE int32 [rows]; count (nullable)
 * DEVICE int32 [rows].
 *   rank    ids are ranked by (key(lp[id]) descending, id ascending), key = the samplers' order-preserving 32-bit key: float order, with
 *           +0.0 above -0.0 and NaNs placed by their bits; ties go to the lowest id, the samplers' rule at the top-k boundary
 *   output  out_ids int32 [rows, n + 1], out_vals fp32 [rows, n + 1].  Slot 0: (tokens[r], lp[r][tokens[r]]), or (-1, -inf) when tokens is
 *           NULL or the id lies outside [0, V) (never indexed).  Slots 1..m, m = min(c, V): the first m ids in rank order with bit copies
 *           of their values.  Slots m + 1..n: (-1, -inf)
 *   count   c = count ? count[r] : n, read on the device and not trusted: c > n acts as n; c == 0 writes slot 0 and the fill; c < 0 leaves
 *           the row's record untouched (its workgroups return at once)
 * Two launches (slices of 512 ids, then one workgroup per row), deterministic: no atomics, nothing depends on arrival order.  workspace:
 * pie_top_logprobs_workspace_bytes(rows, V, n) bytes of device memory, 8-byte aligned; needs no initialisation and carries nothing from call
 * to call (0 is returned for sizes the op refuses).  n outside 1..20: PIE_E_ARG; rows < 1, V < 1 or V > 524288: PIE_E_SHAPE; logprobs,
 * tokens, count or an output not 4-byte aligned, or the workspace not 8-byte aligned: PIE_E_ALIGN -- each before any launch. */
enum { PIE_TOP_LOGPROBS_MAX = 20 };
size_t pie_top_logprobs_workspace_bytes(int rows, int V, int n);
int pie_top_logprobs(const float *logprobs, int rows, int V, int n, const int32_t *tokens, const int32_t *count, int32_t *out_ids, float *out_vals,
                     void *workspace, void *stream);

/* ---------------------------------------------------------------- log-probabilities of prompt tokens
 * `echo` / prompt_logprobs: pie_top_logprobs' record of every row, straight from a block of T logits [rows, V] -- no fp32 row is written.
 * lp[i] = f32(logits[r][i]) - lse_r in fp32, lse_r the row's log-sum-exp exactly as pie_logprobs_argmax computes it; slot 0 is
 * (targets[r], lp[targets[r]]) -- (-1, -inf) for NULL targets or an id outside [0, V), never indexed -- and slots 1..n follow pie_top_logprobs'
 * rank, output and count rules, ranked on lp (two logits may round to one lp: the tie goes to the lower id).  The record equals, bit for bit,
 * pie_top_logprobs over the logprobs pie_logprobs_argmax writes for the same row.  targets, count (both nullable) DEVICE int32 [rows].
 * Four launches (the tail's partials, one lse per row, slices of 512 ids, one workgroup per row), deterministic; a row with count <= 0
 * leaves the slices launch at once.  workspace: pie_prompt_logprobs_workspace_bytes(rows, V, n) bytes of device memory, 8-byte aligned; needs
 * no initialisation and carries nothing from call to call (0 is returned for sizes the op refuses).  Checked in this order, each before any
 * launch: n outside 1..20: PIE_E_ARG; rows outside 1..65535 or V outside 1..524288: PIE_E_SHAPE; targets, count or an output not 4-byte
 * aligned, logits not 2-byte, the workspace not 8-byte aligned: PIE_E_ALIGN; a dtype that is neither PIE_BF16 nor PIE_F16: PIE_E_ARG. */
size_t pie_prompt_logprobs_workspace_bytes(int rows, int V, int n);
int pie_prompt_logprobs(const void *logits, int rows, int V, int dtype, int n, const int32_t *targets, const int32_t *count, int32_t *out_ids,
                        float *out_vals, void *workspace, void *stream);

/* ---------------------------------------------------------------- greedy speculative decoding
 * No reference counterpart beyond the shape of its loop: generate() consumes several tokens per generate_step yield
 * (engine/inference_engine.py:200-206).  Two ops: a prompt-lookup drafter (n-gram copy from the sequence's own ids) and the verify of a block
 * of raw logits against a draft.
 * pie_ngram_draft: ids DEVICE int32 [>= cap] = the sequence so far, the last id being the token about to be fed; len DEVICE int32 [1], read on
 *   the device and CLAMPED there to [0, cap] (a device value cannot be refused before the launch: the search never reads beyond the cap ids
 *   the caller vouches for); out_ids DEVICE int32 [k], out_count DEVICE int32 [1].  RULE: for n = ngram_max down to ngram_min the suffix is
 *   ids[len - n : len]; a match is a start p with p + n <= len - 1 and ids[p : p + n] == suffix; the LARGEST p of the LARGEST n that has any
 *   match is taken, and with h' = ids ++ draft, draft[i] = h'[p + n + i] for i < k -- an overlapped (LZ77) copy, so a period-3 tail drafts k
 *   ids -- and out_count = k.  No match for any n, or len <= ngram_min: out_count = 0 and out_ids keeps its contents.  Deterministic: no
 *   atomics, nothing depends on arrival order.  Two launches: the search over a grid sized from cap (one workgroup per 2048 ids, at most
 *   1024, grid-stride beyond; one partial per workgroup in the workspace), then one workgroup that reduces the partials and one thread of
 *   it that copies the k ids.  workspace: pie_ngram_draft_workspace_bytes() bytes of device memory, 4-byte aligned, no initialisation.
 *   Checked in this order, each before any launch: ngram_min < 1, ngram_min > ngram_max, ngram_max > 8, k outside 1..31, a null pointer:
 *   PIE_E_ARG; cap outside 1..2^27: PIE_E_SHAPE; a pointer not 4-byte aligned: PIE_E_ALIGN.
 * pie_spec_verify: logits [rows, V] T, rows 2..32: row 0 is the fed token's, row i the i-th draft's; draft DEVICE int32 [rows - 1].  a_r = row
 *   r's greedy token, bit for bit what pie_logprobs_argmax gives that row alone (same 256-tile partition, same merge, same first-argmax
 *   rule).  n_acc = the largest j with draft[i - 1] == a_{i - 1} for all 1 <= i <= j; a draft id outside [0, V) is never accepted and never
 *   used as an index.  out_n [1] = n_acc + 1; out_tokens [rows]: a_0 .. a_{n_acc}, then -1.  logprobs (nullable) fp32 [rows, V]: rows
 *   0 .. n_acc are written, bit-identical with pie_logprobs_argmax's; the rows behind them keep their contents (the predicate is read on
 *   the device: their workgroups return at once).  Three launches: the partials over (256, rows), one merge workgroup per row, the accept
 *   and log-probabilities over (64, rows).  workspace: pie_spec_verify_workspace_bytes(rows) bytes (0 for refused sizes), 16-byte aligned,
 *   no initialisation.  A null pointer: PIE_E_ARG; rows outside 2..32, V < 1: PIE_E_SHAPE; logits not 2-byte, draft or an output not
 *   4-byte, the workspace not 16-byte aligned: PIE_E_ALIGN; a dtype that is neither PIE_BF16 nor PIE_F16: PIE_E_ARG -- each before any launch. */
size_t pie_ngram_draft_workspace_bytes(void);
int pie_ngram_draft(const int32_t *ids, const int32_t *len, int cap, int ngram_max, int ngram_min, int k, int32_t *out_ids, int32_t *out_count,
                    void *workspace, void *stream);
size_t pie_spec_verify_workspace_bytes(int rows);
int pie_spec_verify(const void *logits, int rows, int V, int dtype, const int32_t *draft, int32_t *out_tokens, int32_t *out_n, float *logprobs,
                    void *workspace, void *stream);
/* pie_spec_verify_sampled: pie_spec_verify under a stochastic sampler.  A prompt-lookup draft is a point mass, so "draw row
 * r from the model's own distribution with the draw the plain loop would have used for that token, and accept while the draw equals the
 * draft" is exact and needs no rejection-sampling arithmetic.  Let c = counter[0] at entry, READ ON THE DEVICE (no host round trip):
 *   - logprobs (required) fp32 [rows, V]: EVERY row r gets pie_logprobs_argmax's bits of row r alone (the draws read them before n_acc is
 *     known -- unlike pie_spec_verify, which leaves the rows behind the accepted run alone);
 *   - t_r = the token pie_sample_xtc(logprobs + r * V, rows = 1, V, mode, temp, p, k, seed, counter = {c + r, 0}, ..., xtc) draws (pie_sample's
 *     when xtc == NULL), bit for bit: row r goes through pie_sample_rows(_xtc)'s launches with a record whose calls = c + r;
 *   - n_acc = the largest j with draft[i] == t_i for all i < j; a draft id outside [0, V) is never accepted and never used as an index;
 *   - out_n [1] = n_acc + 1; out_tokens [rows] = t_0 .. t_{n_acc}, then -1;
 *   - afterwards counter = {c + out_n, 0}: the draws of the rows behind the accepted run are discarded and their stream positions are NOT
 *     consumed, so token number j of a generation is always draw number j of the seed, whether a step or a pass produced it.
 * xtc (nullable): ONE DEVICE record shared by the rows.  Launches: the partials and the finish over every row (2), one workgroup that
 * fills the rows' records from counter[0] (1), pie_sample_rows' 5 (6 with xtc), and one thread that accepts, writes the outputs and stores
 * the counter: 9 or 10.  No atomics beyond the sampler's own; nothing depends on arrival order.  workspace:
 * pie_spec_verify_sampled_workspace_bytes(rows, V) bytes (0 for refused sizes), 16-byte aligned, ZEROED ONCE by the caller (as
 * pie_sample's) and reusable from call to call.  Each before any launch: a null pointer (xtc excepted), mode PIE_SAMPLE_GREEDY (use
 * pie_spec_verify), a dtype that is neither PIE_BF16 nor PIE_F16, a parameter outside pie_sample's rules: PIE_E_ARG; rows outside 2..32, V
 * outside 1..524288: PIE_E_SHAPE; logits not 2-byte, draft, xtc or an output not 4-byte, the counter not 8-byte, the workspace not 16-byte
 * aligned: PIE_E_ALIGN. */
size_t pie_spec_verify_sampled_workspace_bytes(int rows, int V);
int pie_spec_verify_sampled(const void *logits, int rows, int V, int dtype, const int32_t *draft, int mode, double temp, double p, int k, unsigned long long seed,
                            unsigned long long *counter, const pie_xtc *xtc, int32_t *out_tokens, int32_t *out_n, float *logprobs, void *workspace, void *stream);
/* pie_spec_verify_draft: the verify of a block drafted by a MODEL -- speculative sampling (Leviathan et al. 2023, Chen et
 * al. 2023).  logits [rows, V] T as above; q_logprobs DEVICE fp32 [rows - 1, V]: the drafter's log-probabilities at the step that drew
 * draft[i]; one sampler setting (mode, temp, p, k) for both sides; (seed, counter) the TARGET's stream, c = counter[0] read on the device.
 *   dist: for a row of fp32 log-probabilities lp with the sampler's kept set K -- exactly the kept_mask pie_sample yields on that row (the
 *     op runs the sampler's own filter launches with a mask output) -- dist(x) = exp((lp[x] - max_K lp) * inv_temp) / sum_{y in K}
 *     exp((lp[y] - max_K lp) * inv_temp) for x in K and 0 elsewhere, inv_temp = fp32(1 / temp); a filter that kept nothing (top_p below
 *     2^-25) gives dist = 0 everywhere.  P_r = dist of pie_logprobs_argmax's bits of logits row r (written to logprobs, required, fp32
 *     [rows, V], every row); Q_i = dist of q_logprobs row i.  The arithmetic is fp64, rounded to fp32 where a value is stored or tested.
 *   u_i = ((w >> 8) + 0.5) * 2^-24 in fp32, w = word 0 of the Philox-4x32-10 block with key seed and counter {0xFFFFFFFE, 0, call lo, call
 *     hi}, call = c + i: XTC's coin construction on an index word that neither the coin (0xFFFFFFFF) nor a vocabulary index (<= V / 4) uses.
 *   Draft i is accepted iff 0 <= draft[i] < V and Q_i(draft[i]) > 0 and u_i * Q_i(draft[i]) < P_i(draft[i]) (fp32 values, one fp32 multiply,
 *     one fp32 compare); n_acc = the length of the accepted prefix; an id outside [0, V) is never used as an index.
 *   n_acc < rows - 1, j = n_acc: the last token is what pie_sample(PIE_SAMPLE_CATEGORICAL, temp = 1) draws at counter {c + j, 0} over the
 *     residual row R_j[x] = log(max(0, P_j(x) - Q_j(x))), -inf where the difference is <= 0 -- bit for bit, through pie_sample's launches.
 *     FALLBACK: if every entry of R_j is -inf (Q_j covers P_j: the refusal came from an id outside the vocabulary), the last token is
 *     pie_sample's ordinary draw from row j at {c + j, 0}.
 *   n_acc == rows - 1: the last token is pie_sample's ordinary draw from row rows - 1 at {c + rows - 1, 0}, the bonus token.
 *   out_tokens [rows] = the accepted drafts, the last token, then -1; out_n [1] = n_acc + 1; afterwards counter = {c + out_n, 0}.
 *   accept_rec (nullable) fp32 [rows - 1, 3] = (P_i(d_i), Q_i(d_i), u_i) of EVERY draft (0, 0 for an id outside the vocabulary); residual
 *     (nullable) fp32 [rows, V]: rows 0 .. rows - 2 = R_i, row j holding the bits drawn from; row rows - 1 is not written.  Diagnostics.
 * 19 launches: the partials and the finish over every row (2), one workgroup that fills both filters' records (1), pie_sample_rows' 5
 * over the target's rows -- whose draws are the rows' ordinary tokens -- and 5 over the drafter's, one over (ceil(V / 512), 2 rows - 1) for
 * the tiles' shares of the normalisers and one workgroup per row that merges them in a fixed order (2), one over ceil(V / 512) tiles --
 * times rows - 1 with the residual diagnostic -- that decides the drafts in every workgroup and writes R_j (1), pie_sample's 2, and one
 * workgroup that composes the tokens and stores the counter (1).  n_acc never visits the host.  No floating-point atomics, nothing
 * depends on arrival order: results are bit-identical from run to run.  workspace: pie_spec_verify_draft_workspace_bytes(rows, V) bytes
 * (0 for refused sizes), 16-byte aligned, ZEROED ONCE by the caller (as pie_sample's) and reusable from call to call.  Each before any
 * launch: a null pointer (the diagnostics excepted), mode PIE_SAMPLE_GREEDY (a greedy draft is a point mass: pie_spec_verify), a dtype that
 * is neither PIE_BF16 nor PIE_F16, a parameter outside pie_sample's rules: PIE_E_ARG; rows outside 2..32, V outside 1..524288: PIE_E_SHAPE;
 * logits not 2-byte, draft, q_logprobs or an output not 4-byte, the counter not 8-byte, the workspace not 16-byte aligned: PIE_E_ALIGN. */
size_t pie_spec_verify_draft_workspace_bytes(int rows, int V);
int pie_spec_verify_draft(const void *logits, int rows, int V, int dtype, const int32_t *draft, const float *q_logprobs, int mode, double temp, double p, int k,
                          unsigned long long seed, unsigned long long *counter, int32_t *out_tokens, int32_t *out_n, float *logprobs, float *accept_rec, float *residual,
                          void *workspace, void *stream);

/* ---------------------------------------------------------------- fused decode step
 * One forward of Model.__call__ (models/llama/language.py:199-210) for inputs[1,1] over per-layer
 * ReusableKVCache buffers (cache/kv_cache/reusable.py:96-142) followed by the tail of _inference
 * (engine/inference_engine.py:252-271) with the greedy sampler, as 5 launches per layer (6 beyond 1024 positions):
 *   rmsnorm+qkv GEMV+RoPE+cache append | split-KV attention | [combine] | split merge+o_proj+residual |
 *   rmsnorm+gate/up GEMV+SwiGLU | down_proj+residual ; then rmsnorm+lm_head ; log-softmax+argmax.
 * 4 per layer for models with 32 query / 8 kv heads of 128 and hidden <= 4096 (Llama-3-8B, Mistral-7B; any weight format) on a contiguous or T-page cache up to 1024 positions: the
 * attention then runs inside the q|k|v launch, behind an XCD-local seam (PIE_KNOB_FUSE_ATTN; bit-identical), which also merges its splits, so
 * o_proj takes one attention vector (PIE_KNOB_ATTN_MERGE_IN_LAUNCH; bit-identical).
 * Position and token live in device memory so the captured hipGraph is replayable. */
typedef struct pie_decoder pie_decoder;

typedef struct {
    int dtype;          /* PIE_BF16 / PIE_F16 */
    int hidden, n_layers, n_heads, n_kv_heads, head_dim, inter, vocab;
    float rms_eps;
    int tie_word_embeddings; /* lm_head = embed_tokens.as_linear (language.py:206-207) */
    int kv_splits;      /* split-KV factor of the attention kernel (0 = default) */
    int weight_format;  /* PIE_W_INT4_G64 (MLX int4 group-64 triplets, W4S units) or PIE_W_DENSE (16-bit nn.Linear
                           weights, W16S units; embed_codes is then the T [vocab, hidden] table, scales/biases NULL) */
    int rope_traditional; /* ModelArgs.rope_traditional (language.py:27,69): rotate the interleaved pairs (2i, 2i+1); wqkv is
                             then the plain q|k|v concatenation (row_map NULL), not pie_qkv_row_map's order */
    int tp_rank, tp_world; /* tensor parallelism (0, 0 or 0, 1 = none).  With tp_world > 1 this decoder is ONE RANK's shard:
                             n_heads, n_kv_heads, inter and vocab are the LOCAL sizes (heads / world, intermediate / world, vocabulary
                             rows / world: proxy_inference_engine_amd/tp.py shard_config), hidden is the full width, the embedding
                             table holds all vocab * tp_world rows.  o_proj / down_proj produce fp32 partial sums that
                             pie_decoder_set_comm's communicator adds over the ranks before the one rounding + residual add. */
} pie_decoder_config;
enum { PIE_W_INT4_G64 = 0, PIE_W_DENSE = 1, PIE_W_INT8_G64 = 2 /* W8S units, embed_codes uint32 [vocab, hidden/4] */,
       PIE_W_INT4_G32 = 3 /* W4S32 units, embed scales / biases [vocab, hidden/32] */, PIE_W_INT8_G32 = 4 /* W8S32 units */,
       PIE_W_INT2_G64 = 5 /* W2S units (Linear matrices only: per-matrix fmt_* or the default with fmt_embed = PIE_W_INT4_G64 + 1) */,
       PIE_W_INT6_G64 = 6 /* W6S units (Linear matrices only; the embedding table as 8-bit codes, fmt_embed = PIE_W_INT8_G64 + 1) */ };

typedef struct {
    const void *attn_norm, *mlp_norm;   /* T [hidden] */
    const void *wqkv;                    /* W4S of [q;k;v] rows in RoPE-paired order (pie_qkv_row_map) */
    const void *wo;                      /* W4S [hidden, n_heads*head_dim] */
    const void *wgateup;                 /* W4S of interleaved (gate_i, up_i) rows */
    const void *wdown;                   /* W4S [hidden, inter] */
    /* optional Linear biases (attention_bias / mlp_bias, models/llama/language.py:42-53,117-126), T, NULL = none;
       bqkv in the packed q|k|v row order (pie_qkv_row_map), bgateup interleaved (pie_gateup_row_map) */
    const void *bqkv, *bo, *bgateup, *bdown;
    /* Per-matrix weight format: 0 = the decoder's weight_format, else PIE_W_* + 1.  The reference decides quantisation PER MODULE
       (models/utils.py:99-109: quantised iff the checkpoint holds "{path}.scales" and the input width is a multiple of 64), so a
       checkpoint may mix int4 and 16-bit Linears; the fused groups (q|k|v, gate|up) must be uniform inside. */
    int fmt_qkv, fmt_o, fmt_gateup, fmt_down;
} pie_layer_weights;

typedef struct {
    const uint32_t *embed_codes;         /* MLX layout [vocab, hidden/8] */
    const void *embed_scales, *embed_biases; /* T [vocab, hidden/64] */
    const void *final_norm;              /* T [hidden] */
    const void *lm_head;                 /* W4S [vocab, hidden] (of embed_tokens when tied) */
    const float *rope_freqs;             /* fp32 [head_dim/2], Llama3RoPE._freqs (models/llama/utils.py:39) */
    int fmt_embed, fmt_lm_head;          /* 0 = the decoder's weight_format, else PIE_W_* + 1 (see pie_layer_weights); a dense embedding:
                                            embed_codes is the T [vocab, hidden] table, scales / biases NULL */
} pie_global_weights;

/* Host helpers producing the row maps the decoder's fused epilogues assume (host int32 arrays). */
int pie_qkv_row_map(int n_heads, int n_kv_heads, int head_dim, int32_t *map /* [(n_heads+2*n_kv_heads)*head_dim] */);
int pie_gateup_row_map(int inter, int32_t *map /* [2*inter], source rows of cat(gate, up) */);

int pie_decoder_create(const pie_decoder_config *cfg, pie_decoder **out);
int pie_decoder_destroy(pie_decoder *d);
int pie_decoder_set_layer(pie_decoder *d, int layer, const pie_layer_weights *w);
int pie_decoder_set_globals(pie_decoder *d, const pie_global_weights *w);
/* Per-layer cache buffers [n_kv_heads, capacity, head_dim] T (ReusableKVCache.keys/values with B=1);
 * call again whenever a cache re-allocates (reusable.py:167-203).  k_ptrs/v_ptrs: HOST arrays of device pointers. */
int pie_decoder_set_kv(pie_decoder *d, const void *const *k_ptrs, const void *const *v_ptrs, int capacity, void *stream);
/* Paged alternative to pie_decoder_set_kv (the role of the reference's stub PagedKVCache,
 * cache/kv_cache/paged.py:1-14, over its PageAllocator): slabs = HOST array [n_layers] of device slab pointers (one
 * pie_page_pool geometry each, the same page ids valid in all of them), block_table = DEVICE int32 [max_blocks], caller-owned
 * and editable between steps (logical block j of the sequence -> page id).  Position p is stored in / read from page
 * block_table[p / 64], row p % 64; the caller must have filled the table for every position a step or prefill touches.
 * Capacity = max_blocks * 64.  Steps, prefill, graphs and outputs behave exactly as with contiguous buffers. */
int pie_decoder_set_paged_kv(pie_decoder *d, const void *const *slabs, size_t n_pages, const int32_t *block_table, int max_blocks,
                             void *stream);
/* One decode step for B sequences at once over the paged KV pool (continuous batching): the weights stream once for all rows;
 * row s is its own sequence -- input token tokens[s], attending context_lens[s] positions INCLUDING the new one (its position is
 * context_lens[s] - 1; 0 = idle slot), K / V appended to page block_tables[s][pos / 64] of every layer's slab (slabs: HOST array
 * [n_layers] of device pointers), attention over its own table row.  Outputs per row: logits T [B, vocab], logprobs fp32
 * [B, vocab], next_tokens int32 [B] (greedy).  What the reference's decode-state batch is meant to be (BatchDetails,
 * include/engine/batch_details.hpp:10-88; Scheduler and the paged attention kernel are skeletons there).  Independent of
 * pie_decoder_set_kv / set_state / bind_outputs; all device arrays are caller-owned.  flags: PIE_STEP_GRAPH replays a captured
 * hipGraph of the step while the caller passes the same buffers (their contents may change) -- captured on the second such call. */
int pie_decoder_step_batch(pie_decoder *d, const int32_t *tokens, const int32_t *context_lens, const void *const *slabs, size_t n_pages, size_t slab_bytes,
                           const int32_t *block_tables, int max_blocks, int B, void *logits, float *logprobs, int32_t *next_tokens,
                           int flags, void *stream);
/* Several FRESH prompts in one pass (the prefill-state half of BatchDetails, batch_details.hpp:10-88): their N rows are
 * concatenated -- ids [N]; per row: row_context_lens (position + 1), row_seq (which prompt, = its block-table row), seg_lo
 * (index of its prompt's first row), seg_hi (row index + 1: causal); per prompt: last_rows [S] (index of its last row).  K / V
 * go to each prompt's pages; attention reads this pass's own rows.  Outputs per prompt as in pie_decoder_step_batch.
 * All index arrays are device int32.  slab_bytes (here and in pie_decoder_step_batch): the size of EACH layer's slab; it must hold
 * n_pages pages of the ACTIVE page format (T pages, or int8 pages under PIE_OPT_KV_I8) -- a pool of the other format is refused
 * instead of being indexed with the wrong page stride. */
int pie_decoder_prefill_batch(pie_decoder *d, const int32_t *ids, const int32_t *row_context_lens, const int32_t *row_seq, const int32_t *seg_lo,
                              const int32_t *seg_hi, const int32_t *last_rows, int N, int S, const void *const *slabs, size_t n_pages, size_t slab_bytes,
                              const int32_t *block_tables, int max_blocks, void *logits, float *logprobs, int32_t *next_tokens, void *stream);
/* A MIXED batch: decode-state sequences and prompts in ONE pass over the weights (batch_details.hpp:10-88 holds both kinds in one
 * BatchDetails; the scheduler body that would form it is empty upstream).  The layout of pie_decoder_prefill_batch with n_decode decode
 * rows in front: row r < n_decode is sequence r (row_seq[r] == r, block-table row r) with its input token ids[r], row_context_lens[r] =
 * the positions it attends INCLUDING the new one, seg_lo[r] = r, seg_hi[r] = r + 1; the prompts' rows follow with row_seq >= n_decode.
 * out_rows [S]: the rows whose logits are wanted -- the n_decode decode rows first, then every prompt's last row.  The decode rows'
 * attention runs over their pages (pie_decoder_step_batch's kernel), a fresh prompt's rows' over this pass's own rows.
 * chunks_host (HOST int32 [n_chunks][4] = {first row, rows, cached positions, sequence}; n_chunks may be 0): prompts that CONTINUE a cached
 * prefix -- a chunk of a long prompt, or a suffix behind shared prefix pages (KVPage ref counts, page.hpp:55-68).  Their rows carry
 * row_context_lens = cached + i + 1 and trivial segments (seg_lo = r, seg_hi = r + 1); their attention is the single-prompt causal flash
 * kernel over the sequence's pages from that offset.  T pages only.  n_decode == 0 and n_chunks == 0 is pie_decoder_prefill_batch. */
int pie_decoder_step_mixed(pie_decoder *d, const int32_t *ids, const int32_t *row_context_lens, const int32_t *row_seq, const int32_t *seg_lo,
                           const int32_t *seg_hi, const int32_t *out_rows, int N, int S, int n_decode, const void *const *slabs, size_t n_pages,
                           size_t slab_bytes, const int32_t *block_tables, int max_blocks, void *logits, float *logprobs, int32_t *next_tokens,
                           int n_chunks, const int32_t *chunks_host, void *stream);
/* offset = cache.offset before the step (reusable.py:111); token < 0 keeps the device-side token (the
 * previous step's argmax). */
int pie_decoder_set_state(pie_decoder *d, int offset, int token, void *stream);
/* Runs one step.  flags: PIE_STEP_LOGITS computes lm_head + logprobs + argmax (else the step only fills
 * the KV caches: prompt tokens before the last); PIE_STEP_GRAPH replays a captured hipGraph of the step
 * (captured on first use per flag set).  After the step the device-side offset is incremented and, with
 * PIE_STEP_LOGITS, the device-side token is the greedy choice. */
enum { PIE_STEP_LOGITS = 1, PIE_STEP_GRAPH = 2 };
int pie_decoder_step(pie_decoder *d, int flags, void *stream);
/* Kernel nodes of the captured step graph (read back with hipGraphGetNodes when it was instantiated); -1 while no step with these flags has
 * been captured.  bench.py reports it as config.launches_per_step. */
int pie_decoder_graph_launches(const pie_decoder *d, int flags);
/* Prompt processing: Model.__call__(inputs[1, L]) from the current device-side offset, ids[0..L) device int32, all
 * launches queued back to back with no host round trip.  L >= 6 (pie_set_knob(PIE_KNOB_PREFILL_MIN, n)): batched, in chunks of
 * 4096 rows (PIE_KNOB_PREFILL_CHUNK) -- MLX's qmm regime: nn.QuantizedLinear at L > 1 dequantises to T before a T x T -> fp32 MMA.
 * int4 group-64 matrices run hand-written MFMA GEMMs straight from their 4-bit tiles (k_w4r_gemm up to 256 rows, k_w4l2_gemm beyond);
 * dense, int8 and group-32 matrices multiply a 16-bit copy in MFMA-ordered tiles (W16M; k_w16l_gemm -- no library GEMM since round 5;
 * in_features % 64 == 0), with HIP kernels for RMSNorm, RoPE + cache append, causal attention, SwiGLU and residuals.  Shorter prompts: iterated decode steps (the qmv regime).  logits_all == NULL: lm_head + tail only for the last token (the engine only
 * reads logits[:, -1, :], engine/inference_engine.py:254).  logits_all != NULL: T [L, vocab], lm_head on every
 * position like the reference's Model.__call__ (language.py:205-209). */
int pie_decoder_prefill(pie_decoder *d, const int32_t *ids, int L, void *logits_all, void *stream);
/* The same with the input embeddings given instead of token ids: embeds T [L, hidden] replaces embed_tokens(ids) --
 * `h = inputs_embeds` of the VLM text tower (models/intern/language.py:155-158), fed by the ensemble's merged text and image
 * features (models/intern/ensemble.py:33-91, :106-108).  Always the batched path, whatever L -- except on int8 pages (PIE_OPT_KV_I8 with a
 * paged cache), where the rows run as decode steps like a prompt of tokens does there. */
int pie_decoder_prefill_embeds(pie_decoder *d, const void *embeds, int L, void *logits_all, void *stream);
/* Output buffers of the step, allocated by the caller (device): logits T [vocab], logprobs fp32 [vocab],
 * token int32 [1] (the greedy choice), hidden T [hidden] (the residual stream; after a step it holds the
 * output of the last block, the input of the final norm).  history (optional, int32 [history_len]): the tail
 * kernel stores the greedy token chosen for position p at history[p], so the host can read the generated ids
 * later in one copy instead of synchronising every step (PromptCache.computed_ids, cache/prompt_cache.py:43-50).
 * Required before the first step. */
int pie_decoder_bind_outputs(pie_decoder *d, void *logits, float *logprobs, int32_t *token, void *hidden, int32_t *history,
                             int history_len);
/* Copies a device-resident token id into the decoder's device-side state (the input of the next
 * pie_decoder_step) without a host round trip; a no-op when `token_dev` is the bound token output. */
int pie_decoder_set_token_from(pie_decoder *d, const int32_t *token_dev, void *stream);
/* The step's configurable tail: the engine's two generation knobs inside the launch sequence, so that a request with a
 * repetition penalty or a stochastic sampler still costs one graph replay per token and no host synchronisation.  The configuration applies
 * wherever the tail writes the BOUND outputs: pie_decoder_step with PIE_STEP_LOGITS (eager or PIE_STEP_GRAPH) and the last row of
 * pie_decoder_prefill / _prefill_embeds with logits_all == NULL; with logits_all != NULL the logits stay raw and the tail greedy.  Order:
 * lm_head | penalty on the bound logits (which then hold the processed logits) | per-tile partials recomputed from them (pie_logprobs_argmax's
 * own partition, so logprobs and the greedy token are bit-identical with pie_logprobs_argmax of the bound logits) | finish | pie_sample's
 * launches over the bound logprobs; the drawn id becomes *token, the fed-back token and history[new position].  Any cache kind; refused
 * (PIE_E_STATE) on tensor-parallel decoders, whose tail is vocabulary-parallel.  pie_decoder_step_batch / _prefill_batch / _step_mixed ignore
 * it (their own tail: pie_decoder_set_batch_tail).  A change of either setting (the seed included: it is a launch argument) drops the captured graphs; with neither set the step is
 * exactly the unconfigured one.
 * pie_decoder_set_logits_penalty: pie_logits_penalty over the ids the model was fed at positions max(0, p + 1 - context_size) .. p, p = the
 *   position the tail processes (the row's own input id included, the token about to be chosen not: prompt_cache.update runs before the
 *   processors, inference_engine.py:255-266).  ids_by_pos: caller-owned DEVICE int32 [ids_cap], ids_by_pos[q] = the id fed at position q.  The
 *   caller writes every id it passes explicitly (a prompt's rows, an explicit single token); a step records its input token -- the
 *   device-side state's -- at ids_by_pos[p] itself before it penalises, so fed-back tokens need no host.  Every index is checked against
 *   ids_cap on the device.  penalty == 1.0 or context_size == 0 switches it off; otherwise penalty finite and >= 0, context_size 1..1024.
 * pie_decoder_set_sampler: mode PIE_SAMPLE_GREEDY restores the greedy tail; otherwise pie_sample's modes, argument checks, random stream
 *   (seed, DEVICE counter) and workspace (pie_sample_workspace_bytes(1, vocab) bytes, zeroed once by the caller), all caller-owned and
 *   alive while set. */
int pie_decoder_set_logits_penalty(pie_decoder *d, double penalty, int context_size, int32_t *ids_by_pos, int ids_cap);
int pie_decoder_set_sampler(pie_decoder *d, int mode, double temp, double p, int k, unsigned long long seed, unsigned long long *counter,
                            void *workspace, size_t workspace_bytes);
/* Token mask and logit bias in the step's configured tail, applied wherever that tail applies (above).  The processed
 * logits are what this sequence gives on T: (1) mask: pie_logprobs_argmax_masked's rule; (2) the repetition penalty, exactly as above;
 * (3) bias: pie_logits_bias; then the unchanged log-softmax, finish and draw.  The bound logits hold the processed logits afterwards, and
 * the bound logprobs and the greedy token are bit-identical with pie_logprobs_argmax of them.  RULE: a masked id is -inf in the processed
 * logits, whatever else is configured.  (The mask is applied physically last, inside the partials pass: -inf stays -inf under any
 * penalty > 0 and any finite bias.  The one deviation from the reference's order: with penalty == 0.0 a masked id inside the window is
 * -inf here, where -inf * 0 gives the reference a NaN and a NaN row.)  Launches beyond the unconfigured step's: mask alone 1 (the masked
 * partials); bias and / or penalty 2 (one edit launch, the partials), a mask on top of them none.
 * pie_decoder_set_logits_mask: mask DEVICE uint32 [mask_words >= ceil(vocab / 32)]; NULL switches it off.  mask_words too small:
 *   PIE_E_SHAPE; not 4-byte aligned: PIE_E_ALIGN.
 * pie_decoder_set_logit_bias: ids DEVICE int32 [n], bias DEVICE float [n], n 1..1024; n == 0 switches it off; n outside 0..1024: PIE_E_ARG; ids or bias not
 *   4-byte aligned: PIE_E_ALIGN.  With only a bias set the
 *   edit launch runs with its penalty phase off and records nothing in ids_by_pos.
 * Both keep caller-owned device memory that stays alive while set; its CONTENTS may change between steps (the host writes in stream
 * order and a captured graph keeps replaying).  Switching either on or off, a new address or a new n drops the captured graphs.
 * Tensor-parallel decoders refuse (PIE_E_STATE).  pie_decoder_step_batch / _prefill_batch / _step_mixed ignore both: they take per-row
 * masks and biases of their own (pie_decoder_set_batch_logits_edits). */
int pie_decoder_set_logits_mask(pie_decoder *d, const uint32_t *mask, int mask_words);
int pie_decoder_set_logit_bias(pie_decoder *d, const int32_t *ids, const float *bias, int n);
/* The multi-sequence passes' tail: per-row penalties and samplers inside pie_decoder_step_batch (eager or PIE_STEP_GRAPH),
 * pie_decoder_prefill_batch and pie_decoder_step_mixed.  table: DEVICE pie_row_tail [rows_cap], record s belongs to output row s (in the
 * two prompt passes the decoding rows first, then prompt j at n_decode + j: a request's first token is drawn by its own sampler);
 * recent_ids: DEVICE int32 [rows_cap, 1024]; workspace: pie_sample_workspace_bytes(rows_cap, vocab) bytes, zeroed once; all caller-owned
 * and alive while set.  With a table set the passes end in: lm_head | pie_logits_penalty_rows on the output logits (input ids and context
 * lengths: tokens / context_lens, or ids / row_context_lens / out_rows) | the unchanged log-softmax + argmax over every row |
 * pie_sample_rows into next_tokens.  logits then hold the processed logits and logprobs their log-softmax, each row bit-identical with
 * pie_logits_penalty + pie_logprobs_argmax + a one-row pie_sample of that row.  The records' CONTENTS may change between calls (the host
 * writes them in stream order) and a captured step keeps replaying; the three addresses and rows_cap are part of the captured graph's key.
 * table == NULL switches the tail off: the passes then launch exactly what they launch without it.  A pass with more output rows than
 * rows_cap is PIE_E_SHAPE before any launch; a misaligned table or workspace (8 bytes) or ring (4) PIE_E_ALIGN; tensor-parallel decoders
 * refuse the setter (PIE_E_STATE).  pie_decoder_batch_graph_replays: how many pie_decoder_step_batch calls so far were served by
 * replaying the captured graph (tests assert the replay branch with it); pie_decoder_batch_graph_launches: the kernel nodes of the
 * graph captured last (-1: none yet), what one replayed step launches. */
int pie_decoder_set_batch_tail(pie_decoder *d, pie_row_tail *table, int rows_cap, int32_t *recent_ids, void *workspace);
unsigned long long pie_decoder_batch_graph_replays(const pie_decoder *d);
int pie_decoder_batch_graph_launches(const pie_decoder *d);
/* Top-n log-probabilities inside the passes: pie_top_logprobs as the last launches of a tail, after the token is final.
 * pie_decoder_set_top_logprobs: the single-sequence step.  Applies wherever the configured tail applies (above: eager and PIE_STEP_GRAPH
 *   steps, the last row of pie_decoder_prefill / _prefill_embeds with logits_all == NULL), after the draw: slot 0 is the token that is fed
 *   back, on every KV binding.  out_ids int32 [n + 1], out_vals fp32 [n + 1], workspace of at least pie_top_logprobs_workspace_bytes(1, vocab, n)
 *   bytes (workspace_bytes; smaller: PIE_E_SHAPE), all caller-owned DEVICE memory, alive while set.  n == 0 switches it off; a decoder that does
 *   not set it launches exactly what it launches without; setting it, a new n or a new address drops the captured graphs;
 *   pie_decoder_graph_launches counts its 2 launches.
 * pie_decoder_set_batch_top_logprobs: pie_decoder_step_batch (eager or PIE_STEP_GRAPH), _prefill_batch and _step_mixed, after next_tokens
 *   are final (after pie_sample_rows with a batch tail, after the argmax without: the two settings are independent).  Record s = output
 *   row s (pie_decoder_set_batch_tail's row order): out_ids int32 [rows_cap, n + 1], out_vals fp32 [rows_cap, n + 1], count DEVICE int32
 *   [rows_cap] (NULL: n in every row) whose CONTENTS may change between calls while a captured step keeps replaying; workspace
 *   pie_top_logprobs_workspace_bytes(rows_cap, vocab, n) bytes.  The addresses, n and rows_cap are part of the captured graph's key.
 *   n == 0 switches it off.  A pass with more output rows than rows_cap is PIE_E_SHAPE before any launch.
 * Both: the op's argument rules; tensor-parallel decoders refuse (PIE_E_STATE). */
int pie_decoder_set_top_logprobs(pie_decoder *d, int n, int32_t *out_ids, float *out_vals, void *workspace, size_t workspace_bytes);
int pie_decoder_set_batch_top_logprobs(pie_decoder *d, int n, int rows_cap, int32_t *out_ids, float *out_vals, const int32_t *count, void *workspace);
/* Log-probabilities of prompt tokens inside the prompt passes: while set, record i = pie_prompt_logprobs' record of row i of
 * the call, for pie_decoder_prefill / _prefill_embeds (the batched path per chunk, the iterated path per step: every step then computes its
 * logits, as with logits_all, and the regime a prompt runs in does not depend on the setting) and for the prompt rows n_decode..N-1 of
 * pie_decoder_prefill_batch / _step_mixed (decode rows are not scored and their records stay untouched; pie_decoder_step_batch ignores the
 * setting).  The rows are scored in blocks of at most block_rows (8..1024): the lm_head on the block's final-normed rows, as the logits_all
 * branch multiplies it, into a T [block_rows, vocab] block at the head of the workspace, then the op's four launches.  The log-probabilities
 * are of the RAW model distribution, as logits_all is raw: configured masks, biases, penalties and samplers do not apply to prompt rows (on
 * the iterated path a row before the last ends in the raw greedy tail).  The library never guesses targets: the host writes targets[i] = the
 * id that follows row i in its prompt, across chunk boundaries too, and count[i] = -1 for a prompt's last row.
 *   targets, count DEVICE int32 [rows_cap], whose CONTENTS may change between calls; out_ids int32 [rows_cap, n + 1], out_vals fp32
 *   [rows_cap, n + 1]; workspace of at least pie_decoder_prompt_logprobs_workspace_bytes(d, n, block_rows) bytes (0 for refused sizes),
 *   16-byte aligned -- all caller-owned DEVICE memory, alive while set.  n == 0 switches it off; a decoder that does not set it launches
 *   exactly what it launches without.  The op's argument rules; block_rows outside 8..1024: PIE_E_ARG; tensor-parallel decoders refuse
 *   (PIE_E_STATE); a pass with more rows than rows_cap is PIE_E_SHAPE before any launch. */
size_t pie_decoder_prompt_logprobs_workspace_bytes(const pie_decoder *d, int n, int block_rows);
int pie_decoder_set_prompt_logprobs(pie_decoder *d, int n, int rows_cap, int block_rows, const int32_t *targets, const int32_t *count,
                                    int32_t *out_ids, float *out_vals, void *workspace, size_t workspace_bytes);
/* Per-row token masks and logit biases inside the multi-sequence passes: pie_decoder_step_batch (eager or PIE_STEP_GRAPH),
 * pie_decoder_prefill_batch and pie_decoder_step_mixed, output row s in pie_decoder_set_batch_tail's row order.  The processed logits of a row
 * are the single-sequence tail's (above) with the row's own parameters: (1) mask, (2) the row's repetition penalty from its pie_row_tail
 * record when a batch tail is set, (3) bias; then the unchanged log-softmax + argmax, pie_sample_rows and the top-n records.  A masked id is
 * -inf in the processed logits whatever else is configured (the mask is applied physically last, inside the partials pass).  logits then hold
 * the processed logits and logprobs their log-softmax, each row bit-identical with pie_logits_penalty over the ring's window +
 * pie_logits_bias + pie_logprobs_argmax_masked + a one-row pie_sample of that row alone.
 *   masks / mask_on    DEVICE uint32 [rows_cap, mask_words >= ceil(vocab / 32)] and int32 [rows_cap] as pie_logprobs_argmax_rows_masked takes
 *                      them: mask_on[s] == 0 leaves row s unmasked, bit for bit.  masks == NULL (then mask_on == NULL too): no mask part
 *   bias_ids / _vals / _n  DEVICE int32 / float [rows_cap, bias_cap] and int32 [rows_cap] as pie_logits_bias_rows takes them, bias_cap 1..1024;
 *                      bias_n[s] is clamped to [0, bias_cap] on the device, 0: none.  bias_cap == 0: no bias part
 * All five arrays are caller-owned and alive while set; their CONTENTS may change between calls in stream order while a captured step keeps
 * replaying; the addresses, rows_cap, mask_words and bias_cap are part of the captured graph's key, so switching a part on or off or changing
 * any of them leaves the captured batch graph behind.  rows_cap == 0 switches the edits off: the passes then launch exactly what they launch
 * without.  Independent of pie_decoder_set_batch_tail and of pie_decoder_set_batch_top_logprobs.  Launches: lm_head | pie_logits_penalty_rows,
 * or k_logits_edit_rows (the same row lookup, ring window and penalise phase, then the bias phase, in one launch) when a bias part is set | the partials, masked per row when a mask part
 * is set | finish | [pie_sample_rows] | [top-n]: per pass +0 for masks and +1 for a bias without a batch tail, +0 with one; the fused
 * few-sequence step, whose lm_head epilogue partials are stale after an edit, +1 / +2 without a batch tail and +0 with one.
 * rows_cap < 0, bias_cap outside 0..1024, neither part, a part with a NULL array: PIE_E_ARG; mask_words < ceil(vocab / 32): PIE_E_SHAPE; an
 * array not 4-byte aligned: PIE_E_ALIGN; a pass with more output rows than rows_cap: PIE_E_SHAPE before any launch; tensor-parallel
 * decoders refuse the setter (PIE_E_STATE). */
int pie_decoder_set_batch_logits_edits(pie_decoder *d, int rows_cap, const uint32_t *masks, int mask_words, const int32_t *mask_on,
                                       const int32_t *bias_ids, const float *bias_vals, const int32_t *bias_n, int bias_cap);
/* Frequency and presence penalties inside the passes: pie_logits_count_penalty_rows' kernel as step (4) of a tail -- after
 * the mask's, the repetition penalty's and the bias' turn in the order above, before the log-softmax (whose partials are recomputed from the
 * processed logits: k_logits_stats, as after a penalty or a bias; in the fused few-sequence step too).  One more launch per pass, plus
 * the partials launch where nothing else had made them stale already.
 * pie_decoder_set_count_penalty: the single-sequence tail, wherever the configured tail applies (pie_decoder_step with PIE_STEP_LOGITS, eager
 *   or PIE_STEP_GRAPH; the last row of pie_decoder_prefill / _prefill_embeds with logits_all == NULL -- with logits_all != NULL the logits
 *   stay raw), on every KV binding.  record: DEVICE pie_count_penalty, counts: DEVICE int32 [vocab], caller-owned and alive while set.  A step
 *   takes its position and input id from the device-side state (the fed-back token, or the explicit one) and counts it under the rule
 *   above; a prompt pass counts nothing (its rows are prompt tokens) and applies the penalty from the counts as they are.  The record's and
 *   the counts' CONTENTS may change between steps in stream order while a captured graph keeps replaying; the two addresses are launch
 *   arguments: setting, clearing or moving them drops the captured graphs.  record == NULL switches it off.  A null counts with a record:
 *   PIE_E_ARG; misaligned (4 bytes): PIE_E_ALIGN.
 * pie_decoder_set_batch_count_penalty: pie_decoder_step_batch (eager or PIE_STEP_GRAPH), _prefill_batch and _step_mixed; record s and counts
 *   row s belong to output row s in pie_decoder_set_batch_tail's row order, with the pass's own ids / context lengths / output rows as the
 *   op's ids / ctx / out_rows.  records DEVICE pie_count_penalty [rows_cap], counts DEVICE int32 [rows_cap, vocab].  Independent of the batch
 *   tail, the batch edits and the batch top-n setters; the addresses and rows_cap are part of the captured batch graph's key.
 *   records == NULL switches it off.  rows_cap < 1, a null counts: PIE_E_ARG; misaligned: PIE_E_ALIGN; a pass with more output rows than
 *   rows_cap: PIE_E_SHAPE before any launch.
 * With neither set every pass launches exactly what it launches without.  Tensor-parallel decoders refuse both (PIE_E_STATE). */
int pie_decoder_set_count_penalty(pie_decoder *d, pie_count_penalty *record, int32_t *counts);
int pie_decoder_set_batch_count_penalty(pie_decoder *d, pie_count_penalty *records, int32_t *counts, int rows_cap);
/* The DRY penalty inside the passes: the op's kernels as step (5) of a tail, behind the count penalties and in front of the
 * log-softmax, whose partials are recomputed from the processed logits as after every other edit (in the fused few-sequence step too).
 * One more launch per pass, plus the partials launch where nothing else had made them stale already.
 * pie_decoder_set_dry_penalty: the single-sequence tail, wherever the configured tail applies (pie_decoder_step with PIE_STEP_LOGITS, eager
 *   or PIE_STEP_GRAPH; the last row of pie_decoder_prefill / _prefill_embeds with logits_all == NULL -- with logits_all != NULL the logits
 *   stay raw), on every KV binding.  record: DEVICE pie_dry_penalty; breakers: DEVICE int32 [PIE_DRY_BREAKERS_MAX]; ids_by_pos: DEVICE int32
 *   [ids_cap], the id fed at every position (pie_decoder_set_logits_penalty's; a step records its input token there first, and every index
 *   is checked against ids_cap).  All caller-owned and alive while set; their CONTENTS may change between steps in stream order while a
 *   captured graph keeps replaying; the addresses and ids_cap are launch arguments: setting, clearing or moving them drops the captured
 *   graphs.  record == NULL switches it off.  A null breakers or ids_by_pos with a record, ids_cap < 1: PIE_E_ARG; misaligned (4 bytes):
 *   PIE_E_ALIGN.
 * pie_decoder_set_batch_dry_penalty: pie_decoder_step_batch (eager or PIE_STEP_GRAPH), _prefill_batch and _step_mixed; record s, breakers
 *   row s and ring s belong to output row s, with the pass's own ids / context lengths / output rows as the op's.  records DEVICE [rows_cap],
 *   breakers DEVICE int32 [rows_cap, PIE_DRY_BREAKERS_MAX], recent_ids DEVICE int32 [rows_cap, 1024]: a ring of its own, so the setter is
 *   independent of the batch tail, the batch edits, the batch counts and the batch top-n setters; the addresses and rows_cap are part of the
 *   captured batch graph's key.  records == NULL switches it off.  rows_cap < 1, a null array: PIE_E_ARG; misaligned: PIE_E_ALIGN; a pass
 *   with more output rows than rows_cap: PIE_E_SHAPE before any launch.
 * With neither set every pass launches exactly what it launches without.  Tensor-parallel decoders refuse both (PIE_E_STATE), and
 * pie_decoder_spec_step refuses a configured DRY penalty like every other tail. */
int pie_decoder_set_dry_penalty(pie_decoder *d, const pie_dry_penalty *record, const int32_t *breakers, int32_t *ids_by_pos, int ids_cap);
int pie_decoder_set_batch_dry_penalty(pie_decoder *d, const pie_dry_penalty *records, const int32_t *breakers, int32_t *recent_ids, int rows_cap);
/* XTC inside the passes: the configured sampler draws with pie_sample_xtc / pie_sample_rows_xtc instead of pie_sample /
 * pie_sample_rows: one launch more per pass.  The bound logits, logprobs and top-n records stay those of the distribution before XTC.
 * pie_decoder_set_xtc: the single-sequence tail, wherever pie_decoder_set_sampler's sampler draws.  record: DEVICE pie_xtc, caller-owned
 *   and alive while set; its CONTENTS may change between steps in stream order while a captured graph keeps replaying; the address is a
 *   launch argument: setting, clearing or moving it drops the captured graphs.  NULL switches it off.
 * pie_decoder_set_batch_xtc: pie_decoder_step_batch (eager or PIE_STEP_GRAPH), _prefill_batch and _step_mixed; record s belongs to output
 *   row s in pie_decoder_set_batch_tail's row order.  records DEVICE [rows_cap]; the address and rows_cap are part of the captured batch
 *   graph's key.  NULL switches it off.  rows_cap < 1: PIE_E_ARG; a pass with more output rows than rows_cap: PIE_E_SHAPE before any launch.
 * Without a sampler (or a batch tail) to act on, a set record is a NO-OP: the greedy tail runs exactly what it runs without, and the record
 * takes effect as soon as a sampler is set.  Misaligned (4 bytes): PIE_E_ALIGN.  Tensor-parallel decoders refuse both (PIE_E_STATE), and
 * pie_decoder_spec_step refuses a set record like every other tail. */
int pie_decoder_set_xtc(pie_decoder *d, const pie_xtc *record);
int pie_decoder_set_batch_xtc(pie_decoder *d, const pie_xtc *records, int rows_cap);
/* Token automaton: a grammar as a token-level DFA compressed by token classes, whose state lives on the device.  An automaton
 * over a vocabulary of V ids with S states and C classes is V + S * C consecutive int32 words inside a caller-owned DEVICE arena
 * `tables` [tables_len]: cls [V] (token id -> class in [0, C)), then trans [S, C] (the next state in [0, S), or -1: not allowed).  Token t
 * is allowed in state s iff trans[s, cls[t]] >= 0.  A row is a record pie_row_dfa (word offsets into the arena) and a state (int32), both
 * DEVICE memory whose CONTENTS the host may rewrite in stream order, and neither is trusted.  A row is ARMED iff n_states > 0 and
 * n_classes > 0, both offsets >= 0, cls_off + V <= tables_len and trans_off + n_states * n_classes <= tables_len (in 64 bits); an id
 * whose class lies outside [0, n_classes) is disallowed.  An all-zero record is unarmed.
 * pie_token_dfa_mask: records [rows], states [rows]; masks DEVICE uint32 [rows, mask_words >= ceil(V / 32)] in pie_logprobs_argmax_masked's
 *   bit layout; mask_on nullable DEVICE int32 [rows] (pie_logprobs_argmax_rows_masked's).  Armed row, state in [0, S): words 0 ..
 *   ceil(V / 32) - 1 of the row are written (bits at or beyond V as 0; later words are never touched) and mask_on[row] = 1.  Armed row,
 *   state outside [0, S) -- the automaton has been left, or is finished: mask_on[row] = 0 and the words are left alone; without mask_on
 *   the words are written all-allowed below V.  Unarmed row: nothing of the row is written -- a mask the host wrote survives.
 * pie_token_dfa_advance: tokens DEVICE int32 [rows].  Armed row with a state in [0, S): states[row] = trans[s, cls[token]] for a token
 *   in [0, V) whose class is in range, -1 for any other token.  A state outside [0, S) stays what it is; an unarmed row is untouched.
 * Both: one launch.  A NULL pointer (but mask_on): PIE_E_ARG; rows outside 1..65535, V < 1, tables_len < 1, mask_words < ceil(V / 32):
 * PIE_E_SHAPE; a pointer not 4-byte aligned: PIE_E_ALIGN -- all before any launch.
 * pie_decoder_set_token_dfa: the single-sequence step derives its token mask from the state and advances the state by the token it feeds
 *   back, inside the replayed graph.  record: one pie_row_dfa, state: one int32, tables [tables_len], mask [mask_words >= ceil(vocab /
 *   32)] (the buffer the part writes and the masked partials read) -- all caller-owned DEVICE memory, alive while set.  Wherever the
 *   configured tail applies: pie_token_dfa_mask first | the edits | the partials, masked with `mask` | finish, sampler, top-n |
 *   pie_token_dfa_advance on the bound token, after the draw.  With logits_all != NULL nothing of it runs and the state does not move.
 *   Launches beyond the unconfigured step's: alone 3 (pie_decoder_set_logits_mask's 1, plus 2); with a bias and / or a penalty 4.  The
 *   CONTENTS of record, state and tables may change between steps in stream order while a captured graph keeps replaying; a new address or
 *   size drops the captured graphs.  record == NULL switches it off.  Mutually exclusive with pie_decoder_set_logits_mask: whichever is
 *   set second is refused (PIE_E_STATE).  pie_decoder_spec_step_tail refuses a set automaton by name; tensor-parallel decoders refuse the
 *   setter (PIE_E_STATE).  The op's argument rules.
 * pie_decoder_set_batch_token_dfa: pie_decoder_step_batch (eager or PIE_STEP_GRAPH, the fused few-sequence form included),
 *   _prefill_batch and _step_mixed; record s and state s belong to output row s in pie_decoder_set_batch_tail's row order.  records DEVICE
 *   pie_row_dfa [rows_cap], states DEVICE int32 [rows_cap], tables [tables_len].  Needs pie_decoder_set_batch_logits_edits with a mask
 *   part set first (else PIE_E_STATE; a pass that finds the mask part gone is PIE_E_STATE before any launch): pie_token_dfa_mask over
 *   the pass's output rows writes the armed rows' words and mask_on entries into that part's arrays in front of the tail, so an unarmed
 *   row keeps the mask the host wrote, or none; pie_token_dfa_advance on next_tokens follows the rows' samplers.  +2 launches on every
 *   path, relative to masks alone.  The addresses, tables_len and rows_cap are part of the captured batch graph's key.  rows_cap == 0
 *   switches it off.  A pass with more output rows than rows_cap is PIE_E_SHAPE before any launch; tensor-parallel decoders refuse. */
typedef struct pie_row_dfa {
    int32_t cls_off, trans_off, n_states, n_classes;
} pie_row_dfa;
int pie_token_dfa_mask(const pie_row_dfa *records, const int32_t *states, const int32_t *tables, int tables_len, int rows, int V, uint32_t *masks,
                       int mask_words, int32_t *mask_on, void *stream);
int pie_token_dfa_advance(const pie_row_dfa *records, int32_t *states, const int32_t *tables, int tables_len, int rows, int V, const int32_t *tokens,
                          void *stream);
int pie_decoder_set_token_dfa(pie_decoder *d, const pie_row_dfa *record, int32_t *state, const int32_t *tables, int tables_len, uint32_t *mask,
                              int mask_words);
int pie_decoder_set_batch_token_dfa(pie_decoder *d, int rows_cap, const pie_row_dfa *records, int32_t *states, const int32_t *tables, int tables_len);
/* One speculative pass of the single-sequence decoder: m = n_draft drafted ids (draft_ids DEVICE int32 [m]) are verified in one
 * pass over the weights.  In order: (1) rows [the device-side token, draft_0 .. draft_{m - 1}] are gathered on the device (a draft id the
 * embedding could not index is fed as id 0; pie_spec_verify never accepts it) and forwarded from the device-side offset through
 * pie_decoder_prefill's many-row pass with raw logits on every row into a block of the workspace; (2) pie_spec_verify on the block, into
 * out_tokens [m + 1], out_n [1] and logprobs_rows (nullable fp32 [m + 1, vocab]); (3) its last launch leaves the decoder as if out_n plain
 * greedy steps had run: the device-side offset advanced by out_n (not by m + 1), the device-side token and the bound token output = the last
 * accepted token, history[o + 1 + i] = accepted token i.  The K / V rows of rejected drafts stay behind the offset and are overwritten by
 * the positions that follow; nothing reads them.  The bound logits and log-probabilities hold row m's, accepted or not.
 * seq_ids (nullable DEVICE int32 [seq_cap]) = the sequence's ids by position, kept whole for pie_ngram_draft: seq_ids[o] = the fed token and
 * seq_ids[o + 1 + i] = accepted token i are written, every index checked against seq_cap; seq_len (nullable DEVICE int32 [1]) = o + out_n + 1,
 * the drafter's len for the next draft, so that a draft can be queued behind the pass before the host has read out_n.
 * The caller has made room for m + 1 rows at the offset (pie_decoder_set_kv / _set_paged_kv, block table filled).  4 launches (the gather and
 * pie_spec_verify's three) beyond pie_decoder_prefill's; nothing is captured in a graph, and a decoder
 * that never calls this entry launches exactly what it launches without it.
 * Speculation here is greedy and raw (the pass under a sampler, a repetition penalty and a logit bias is pie_decoder_spec_step_tail,
 * below).  PIE_E_STATE before any launch: a tensor-parallel decoder; a quantized or rotating KV cache; int8
 * pages (PIE_OPT_KV_I8); any configured tail (sampler, repetition penalty, mask, bias, top-logprobs, counts) or prompt scoring.
 * PIE_E_SHAPE before any launch: m + 1 below the many-row pass's first row count (PIE_KNOB_PREFILL_MIN, default 6: the rows would run as
 * iterated steps -- the host runs a plain step instead) or above 32.  workspace: pie_decoder_spec_workspace_bytes(d, m + 1) bytes (0 for
 * refused row counts), 16-byte aligned, caller-owned, no initialisation. */
size_t pie_decoder_spec_workspace_bytes(const pie_decoder *d, int rows);
int pie_decoder_spec_step(pie_decoder *d, const int32_t *draft_ids, int n_draft, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows, void *workspace,
                          int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream);
/* One speculative pass under the decoder's configured single-sequence tail: pie_decoder_spec_step's arguments and row bounds
 * (m + 1 rows, PIE_KNOB_PREFILL_MIN .. 32), except that logprobs_rows is REQUIRED and every one of its m + 1 rows is written.  With o = the
 * device-side offset, in order: (1) the gather and pie_decoder_prefill with raw logits on every row, as pie_decoder_spec_step; the pass's
 * own last-row tail stays raw and greedy, so the sampler's counter does not move there; (2) unless neither a repetition penalty nor a
 * logit bias is set, ONE edit launch, a workgroup per row r: pie_logits_penalty over the ids of positions max(0, o + r + 1 - context) ..
 * o + r -- ids_by_pos[q] for q < o, the device-side token for q == o (recorded at ids_by_pos[o], as the step's tail records its input),
 * draft[q - o - 1] for q > o (not recorded) -- then pie_logits_bias with the decoder's table: row r's processed logits are those of the
 * step's tail on that row alone; (3) pie_spec_verify_sampled's launches on the processed block with the decoder's mode / temp / p / k / seed
 * / counter / XTC record -- under the greedy sampler (a penalty and / or a bias only) the rows' tokens are the argmaxes of the processed
 * rows, nothing is drawn and the counter is untouched; (4) its accept launch leaves what pie_decoder_spec_step's leaves, and
 * ids_by_pos[o + 1 + i] = token i for i < out_n (with a penalty set), so that the plain step that follows finds its window whole, and the
 * counter = {c + out_n, 0}.  Afterwards the decoder is where out_n plain steps under the same tail would have left it, and the workspace's
 * block holds the PROCESSED logits.  3 or 4 launches (greedy sampler), 9 .. 11 otherwise, beyond the gather and pie_decoder_prefill's;
 * nothing is captured in a graph, and a decoder that never calls this entry launches exactly what it launches without it.
 * Accepted tail settings, at least one of which must be set (else PIE_E_STATE: that pass is pie_decoder_spec_step's):
 * pie_decoder_set_sampler (any mode), pie_decoder_set_xtc, pie_decoder_set_logits_penalty, pie_decoder_set_logit_bias.  PIE_E_STATE before
 * any launch: a token mask, a top-logprobs record, frequency / presence counts, a DRY penalty, prompt scoring, a tensor-parallel decoder, a
 * quantized or rotating KV cache, int8 pages.  workspace: pie_decoder_spec_tail_workspace_bytes(d, m + 1) bytes (0 for refused row
 * counts), 16-byte aligned, caller-owned, ZEROED ONCE and reusable from pass to pass. */
size_t pie_decoder_spec_tail_workspace_bytes(const pie_decoder *d, int rows);
int pie_decoder_spec_step_tail(pie_decoder *d, const int32_t *draft_ids, int n_draft, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows, void *workspace,
                               int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream);
/* The automaton along a draft.  record, state, tables: ONE row of pie_token_dfa_mask's, untrusted like there: every index a
 * kernel forms is checked against tables_len, V, S and C, and a record that is not armed constrains nothing.  Both ops: one launch of one wave.
 * pie_token_dfa_walk: tokens DEVICE int32 [n], 1 <= n <= 31 -> out_states DEVICE int32 [n + 1]: out_states[0] = *state, out_states[i + 1] =
 *   pie_token_dfa_advance's result for out_states[i] and tokens[i] -- a state outside [0, S) stays what it is; an unarmed record copies
 *   *state to every slot.  Neither *state nor anything else is modified.
 * pie_token_dfa_draft: the grammar-aware drafter.  forced DEVICE int32 [forced_states, 2], 8-byte aligned: row s = (t, next) when exactly one
 *   id t is allowed in state s and leads to next, else (-1, -1) (TokenAutomaton.forced()) -- a HINT: an entry is used only where the tables
 *   re-derive it.  cand DEVICE int32 [>= min(*cand_count, 31)]: a candidate draft (pie_ngram_draft's), cand_count DEVICE int32 [1], clamped
 *   on the device to [0, 31]; 1 <= k <= 31; out_ids DEVICE int32 [k] (may be cand), out_count DEVICE int32 [1] (may be cand_count).
 *     unarmed record, or s0 = *state outside [0, S): out_ids = cand[: min(cand_count, k)], out_count likewise
 *     s = s0; j = 0; live = true; n = 0
 *     while n < k:
 *         (f, fn) = forced[s] when s < forced_states, else (-1, -1)
 *         if 0 <= f < V and fn >= 0 and trans[s, cls[f]] == fn:  t, next = f, fn;  if live and j < cand_count and cand[j] == t: j += 1, else: live = false
 *         else if live and j < cand_count and cand[j] is allowed in s:  t, next = cand[j], trans[s, cls[cand[j]]];  j += 1
 *         else: stop
 *         out_ids[n] = t; n += 1; s = next;  stop when s is outside [0, S)
 *     out_count = n;  out_ids[n ..] keep their contents
 *   So a looked-up draft is cut at the first id the grammar forbids, a forced id replaces whatever was looked up (which ends the
 *   look-up's part), and without a look-up the grammar drafts its forced run.  Every id written is allowed in the state the ids before it
 *   lead to, whatever `forced` holds.  *state is not modified.
 * Both: a NULL pointer: PIE_E_ARG; n or k outside 1..31, V < 1, tables_len < 1, forced_states < 1: PIE_E_SHAPE; a pointer not aligned:
 * PIE_E_ALIGN -- all before any launch. */
int pie_token_dfa_walk(const pie_row_dfa *record, const int32_t *state, const int32_t *tables, int tables_len, int V, const int32_t *tokens, int n,
                       int32_t *out_states, void *stream);
int pie_token_dfa_draft(const pie_row_dfa *record, const int32_t *state, const int32_t *tables, int tables_len, const int32_t *forced, int forced_states, int V,
                        const int32_t *cand, const int32_t *cand_count, int k, int32_t *out_ids, int32_t *out_count, void *stream);
/* One speculative pass under a token automaton: pie_decoder_spec_step_tail's arguments, row bounds and settings PLUS
 * pie_decoder_set_token_dfa, which is REQUIRED (without one: PIE_E_STATE, the pass is pie_decoder_spec_step_tail's) and alone is enough.
 * With o the device-side offset and s0 the automaton's state, in order: (1) the gather and pie_decoder_prefill with raw logits on every row;
 * (2) pie_token_dfa_walk over draft_ids into states [m + 1] of the workspace (the same launch replicates the record per row and zeroes
 * mask_on); (3) pie_token_dfa_mask over the m + 1 rows into masks / mask_on of the workspace: a row whose state has left [0, S) is an
 * unmasked row; (4) pie_decoder_spec_step_tail's edit launch when a penalty or a bias is set; (5) pie_spec_verify_sampled's launches, the
 * partials masked per row (pie_logprobs_argmax_rows_masked's); (6) the accept launch also stores the automaton's state: states[out_n - 1]
 * advanced by token out_n - 1 under pie_token_dfa_advance's rule.  Row r's log-probabilities and token are those of the step's tail on that
 * row alone in state states[r] at stream position c + r; afterwards the decoder -- pos, tokens, history, ids_by_pos, seq_ids / seq_len, the
 * counter {c + out_n, 0} and the automaton's state -- is where out_n configured steps would have left it.  2 launches beyond
 * pie_decoder_spec_step_tail's; nothing is captured in a graph, and a decoder that never calls this entry launches exactly what it
 * launches without it.  PIE_E_STATE before any launch, each by name: no automaton; a token mask; a top-logprobs record; frequency /
 * presence counts; a DRY penalty; prompt scoring; a tensor-parallel decoder; a quantized or rotating KV cache; int8 pages.  workspace:
 * pie_decoder_spec_dfa_workspace_bytes(d, m + 1) bytes (0 for refused row counts), 16-byte aligned, caller-owned, ZEROED ONCE. */
size_t pie_decoder_spec_dfa_workspace_bytes(const pie_decoder *d, int rows);
int pie_decoder_spec_step_dfa(pie_decoder *d, const int32_t *draft_ids, int n_draft, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows, void *workspace,
                              int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream);
/* One speculative pass over a draft MODEL's block: pie_decoder_spec_step_tail's arguments, row bounds and order, plus
 * q_logprobs DEVICE fp32 [m, vocab] (the drafter's log-probabilities at the step that drew draft i), with pie_spec_verify_draft's launches
 * in place of pie_spec_verify_sampled's: (1) the gather and pie_decoder_prefill, raw logits on every row; (2) the edit launch when a
 * repetition penalty or a logit bias is set; (3) pie_spec_verify_draft on the processed block with the decoder's mode / temp / p / k / seed /
 * counter; (4) its last launch leaves pos = o + out_n, the device-side token and the bound token = the last token, and history, seq_ids,
 * seq_len and ids_by_pos as pie_decoder_spec_step_tail leaves them; counter = {c + out_n, 0}.  19 or 20 launches beyond the gather and
 * pie_decoder_prefill's; nothing is captured in a graph, and a decoder that never calls this entry launches exactly what it launches
 * without it.  REQUIRED: a stochastic sampler (pie_decoder_set_sampler).  PIE_E_STATE before any launch, each by name: no stochastic
 * sampler; an XTC record (its coin changes P from call to call: out of scope); a token mask; a top-logprobs record; frequency / presence
 * counts; a DRY penalty; prompt scoring; a tensor-parallel decoder; a quantized or rotating KV cache; int8 pages.  workspace:
 * pie_decoder_spec_draft_workspace_bytes(d, m + 1) bytes (0 for refused row counts), 16-byte aligned, caller-owned, ZEROED ONCE. */
size_t pie_decoder_spec_draft_workspace_bytes(const pie_decoder *d, int rows);
int pie_decoder_spec_step_draft(pie_decoder *d, const int32_t *draft_ids, int n_draft, const float *q_logprobs, int32_t *out_tokens, int32_t *out_n, float *logprobs_rows,
                                void *workspace, int32_t *seq_ids, int seq_cap, int32_t *seq_len, void *stream);
/* The step's launches by name.  pie_decoder_launch_kernel() enqueues ONE of them with exactly the arguments
 * the step uses (for per-kernel timing with events / rocprof; it does not advance the decode state, and
 * PIE_K_TAIL, which does, is refused).  pie_decoder_kernel_bytes() is that launch's algorithmic HBM traffic
 * (weights 0.5625 B/parameter + norm weights + KV rows; activations of a few KB are excluded).
 * Inside pie_decoder_step an int4 checkpoint has no PIE_K_EMBED launch: layer 0's PIE_K_QKV launch dequantises the token's row itself;
 * launched by name they remain two kernels with the same results (tests/test_gpu_decode.py::test_step_equals_its_kernels_launched_by_name). */
enum { PIE_K_EMBED = 0, PIE_K_QKV = 1, PIE_K_ATTN = 2, PIE_K_OPROJ = 3, PIE_K_GATEUP = 4, PIE_K_DOWN = 5, PIE_K_LMHEAD = 6, PIE_K_TAIL = 7 };
int pie_decoder_launch_kernel(pie_decoder *d, int which, int layer, void *stream);
size_t pie_decoder_kernel_bytes(const pie_decoder *d, int which, int T);
/* Algorithmic HBM bytes one decode step moves at context length T (SURVEY.md 8d formula). */
size_t pie_decoder_step_bytes(const pie_decoder *d, int T, int with_logits);
/* Decoder options.  PIE_OPT_KV_I8 = 1: the slabs handed to pie_decoder_step_batch / pie_decoder_prefill_batch hold int8 pages (PIE_I8 pools,
 * pie_paged_*_i8 below): new rows are quantised with their page's scales, the step's attention reads them back.  Changing an option drops the
 * captured graphs.  pie_decoder_status: synchronises the device and reports a give-up of a bounded wait of the tensor-parallel collectives in
 * *error (0 = none; sticky; that step's token is -1); bit 31: the fused q|k|v + attention launch (32 / 8 / 128 head geometry, PIE_KNOB_FUSE_ATTN) gave up
 * waiting for its kv-group (the producers of a group must get dispatched while its <= 128 attention workgroups spin: guaranteed for up to five such
 * launches in flight on a full device; the library fuses only while a process holds at most four decoders; a process that masks CUs sets
 * PIE_KNOB_FUSE_ATTN = 0).  Results after a give-up are not valid. */
enum { PIE_OPT_KV_I8 = 2 };
int pie_decoder_configure(pie_decoder *d, int option, int value);
int pie_decoder_status(pie_decoder *d, unsigned *error);

/* ---------------------------------------------------------------- tensor-parallel communicator (SURVEY.md 8 row e)
 * The reference has no multi-GPU path; BASELINE.json configs[4] (Llama-3-70B over the 8 GPUs of one node) needs
 * one.  A decode step has two all-reduces of ONE hidden vector per layer and a 3-number exchange in the tail: latency-bound, so
 * this is a one-shot push over IPC-mapped peer memory, not a ring: every rank stores its fp32 vector as 8-byte {value, epoch}
 * granules into its slot of every peer's receive area (one xGMI hop, the data is its own flag), then adds the slots of its own
 * area in rank order -- bit-identical sums on all ranks.  One process per GPU:
 *   pie_comm_create(rank, world, max_elems, &c)   allocates this rank's receive area (fine-grained device memory)
 *   pie_comm_export(c, handle64)                  64-byte hipIpcMemHandle_t of that area; the host gathers all ranks' handles
 *                                                 (torch.distributed all_gather, MPI, a file: any side channel)
 *   pie_comm_connect(c, handles)                  handles: world * 64 bytes in rank order (own entry ignored); maps the peers
 *   pie_allreduce_f32(c, data, n, stream)         in-place sum over the ranks, stream-ordered, no host synchronisation
 *   pie_decoder_set_comm(d, c)                    the decoder's steps (eager or captured in a hipGraph) use c; every rank must
 *                                                 enqueue the same sequence of steps.  c must outlive d.
 *   pie_comm_status(c, &err)                      synchronises; err != 0: a bounded wait (2 s) for a peer's data gave up
 *   pie_comm_destroy(c)
 * world == 1 is a valid (self-connected) communicator.  A peer may run at most one collective ahead of the slowest rank.
 * Inside the decoder the push half of each all-reduce rides in the row-parallel GEMV's epilogue; the launch behind it pulls, rounds and adds
 * the residual.
 * A second backend runs the same collectives through RCCL (north_star: "RCCL all-reduce over xGMI") -- ncclAllReduce / ncclAllGather on the
 * launch stream, capturable in the step's hipGraph; the comparator and fall-back of the one-shot form on a real node:
 *   pie_comm_rccl_unique_id(id128)                         on one rank; the host hands the 128 bytes to every rank
 *   pie_comm_create_rccl(rank, world, max_elems, id128, &c) collective over the world (ncclCommInitRank); the communicator is connected
 * Its sums are RCCL's (identical on every rank, summed in the ring's order, not in rank order). */
typedef struct pie_comm pie_comm;
enum { PIE_COMM_IPC = 0, PIE_COMM_RCCL = 1 };
int pie_comm_create(int rank, int world, size_t max_elems, pie_comm **out);
int pie_comm_rccl_unique_id(void *id128);
int pie_comm_create_rccl(int rank, int world, size_t max_elems, const void *id128, pie_comm **out);
int pie_comm_export(const pie_comm *c, void *handle64);
int pie_comm_connect(pie_comm *c, const void *handles);
int pie_allreduce_f32(pie_comm *c, float *data, size_t n, void *stream);
int pie_comm_status(pie_comm *c, unsigned *error);
int pie_comm_destroy(pie_comm *c);
int pie_decoder_set_comm(pie_decoder *d, pie_comm *c);

/* ---------------------------------------------------------------- KV page pool
 * Replaces pie_core's PageAllocator / KVPage: src/pie_core/include/engine/page_allocator.hpp:17-72,
 * include/engine/page.hpp:14-123, src/engine/page_allocator.cpp:8-157 (contract pinned by
 * tests/cpp/test_page_allocator.cpp, restated in tests/test_page_pool.py).  A page holds PIE_PAGE_TOKENS token slots
 * (page.hpp:14): a K block then a V block, each T [n_kv_heads, 64, head_dim] (the reference's logical shape is
 * [64, heads, head_dim], page.hpp:29-30; head-major storage keeps one head's rows of a page contiguous).  All pages live in ONE caller-owned
 * device slab of pie_page_pool_slab_bytes() bytes (page p at byte offset p * slab_bytes / num_pages); `slab` may be
 * NULL for bookkeeping only.  The free list is lock-free (tagged index stack) and LIFO, seeded so a fresh pool hands
 * out 0, 1, 2, ... (page_allocator.cpp:52-63).  Every entry point is thread-safe.
 *   create: PIE_E_ARG for num_pages == 0, n_kv_heads <= 0 or head_dim <= 0 (std::invalid_argument, page_allocator.cpp:21-29)
 *   alloc:  PIE_OK and *page_id with ref count 1 and num_tokens 0 (page_allocator.cpp:68-79), or PIE_EXHAUSTED
 *   free:   drops one reference; the page returns to the pool when the count reaches 0 (page_allocator.cpp:81-87)
 *   any id >= size: PIE_E_RANGE (std::out_of_range of check_page_id, page_allocator.cpp:110-117)
 * dtype PIE_BF16 / PIE_F16: the pages hold T rows, the layout the decoder's attention kernels consume.
 * dtype PIE_I8: the reference's own storage (page.hpp:25-32,109-117): int8 K block, int8 V block (each [n_kv_heads, 64, head_dim]), then
 * the fp16 per-head scales of K and of V ([n_kv_heads, 1] each: key_cache_scale_ / value_cache_scale_), padded to 256 bytes
 * (pie_page_i8_bytes); pie_page_scale_ptrs hands out the two scale vectors of a page.  See pie_paged_kv_append_i8 below. */
enum { PIE_PAGE_TOKENS = 64 };
typedef struct pie_page_pool pie_page_pool;
size_t pie_page_pool_slab_bytes(size_t num_pages, int n_kv_heads, int head_dim, int dtype);
int pie_page_pool_create(size_t num_pages, int n_kv_heads, int head_dim, int dtype, void *slab, pie_page_pool **out);
int pie_page_pool_destroy(pie_page_pool *pool);
size_t pie_page_pool_size(const pie_page_pool *pool);
size_t pie_page_pool_num_free(const pie_page_pool *pool);
int pie_page_alloc(pie_page_pool *pool, uint32_t *page_id);
int pie_page_free(pie_page_pool *pool, uint32_t page_id);
int pie_page_add_ref(pie_page_pool *pool, uint32_t page_id);
int pie_page_ref_count(const pie_page_pool *pool, uint32_t page_id, uint32_t *count);
int pie_page_num_tokens(const pie_page_pool *pool, uint32_t page_id, size_t *n);
int pie_page_set_num_tokens(pie_page_pool *pool, uint32_t page_id, size_t n);
int pie_page_ptrs(const pie_page_pool *pool, uint32_t page_id, void **k, void **v);
size_t pie_page_i8_bytes(int n_kv_heads, int head_dim);
int pie_page_scale_ptrs(const pie_page_pool *pool, uint32_t page_id, void **k_scale, void **v_scale);

/* Paged decode attention over a batch of sequences: what the reference's placeholder
 * Attention::invoke_paged_attention_kernel (src/pie_core/src/layers/attention.cpp:71-83) and its dummy Metal kernel
 * (src/kernels/paged_attention.metal:6-23) stand for, with the inputs BatchDetails names
 * (include/engine/batch_details.hpp:42-66): block_table int32 [B, max_blocks] = consolidated_block_table (logical block
 * j of sequence s -> page id), context_lens int32 [B] = positions each query attends INCLUDING its own (0 = idle slot,
 * output row zeroed).  q, out: T [B, n_heads, head_dim]; slab: one layer's page slab (page p at p * page bytes; inside a
 * page K then V, each T [n_kv_heads, 64, head_dim] -- head-major so one head's rows of a page are one 16 KB burst).
 * Same arithmetic contract as pie_sdpa_decode: results equal attention over the gathered contiguous rows.
 * Both tables live in device memory, so a captured graph can replay the launch while the host edits them. */
size_t pie_paged_attn_workspace_bytes(int B, int n_heads, int head_dim);
int pie_paged_attn_decode(const void *q, const void *slab, size_t n_pages, const int32_t *block_table, int max_blocks,
                          const int32_t *context_lens, int B, int n_heads, int n_kv_heads, int head_dim, float scale, int dtype,
                          void *out, void *workspace, void *stream);
/* Writes the new K / V rows (T [B, n_kv_heads, head_dim], after RoPE) of B sequences into their pages: sequence s at
 * position positions[s] (< 0 = idle slot) -> page block_table[s][positions[s] / 64], row positions[s] % 64. */
int pie_paged_kv_append(const void *k, const void *v, void *slab, size_t n_pages, const int32_t *block_table, int max_blocks,
                        const int32_t *positions, int B, int n_kv_heads, int head_dim, int dtype, void *stream);

/* int8 pages (PIE_I8 pools).  The reference declares the storage (page.hpp:25-32; "head-wise quant for now", :114) and neither a
 * quantiser nor a reader, so the arithmetic is this library's (restated in oracle/pie_oracle.py):
 *   store  q = clamp(rint(x / s), -127, 127)   x = the T element as fp32, s = the page's fp16 scale of that kv-head
 *   read   x' = fp32(q) * fp32(s), used in fp32 by the attention (softmax and P.V in fp32, one rounding of the output to T)
 * pie_page_i8_set_scales: writes the K / V scale vectors (fp16 [n_kv_heads], DEVICE; null = ones, the reference constructor's
 *   value) into the listed pages (page_ids: DEVICE int32 [n]; null = pages 0 .. n - 1).  A page's scales must not change under
 *   rows already stored in it.
 * pie_paged_kv_append_i8 / pie_paged_attn_decode_i8: as pie_paged_kv_append / pie_paged_attn_decode (k, v, q, out are T;
 *   `dtype` is T), on a slab of int8 pages.  Workspace: pie_paged_attn_workspace_bytes. */
int pie_page_i8_set_scales(void *slab, size_t n_pages, int n_kv_heads, int head_dim, const int32_t *page_ids, int n, const void *k_scales,
                           const void *v_scales, void *stream);
int pie_paged_kv_append_i8(const void *k, const void *v, void *slab, size_t n_pages, const int32_t *block_table, int max_blocks,
                           const int32_t *positions, int B, int n_kv_heads, int head_dim, int dtype, void *stream);
int pie_paged_attn_decode_i8(const void *q, const void *slab, size_t n_pages, const int32_t *block_table, int max_blocks,
                             const int32_t *context_lens, int B, int n_heads, int n_kv_heads, int head_dim, float scale, int dtype,
                             void *out, void *workspace, void *stream);

/* ---------------------------------------------------------------- batched speculation
 * One verify pass for B decode-state sequences on T pages: sequence s presents 1 + m_s rows (0 <= m_s <= 7), its fed token and its
 * drafts.  Throughout, seg_first DEVICE int32 [B + 1] cuts the pass's N rows into segments: sequence s owns rows seg_first[s] ..
 * seg_first[s + 1] - 1, 1..8 consecutive rows, none for an idle slot; every kernel clamps what it reads of it into [0, N] and to 8 rows.
 *
 * pie_paged_attn_verify: q, out T [N, n_heads, head_dim]; slab, block_tables [B, max_blocks] as pie_paged_attn_decode takes them;
 *   row_seq DEVICE int32 [N] = the block-table row of row r's sequence (read at a segment's first row, clamped to [0, B)),
 *   row_context_lens DEVICE int32 [N] = the positions row r attends INCLUDING its own (clamped to [0, 64 max_blocks]; 0: the row's output
 *   is zeros).  Row r attends positions 0 .. row_context_lens[r] - 1 of its sequence's pages -- the caller has appended the pass's own rows
 *   already -- so inside a segment, whose context lengths rise by one per row, no row sees its successors.  One launch for all segments
 *   over (n_kv_heads, splits, B) workgroups: the positions of a segment's longest row are cut into `splits` parts the way
 *   pie_paged_attn_decode cuts a sequence's, a part's K / V rows are read ONCE for all rows of the segment and all heads of the kv-group,
 *   positions at or behind the longest context are never used; fp32 online softmax, one rounding at the end.  splits > 1: one merge
 *   launch follows.  splits: 1..32, or 0 = pie_paged_attn_verify_splits(B, n_kv_heads, max_blocks), enough workgroups for two per CU
 *   and never more than max_blocks.  A row that belongs to no segment keeps an unspecified output.
 *   workspace: pie_paged_attn_verify_workspace_bytes(N, n_heads, head_dim, splits) bytes with the splits the call will use (0 for
 *   refused sizes), 16-byte aligned, no initialisation.  head_dim 64 / 128, n_heads / n_kv_heads 1..8, N and B 1..65535.  Before any
 *   launch: a NULL pointer, a dtype that is neither PIE_BF16 nor PIE_F16, splits outside 0..32: PIE_E_ARG; a bad shape: PIE_E_SHAPE;
 *   q, slab, out or workspace not 16-byte aligned, an index array not 4-byte aligned: PIE_E_ALIGN.
 * pie_ngram_draft_rows: pie_ngram_draft's rule on B sequences in one call, two launches, no atomics: ids DEVICE int32 [B, cap], len
 *   DEVICE int32 [B] (each clamped on the device to [0, cap]) -> out_ids DEVICE int32 [B, k], out_count DEVICE int32 [B]; row s is bit
 *   for bit what pie_ngram_draft returns for (ids[s], len[s]) alone.  workspace: pie_ngram_draft_rows_workspace_bytes(B) bytes, 4-byte
 *   aligned.  B 1..4096; the other bounds and codes are pie_ngram_draft's.
 * pie_spec_verify_rows: logits T [n_rows, V]; draft_ids DEVICE int32 [B, draft_stride >= 1]: sequence s's m_s drafts (m_s = its rows
 *   - 1: the segments carry the counts; a row behind the draft_stride ids the array holds has no draft and ends the run).  Row r's greedy token a_r is pie_logprobs_argmax's of that row alone (the same partials and
 *   merge: no second softmax).  Per sequence, by pie_spec_verify's rule: n_acc = the longest run draft[i] == a_i (an id outside [0, V)
 *   is never accepted and never used as an index), out_n [B] = n_acc + 1 (0 for an idle slot), out_tokens [B, 8] = a_0 .. a_n_acc, then
 *   -1.  ids / len (nullable, together): DEVICE int32 [B, cap] / [B], the drafter's input, whose ids[s, len[s] - 1] is the token the pass
 *   was fed: the accept launch writes the out_n tokens behind it and len[s] += out_n[s] (both clamped to cap), so the next
 *   pie_ngram_draft_rows can be queued behind the pass before the host reads anything.  Three launches.  workspace:
 *   pie_spec_verify_rows_workspace_bytes(n_rows) bytes, 16-byte aligned, no initialisation.  n_rows 1..65535, B 1..4096.
 * pie_decoder_spec_step_batch: one pass over the weights.  tokens DEVICE int32 [B] = every sequence's fed token; row_context_lens,
 *   row_seq [N], slabs / n_pages / slab_bytes / block_tables / max_blocks as pie_decoder_step_mixed takes them (the pages must reach
 *   every row's position).  In order: the input ids gathered on the device (an id the embedding could not index is fed as 0); the
 *   several-prompts pass's body on the N rows with RoPE + append into each sequence's pages; pie_paged_attn_verify's launches once per
 *   layer; the lm_head over all N rows into the workspace; pie_spec_verify_rows with seq_ids / seq_len / seq_cap as its ids / len / cap.
 *   N <= 256 (one tile of the streaming GEMM) and N <= 8 B.  PIE_E_STATE before any launch, each by name: int8 pages, a
 *   tensor-parallel decoder, any configured batch tail, edits, counts, DRY, XTC, automaton or top-logprobs state, prompt scoring.
 *   Nothing is captured in a graph, and a decoder that never calls this entry launches exactly what it launches without it.
 *   workspace: pie_decoder_spec_batch_workspace_bytes(d) bytes, 16-byte aligned, no initialisation. */
int pie_paged_attn_verify_splits(int B, int n_kv_heads, int max_blocks);
size_t pie_paged_attn_verify_workspace_bytes(int N, int n_heads, int head_dim, int splits);
int pie_paged_attn_verify(const void *q, const void *slab, size_t n_pages, const int32_t *block_tables, int max_blocks, const int32_t *row_seq,
                          const int32_t *row_context_lens, const int32_t *seg_first, int N, int B, int n_heads, int n_kv_heads, int head_dim, float scale,
                          int dtype, int splits, void *out, void *workspace, void *stream);
size_t pie_ngram_draft_rows_workspace_bytes(int B);
int pie_ngram_draft_rows(const int32_t *ids, const int32_t *len, int B, int cap, int ngram_max, int ngram_min, int k, int32_t *out_ids, int32_t *out_count,
                         void *workspace, void *stream);
size_t pie_spec_verify_rows_workspace_bytes(int n_rows);
int pie_spec_verify_rows(const void *logits, int n_rows, int V, int dtype, const int32_t *seg_first, int B, const int32_t *draft_ids, int draft_stride,
                         int32_t *out_tokens, int32_t *out_n, int32_t *ids, int32_t *len, int cap, void *workspace, void *stream);
size_t pie_decoder_spec_batch_workspace_bytes(const pie_decoder *d);
int pie_decoder_spec_step_batch(pie_decoder *d, const int32_t *tokens, const int32_t *draft_ids, int draft_stride, const int32_t *row_context_lens,
                                const int32_t *row_seq, const int32_t *seg_first, int N, int B, const void *const *slabs, size_t n_pages, size_t slab_bytes,
                                const int32_t *block_tables, int max_blocks, int32_t *out_tokens, int32_t *out_n, int32_t *seq_ids, int32_t *seq_len, int seq_cap,
                                void *workspace, void *stream);
/* The batched pass under per-seat tails: pie_spec_verify_sampled's rule -- a prompt-lookup draft is a point mass, so row j
 * is drawn with the draw the plain loop would use for that position and a draft is accepted while it equals the draw -- on every segment
 * of a batched pass, each under its own seat's state.  Record, ring, bias entries and XTC record s belong to segment s.
 * pie_spec_verify_rows_sampled: logits T [n_rows, V], EDITED IN PLACE; seg_first [B + 1] and draft_ids [B, draft_stride] as
 *   pie_spec_verify_rows takes them; fed DEVICE int32 [n_rows] = the rows' input ids (a segment's fed token, then its drafts, an id the
 *   embedding could not index replaced by 0: what pie_decoder_spec_step_batch gathers); pos0 DEVICE int32 [B] = the position of every
 *   segment's first row (negative: the segment's rows are not edited and its seat does not move); table DEVICE pie_row_tail [B], 8-byte
 *   aligned; recent_ids DEVICE int32 [B, 1024], the rings of pie_logits_penalty_rows; bias_ids / bias_vals [B, bias_cap] and bias_n [B]
 *   (nullable, together; 1 <= bias_cap <= 1024) as pie_logits_bias_rows takes them; xtc (nullable) DEVICE pie_xtc [B].
 *   For row r = seg_first[s] + j of segment s, at position p = pos0[s] + j, with calls_s = table[s].calls at entry:
 *   - the repetition penalty of table[s] over the ids at positions max(0, p + 1 - context_size) .. p: recent_ids[s][q & 1023] for q <
 *     pos0[s], fed[seg_first[s] + i] for q = pos0[s] + i, 0 <= i <= j (never read from the ring); then seat s's bias entries: the
 *     arithmetic and the ownership rule among duplicate ids of pie_logits_penalty / pie_logits_bias; a penalty of exactly 1.0 edits nothing;
 *   - logprobs (required) fp32 [n_rows, V]: every row gets pie_logprobs_argmax's bits of the processed row alone;
 *   - t_r = the token a one-row pie_sample (pie_sample_xtc with xtc) draws from that row with table[s]'s mode, temperature, p, k and
 *     seed and a counter of {calls_s + j, 0}; the row's argmax for a greedy or unknown mode;
 *   - n_acc_s = the largest j <= m_s with draft[s][i] == t_{first + i} for all i < j; a draft id outside [0, V) is never accepted and
 *     never used as an index; out_n [B] = n_acc_s + 1 (0 for an idle slot), out_tokens [B, 8] = those tokens, then -1.  The contract
 *     covers every row whose preceding drafts all lie inside the vocabulary; the rows behind an invalid draft are written but unspecified.
 *   Afterwards, by ONE launch behind every draw (one thread per sequence, nothing depends on arrival order): table[s].calls = calls_s +
 *   out_n[s] for a drawing mode (a greedy seat's record is not written); recent_ids[s][(pos0[s] + i) & 1023] = fed[seg_first[s] + i]
 *   for i < out_n[s] and no other slot -- no row writes the ring before that launch, so a plain pass that follows finds the ring and the
 *   stream where out_n[s] plain steps would have left them; ids / len (nullable) move as in pie_spec_verify_rows.
 *   Launches: the edit over (8, B) workgroups (1), the partials and the finish over every row (2), a fill of the rows' records with the
 *   greedy mode and one launch that expands the seats' records over their rows (2), pie_sample_rows' 5 (6 with xtc), the commit (1).
 *   The only atomics are the sampler's own.  workspace: pie_spec_verify_rows_sampled_workspace_bytes(n_rows, V) bytes (0 for refused
 *   sizes), 16-byte aligned, ZEROED ONCE by the caller (as pie_sample's) and reusable from call to call.  Each before any launch: a null
 *   pointer (the bias part, xtc, ids / len excepted), a partial bias part, a dtype that is neither PIE_BF16 nor PIE_F16: PIE_E_ARG;
 *   n_rows outside 1..65535, V outside 1..524288, B outside 1..4096, draft_stride < 1: PIE_E_SHAPE; logits not 2-byte, an index array,
 *   a part of the seats' state or an output not 4-byte, the table not 8-byte, the workspace not 16-byte aligned: PIE_E_ALIGN.
 * pie_decoder_spec_step_batch_tail: pie_decoder_spec_step_batch's arguments plus logprobs fp32 [>= N, V], and its pass up to the lm_head;
 *   behind it pie_spec_verify_rows_sampled with the batch tail's table and rings (pie_decoder_set_batch_tail: required, else PIE_E_STATE),
 *   the bias part of pie_decoder_set_batch_logits_edits and pie_decoder_set_batch_xtc's records where set, seat s = sequence s, pos0[s] =
 *   row_context_lens[seg_first[s]] - 1.  The workspace's head then holds the processed logits [N, V].  PIE_E_STATE before any launch,
 *   each by name: int8 pages, a tensor-parallel decoder, batch token automata, a mask part of the batch logits edits, a batch count
 *   penalty, a batch DRY penalty, batch top log-probabilities, prompt scoring; PIE_E_SHAPE for more sequences than a configured part's
 *   rows_cap.  pie_decoder_spec_step_batch itself still refuses every configured part.  workspace:
 *   pie_decoder_spec_batch_tail_workspace_bytes(d) bytes, 16-byte aligned, zeroed once. */
size_t pie_spec_verify_rows_sampled_workspace_bytes(int n_rows, int V);
int pie_spec_verify_rows_sampled(void *logits, int n_rows, int V, int dtype, const int32_t *seg_first, int B, const int32_t *fed, const int32_t *draft_ids,
                                 int draft_stride, const int32_t *pos0, pie_row_tail *table, int32_t *recent_ids, const int32_t *bias_ids, const float *bias_vals,
                                 const int32_t *bias_n, int bias_cap, const pie_xtc *xtc, int32_t *out_tokens, int32_t *out_n, float *logprobs, int32_t *ids,
                                 int32_t *len, int cap, void *workspace, void *stream);
size_t pie_decoder_spec_batch_tail_workspace_bytes(const pie_decoder *d);
int pie_decoder_spec_step_batch_tail(pie_decoder *d, const int32_t *tokens, const int32_t *draft_ids, int draft_stride, const int32_t *row_context_lens,
                                     const int32_t *row_seq, const int32_t *seg_first, int N, int B, const void *const *slabs, size_t n_pages, size_t slab_bytes,
                                     const int32_t *block_tables, int max_blocks, int32_t *out_tokens, int32_t *out_n, float *logprobs, int32_t *seq_ids,
                                     int32_t *seq_len, int seq_cap, void *workspace, void *stream);

/* ---------------------------------------------------------------- quantized KV cache (QuantizedKVCache, cache/kv_cache/quantized.py)
 * The reference's format: every cached row stored as mx.quantize output -- codes uint32 [n_kv_heads, capacity, head_dim*bits/32],
 * scales / biases T [n_kv_heads, capacity, head_dim/group_size] (B = 1).  bits 4 / 8, group_size 32 / 64 / 128 dividing head_dim,
 * head_dim 64 / 128, T bf16 / f16; anything else is PIE_E_ARG / PIE_E_SHAPE before a launch.
 * pie_kv_quantize: rows [0, n) of every head of x T [H, src_cap, head_dim] -> the same rows of codes / scales / biases [H, dst_cap, ...];
 *   bit-identical with mx.quantize (cache/kv_cache/cache.py:144-147, quantized.py:91-96).
 * pie_attn_decode_quant: quantized_scaled_dot_product_attention (models/base.py:56-89) for one query row: q, out T [n_heads, head_dim],
 *   the first T positions of the cache attended; queries *= scale and the scores rounded to T as there, softmax and the value
 *   product in fp32, one rounding of the output.  workspace: pie_sdpa_decode_workspace_bytes(n_heads, head_dim) bytes.
 * pie_decoder_set_kv_quant: the quantized alternative to pie_decoder_set_kv -- HOST arrays [n_layers] of the layers' six device buffers.
 *   Steps append the new K / V rows quantized (the attention launch quantizes the row its q|k|v launch staged) and attend the cache
 *   as pie_attn_decode_quant does.  Prompts (pie_decoder_prefill / _prefill_embeds) take the batched pass over a T scratch of one layer's
 *   K / V, dequantized from the codes, with the chunk's rows quantized into the cache before its attention.  Refused (PIE_E_STATE) on
 *   tensor-parallel decoders. */
int pie_kv_quantize(const void *x, int H, int n, int src_cap, int head_dim, int group_size, int bits, int dtype, void *codes, void *scales,
                    void *biases, int dst_cap, void *stream);
int pie_attn_decode_quant(const void *q, const void *k_codes, const void *k_scales, const void *k_biases, const void *v_codes,
                          const void *v_scales, const void *v_biases, int n_heads, int n_kv_heads, int T, int cap, int head_dim,
                          int group_size, int bits, float scale, int dtype, void *out, void *workspace, void *stream);
int pie_decoder_set_kv_quant(pie_decoder *d, const void *const *k_codes, const void *const *k_scales, const void *const *k_biases,
                             const void *const *v_codes, const void *const *v_scales, const void *const *v_biases, int capacity,
                             int group_size, int bits, void *stream);

/* ---------------------------------------------------------------- rotating KV cache (RotatingKVCache, cache/kv_cache/rotating.py)
 * A ring of `window` rows over the contiguous buffers of pie_decoder_set_kv, in the reference's row order: rows [0, keep) are the first
 * positions (never evicted), the rest rotate.  Position p >= rot0 lives in row keep + (p - rot0) % (window - keep), earlier positions in row p.
 * pie_decoder_set_kv_ring: binds the ring to the decoder's buffers (call after pie_decoder_set_kv; window 0 = unbounded again).  Steps
 *   (graph replay included) write the new K / V rows to their ring row and attend min(offset + 1, window) rows -- the q|k|v launch stages
 *   the rows, the attention launch moves them.  Prompts of 2+ rows (pie_decoder_prefill / _prefill_embeds) append at buffer rows
 *   row0 .. row0 + L - 1 with RoPE at the absolute positions offset .. offset + L - 1, and row r attends rows row0 + r - window .. row0 + r.
 *   `positions`: the steps' positions stay below it (the staging page's table covers them).  Refused (PIE_E_STATE) on tensor-parallel
 *   decoders and on paged or quantized caches.
 * pie_kv_ring_order: rows keep + j <- rows keep + (j + shift) % n, j < n_dst, of every head of k and v (T [H, cap, head_dim]), through
 *   `scratch` (2 * H * n_dst * head_dim elements of T): a full ring into temporal order, or a long store cut to the window.
 * pie_sdpa_prefill_window: pie_sdpa_prefill where row r also ignores keys below offset + r - window (create_causal_mask(L, offset,
 *   window_size=window), models/base.py:18-34); key blocks below a query tile's window are skipped.
 * pie_sdpa_decode_ring: the decoder's step attention on a ring, op level: the new rows wait in `stage` ([2, Hkv, 64, D] T, row pos % 64),
 *   are moved into ring row slot(pos) of k / v [Hkv, cap, D] and min(pos + 1, window) rows are attended -> out [Hq, D].  workspace:
 *   pie_sdpa_decode_workspace_bytes(Hq, D) + 32 bytes. */
int pie_decoder_set_kv_ring(pie_decoder *d, int window, int keep, int rot0, int row0, int positions, void *stream);
int pie_kv_ring_order(void *k, void *v, int H, int cap, int head_dim, int keep, int n, int shift, int n_dst, void *scratch, void *stream);
int pie_sdpa_prefill_window(const void *q, const void *k, const void *v, int Hq, int Hkv, int L, int offset, int cap, int D, int window,
                            float scale, int dtype, void *out, void *stream);
int pie_sdpa_decode_ring(const void *q, void *k, void *v, const void *stage, int Hq, int Hkv, int cap, int D, int pos, int window, int keep,
                         int rot0, float scale, int dtype, void *out, void *workspace, void *stream);

/* ---------------------------------------------------------------- vision tower ops
 * Call sites: models/intern/vision.py (Qwen2.5-VL vision tower: PatchEmbed :87-121, Attention :143-186, MLP :189-197,
 * PatchMerger :124-140).  RMSNorm, SiLU * up and the residual adds are pie_rms_norm / pie_silu_mul / pie_add.
 * pie_linear_w16m: nn.Linear on M rows -- y [M, N] = x [M, K] . w [N, K]^T (+ bias [N]), T in, fp32 accumulate, T out (rounded
 *   before the bias is added, like the text tower's Linear) on the hand-written 16-bit MFMA GEMM (csrc/w16_gemm.hpp; rounds 1-4
 *   called hipBLASLt here).  The weight is given as W16M tiles -- 32 output rows x 64 columns in MFMA operand order, zero-padded --
 *   built once per matrix: pie_w16m_bytes(N, K) bytes (256-byte aligned), filled by pie_repack_w16m from the row-major [N, K] weight.
 *   x: M rows of ldx elements (0 = packed) holding 64 * ceil(K / 64) used columns, ZEROS past K (the tower's two odd widths, 1176
 *   and 3420, are padded by the host); y: rows of ldy elements (0 = packed).  swiglu != 0: the weight's rows interleave (gate_i, up_i),
 *   bias likewise, and y [M, N / 2] = T(T(silu(g)) * u) with g, u the rounded, biased Linear outputs (MLP, vision.py:196-197: the values
 *   of the GEMM followed by pie_bias_silu_mul).  workspace: pie_linear_w16m_workspace(M, N, K) bytes of device scratch for the
 *   shapes that split K (few rows, narrow matrices; 0 for most and for swiglu).  Any N (16-byte stores when N and ldy are multiples
 *   of 8); swiglu needs N % 8 == 0.
 * pie_gelu: nn.GELU() exact form, fp32 inside, one rounding.
 * pie_vision_qkv_rope: qkv T [N, 3, H, D] (+ optional bias T [3 * H * D], the qkv Linear's) -> q T [N, H, DP], k, v T [H, N, DP] with rotate-half rotary on q and k
 *   (apply_rotary_pos_emb_vision, vision.py:55-70; cos / sin fp32 [N, D/2] = the row's angles) and head dims D..DP-1 zeroed
 *   (DP = 64 or 128, the attention kernel's head sizes).
 * pie_sdpa_segments: block-diagonal non-causal attention, the mask of vision.py:160-167: query row r attends keys
 *   [seg_lo[r], seg_hi[r]) (device int32 [N], non-decreasing, lo <= r < hi).  q, out T [N, H, D]; k, v T [H, N, D]. */
size_t pie_w16m_bytes(int N, int K);
int pie_repack_w16m(const void *w, int N, int K, int dtype, void *w16m, void *stream);
size_t pie_linear_w16m_workspace(int M, int N, int K);
int pie_linear_w16m(const void *x, int ldx, const void *w16m, const void *bias, int M, int N, int K, int dtype, void *y, int ldy, int swiglu,
                    void *workspace, size_t workspace_bytes, void *stream);
int pie_gelu(const void *x, size_t n, int dtype, void *y, void *stream);
int pie_vision_qkv_rope(const void *qkv, const void *bias, const float *cos_t, const float *sin_t, int N, int H, int D, int DP, int dtype,
                        void *q, void *k, void *v, void *stream);
/* Bias adds folded into the op that consumes the GEMM output (same values as pie_linear_w16m with a bias followed by the op):
 * pie_bias_silu_mul: y = silu(gate + bias_gate) * (up + bias_up), T [M, N] (MLP, vision.py:196-197); gate / up rows are `ld`
 *   elements apart (0 = N), so both may be column halves of one [M, 2N] GEMM output;
 * pie_add_bias: y = x + (r + bias), T [M, N] (the residual adds of vision.py:212-218). */
int pie_bias_silu_mul(const void *gate, const void *up, const void *bias_gate, const void *bias_up, int M, int N, int ld, int dtype, void *y,
                      void *stream);
/* pie_add_bias_rms_norm: the residual add and the RMSNorm after it in one pass: y = x + (r + bias), xn = rms_norm(y, norm_w, eps);
 * T [M, N], N % 8 == 0 (the values pie_add_bias followed by pie_rms_norm produce). */
int pie_add_bias_rms_norm(const void *x, const void *r, const void *bias, const void *norm_w, float eps, int M, int N, int dtype, void *y, void *xn,
                          void *stream);
int pie_add_bias(const void *x, const void *r, const void *bias, int M, int N, int dtype, void *y, void *stream);
int pie_sdpa_segments(const void *q, const void *k, const void *v, const int32_t *seg_lo, const int32_t *seg_hi, int N, int H, int D,
                      float scale, int dtype, void *out, void *stream);

/* ---------------------------------------------------------------- few-row int4 GEMM (prompts of 2..32 tokens)
 * mx.quantized_matmul in its many-row regime (weights dequantised to T, T x T products, fp32 accumulation;
 * models/llama/language.py:83,108,127) without a 16-bit copy of the weights: W4M tiles (32 output rows x 64 columns, 1152 B,
 * built on the device from the W4S stream of pie_repack_w4g64) are dequantised in registers into MFMA operand fragments.
 * N % 32 == 0, K % 64 == 0, 1 <= M <= 32.  x T [M, K], y T [M, N] (rows in the packed order of the W4S matrix). */
size_t pie_w4m_bytes(int N, int K);
int pie_repack_w4s_to_w4m(const void *w4s, int N, int K, void *w4m, void *stream);
int pie_qgemm_w4m(const void *x, const void *w4m, int M, int N, int K, int dtype, void *y, void *stream);


#ifdef __cplusplus
}
#endif
#endif /* PIE_HIP_H */
