// decoder.hip -- native decode-step runtime: the fused launch sequence of one Model.__call__
// (models/llama/language.py:199-210) for inputs[1,1] + the tail of _inference
// (engine/inference_engine.py:252-271), replayable as a hipGraph because position, token and the KV
// buffer addresses are read from device memory.
//
// Launches per step: embed | per layer { rmsnorm+qkv+rope+append, split-KV attention, [combine: caches beyond 1024
// positions only], merge+o_proj+residual, rmsnorm+gate/up+swiglu, down+residual } | rmsnorm+lm_head(+wave stats) | finish.
// (The embedding rides in layer 0's q|k|v launch for int4 models; for the 32 / 8 / 128 head geometry the attention rides in every q|k|v launch,
// behind an XCD-local seam: attn_form() below.)
#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "attention.hpp"
#include "tail.hpp"
#include "w4_gemv.hpp"
#include "decoder.hpp"

namespace {
thread_local std::string g_last_error;
#if defined(PIE_GEMV_PROF) && PIE_GEMV_PROF == 3
constexpr int PROF_QKV = 256, PROF_O = 288, PROF_GU = 320, PROF_DOWN = 352;  // 32 words each: the fine prologue stamps sit at +8..13
#else
constexpr int PROF_QKV = 16, PROF_O = 20, PROF_GU = 24, PROF_DOWN = 28;
#endif
}
namespace {
int g_knobs[PIE_KNOB_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
static_assert(PIE_KNOB_COUNT == 13, "one PIE_KNOB_DEFAULT per knob");
}
int pie_knob(int knob) { return knob >= 0 && knob < PIE_KNOB_COUNT ? g_knobs[knob] : PIE_KNOB_DEFAULT; }
namespace pie {
void set_error(const std::string &msg) { g_last_error = msg; }
int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}
}  // namespace pie

__global__ void k_advance(DecState *s) { s->pos += 1; }
__global__ void k_set_state(DecState *s, int pos, int token, int cap) {
    if (pos >= 0) s->pos = pos;
    if (token >= 0) s->token = token;
    if (cap >= 0) s->cap = cap;
}
__global__ void k_set_ring(DecState *s, DecState *rows, int window, int keep, int rot0, int row0) {
    s->window = window, s->keep = keep, s->rot0 = rot0;
    if (rows) rows->pos = row0, rows->cap = s->cap, rows->window = window, rows->keep = keep, rows->rot0 = rot0;
}

// Picks the split count / merge path for the current cache capacity; returns true when the launch sequence changed.
static bool plan_attention(pie_decoder *d) {
    const pie_decoder_config &c = d->cfg;
    int splits;
    // a ring attends at most its window, whatever the buffers hold after a long prompt
    const int cap = d->ring && d->ring_w < d->kv_cap ? d->ring_w : d->kv_cap;
    if (c.kv_splits > 0) splits = c.kv_splits > ATTN_MAX_SPLITS ? ATTN_MAX_SPLITS : c.kv_splits;
    else if (cap <= d->merge_max_cap) splits = GEMV_ATTN_SPLITS;
    else {
        splits = cap / 64;  // >= 64 positions per workgroup, 16 per wave
        const int fill = 256 / c.n_kv_heads > 0 ? 256 / c.n_kv_heads : 1;
        if (splits > fill) splits = fill;
        if (splits > ATTN_MAX_SPLITS) splits = ATTN_MAX_SPLITS;
        if (splits < GEMV_ATTN_SPLITS) splits = GEMV_ATTN_SPLITS;
    }
    const bool combine = splits > GEMV_ATTN_SPLITS;
    const bool changed = splits != d->splits || combine != d->combine;
    d->splits = splits, d->combine = combine;
    return changed;
}

static int dev_alloc(void **p, size_t bytes) {
    PIE_HIP_TRY(hipMalloc(p, bytes));
    PIE_HIP_TRY(hipMemset(*p, 0, bytes));
    return PIE_OK;
}

static void drop_graphs(pie_decoder *d) {
    for (int i = 0; i < 2; ++i)
        if (d->graph[i]) {
            (void)hipGraphExecDestroy(d->graph[i]);
            d->graph[i] = nullptr;
            d->graph_kernels[i] = -1;
        }
}

// The attention launch's idle CUs warm at most this much of o_proj's stream: 9.4 MB (the 8B int4 matrix, all of it) is what the launch's ~5 us
// can carry; uncapped, the 33.5 MB of the dense 8B o_proj stretched the launch itself: dense 2.81 -> 3.00 ms per step, int8 (17.8 MB) 1.74 -> 1.81
// (cap 10: 2.81 / 1.75; off: 2.81 / 1.74; int4: 1.186-1.191 with, 1.190 without)
constexpr int ATTN_WARM_DEFAULT_MB = 10;
// Workgroups with equal blockIdx.x % 8 share an XCD (tools/pilot_probe, every grid size and history): what the fused q|k|v + attention launch
// relies on, so it is checked once per process on the real dispatcher (a partitioned device with one XCD passes trivially).
__global__ void k_xcc_probe(unsigned *out) {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    if (threadIdx.x == 0) out[blockIdx.x] = xcc;
}
static bool xcd_classes_hold() {
    static int cached = -1;  // (one device per process)
    if (cached >= 0) return cached == 1;
    unsigned *dev = nullptr, host[256];
    bool ok = hipMalloc((void **)&dev, sizeof(host)) == hipSuccess;
    for (int rep = 0; rep < 3 && ok; ++rep) {
        hipLaunchKernelGGL(k_xcc_probe, dim3(256), dim3(512), 0, 0, dev);
        ok = hipMemcpy(host, dev, sizeof(host), hipMemcpyDeviceToHost) == hipSuccess;
        for (int b = 0; b < 256 && ok; ++b) ok = host[b] == host[b & 7];
    }
    if (dev) (void)hipFree(dev);
    (void)hipGetLastError();
    cached = ok ? 1 : 0;
    return ok;
}

// The step's attention inside the q|k|v launch (w4_gemv.hpp, FUSE): the 32 / 8 / 128 head geometry (kv-group = XCD class), any weight format,
// the short-cache plan on a contiguous or T-page cache (not int8 pages), one GPU.  Knob PIE_KNOB_FUSE_ATTN = 0 keeps the two launches (bit-identical; the tests' cross-check).
// The fused launch's attention workgroups spin until their kv-group has arrived.  They are the last-dispatched half of the grid, the other half leaves
// after arriving, so a launch holds at most 128 workgroup slots while it waits and the chip has 768 for this kernel: up to five such launches in flight
// cannot starve each other's producers.  A process that holds more than four live decoders gets the two-launch form (captured graphs follow at their next step).
static std::atomic<int> g_live_decoders{0};
// Knob PIE_KNOB_ATTN_MERGE_IN_LAUNCH = 0 leaves the fused launch's partials to o_proj's merging prologue (bit-identical; the tests' cross-check and the A/B).
// This reads process-global state (knobs, the live-decoder count), so it is asked ONCE per q|k|v launch: enqueue_kernel records the answer in
// d->attn_form and the ATTN / OPROJ launches follow the record.
static int attn_form(const pie_decoder *d) {
    const pie_decoder_config &c = d->cfg;
    if (pie_knob(PIE_KNOB_FUSE_ATTN) == 0 || !d->xcd_ok || !d->seam || g_live_decoders.load() > 4) return ATTN_TWO_LAUNCHES;
    const bool fits = !d->tp() && !d->combine && !(d->kv_i8 && d->block_table) && !d->kv_quant && !d->ring && c.n_heads == 32 && c.n_kv_heads == 8 && c.head_dim == 128 && c.hidden <= 4096 &&
                      d->splits >= 1 && d->splits <= 4;  // (any weight format of the q|k|v matrix)
    if (!fits) return ATTN_TWO_LAUNCHES;
    return pie_knob(PIE_KNOB_ATTN_MERGE_IN_LAUNCH) == 0 ? ATTN_FUSED : ATTN_FUSED_MERGED;
}

// What the step's attention launch is given (contiguous or T-page cache, not the int8 pages)
static AttnArgs attn_args(pie_decoder *d, int li) {
    const pie_decoder_config &c = d->cfg;
    const int H = c.hidden, D = c.head_dim, QD = c.n_heads * D;
    const pie_layer_weights &w = d->layers[li];
    AttnArgs a = {};
    a.q = d->qbuf, a.kv_table = d->kv_table, a.layer = li, a.n_layers = c.n_layers, a.state = d->state;
    a.Hq = c.n_heads, a.Hkv = c.n_kv_heads, a.splits = d->splits, a.scale = 1.0f / sqrtf((float)D);
    a.part_acc = d->part_acc, a.part_ml = d->part_ml, a.out = d->attn;
    a.block_table = d->block_table, a.n_pages = d->n_pages, a.bt_stride = 0;
    a.nt_kv = d->combine;  // long-context plan (capacity > 1024): the cache no longer survives in the Infinity Cache between steps
    a.prof = d->pf_sink;
    // the CUs this launch leaves idle warm the Infinity Cache with o_proj's weights (attention.hpp: +1.3 % on the step)
    if (!d->combine) {
        a.pf_rows = (256 - c.n_kv_heads * d->splits) / c.n_kv_heads;
        if (a.pf_rows < 0) a.pf_rows = 0;
        a.pf_ptr = (const char *)w.wo, a.pf_sink = d->pf_sink;
        a.pf_bytes = packed_bytes(d->mat_fmt(w.wo), H, QD);
        const int cap_mb = pie_knob(PIE_KNOB_ATTN_WARM_MAX_MB) >= 0 ? pie_knob(PIE_KNOB_ATTN_WARM_MAX_MB) : ATTN_WARM_DEFAULT_MB;
        if (a.pf_bytes > (unsigned long long)cap_mb << 20) a.pf_bytes = (unsigned long long)cap_mb << 20;
        if (!a.pf_bytes) a.pf_rows = 0;
    }
    return a;
}

// The configured tail over the bound outputs (include/pie_hip.h), in batch_tail_launch's six stages (prefill.hip): edit -- penalty and / or
// bias, one launch | count penalty -- frequency / presence, one launch | DRY, one launch | fresh partials, which apply the token mask on their way | finish |
// the sampler's launches and the top-n log-probabilities' two.
// from_state: the row's input token is the device-side state's (a step): recorded in ids_by_pos before the penalty reads its window.
static int configured_tail(pie_decoder *d, bool from_state, hipStream_t st) {
    const pie_decoder_config &c = d->cfg;
    const StepTail &t = d->tail;
    const LogitStat *stats = d->stats;
    int n_stats = d->n_stats, rc;
    // token automaton: its mask words come first, from the state as the previous step's advance left it
    if (t.dfa.on() && (rc = token_dfa_mask_launch(t.dfa.record, t.dfa.state, t.dfa.tables, t.dfa.tables_len, 1, c.vocab, t.dfa.mask, t.dfa.mask_words, nullptr, st))) return rc;
    if (t.penalty.on() || t.bias.on()) {  // edit
        PenArgs a = {};
        a.logits = d->logits, a.V = c.vocab, a.penalty = (float)t.penalty.value, a.ids_by_pos = t.penalty.ids_by_pos, a.ids_cap = t.penalty.ids_cap, a.context = t.penalty.context;
        a.state = d->state, a.record = from_state;
        const BiasArgs b = {t.bias.ids, t.bias.vals, t.bias.n, t.penalty.on()};
        if ((rc = t.bias.on() ? logits_edit_launch(c.dtype, a, b, st) : logits_penalty_launch(c.dtype, a, st))) return rc;
    }
    if (t.counts.on()) {  // count penalty: behind the penalty and the bias; a prompt pass counts nothing
        CountPenArgs k = {};
        k.logits = d->logits, k.V = c.vocab, k.records = t.counts.record, k.counts = t.counts.counts, k.state = d->state, k.count = from_state;
        if ((rc = logits_count_penalty_rows_launch(c.dtype, k, 1, st))) return rc;
    }
    if (t.dry.on()) {  // DRY: behind the count penalty; a step records its input token before it reads its window
        DryArgs k = {};
        k.w.logits = d->logits, k.w.V = c.vocab, k.w.ids_by_pos = t.dry.ids_by_pos, k.w.ids_cap = t.dry.ids_cap, k.w.state = d->state, k.w.record = from_state;
        k.record = t.dry.record, k.breakers = t.dry.breakers;
        if ((rc = logits_dry_launch(c.dtype, k, st))) return rc;
    }
    if (t.edits_logits()) {  // partials: the lm_head epilogue's are stale
        if ((rc = logits_stats_launch(c.dtype, d->logits, c.vocab, t.tail_stats, st, t.dfa.on() ? t.dfa.mask : t.mask.words))) return rc;
        stats = t.tail_stats, n_stats = TAIL_STAT_TILES;
    }
    // finish
    if ((rc = logits_tail_launch(c.dtype, d->logits, c.vocab, stats, n_stats, d->logprobs, d->token_out, d->state, d->history, d->hist_cap, st))) return rc;
    if (t.sampler.on()) {  // sampler and top-n
        const StepTail::Sampler &s = t.sampler;
        const SampleFeed feed = {&d->state->token, &d->state->pos, d->history, d->hist_cap};
        if ((rc = sample_launch(d->logprobs, 1, c.vocab, s.mode, s.temp, s.p, s.k, s.seed, s.counter, s.ws, d->token_out, nullptr, nullptr, feed, st, SampleXtc{t.xtc.record, nullptr})))
            return rc;
    }
    // after the draw: slot 0 is the token that is fed back
    if (t.top.on() && (rc = top_logprobs_launch(d->logprobs, 1, c.vocab, t.top.n, d->token_out, nullptr, t.top.ids, t.top.vals, t.top.ws, st))) return rc;
    if (!t.dfa.on()) return PIE_OK;
    // last: the automaton's state moves by the token that is fed back
    return token_dfa_advance_launch(t.dfa.record, t.dfa.state, t.dfa.tables, t.dfa.tables_len, 1, c.vocab, d->token_out, st);
}

// One launch of the step's sequence (PIE_K_* of include/pie_hip.h); `li` is the layer for per-layer kernels.
int enqueue_kernel(pie_decoder *d, int which, int li, const int *token_ptr, u16 *logits_dst, hipStream_t st, bool embed_here) {
    const pie_decoder_config &c = d->cfg;
    const int H = c.hidden, D = c.head_dim, QD = c.n_heads * D, KVD = c.n_kv_heads * D;
    const pie_layer_weights &w = d->layers[li];
    const int efmt = d->mat_fmt(d->glob.embed_codes);
    const bool dense_embed = efmt == PIE_W_DENSE;
    switch (which) {
        case PIE_K_EMBED:  // h = embed_tokens(inputs)  (language.py:176)
            if (dense_embed) return pie_embedding_dense(token_ptr, 1, d->glob.embed_codes, d->embed_vocab(), H, c.dtype, d->h, st);
            return embedding_launch(token_ptr, 1, d->glob.embed_codes, d->glob.embed_scales, d->glob.embed_biases, d->embed_vocab(), H, c.dtype, d->h,
                                    d->glob.rope_freqs, d->state, d->rope_cs, D / 2, st, efmt);
        case PIE_K_QKV: {  // q,k,v = proj(input_layernorm(x)); rope(offset=cache.offset); cache.update_and_fetch  (language.py:83-95)
            GemvArgs a = {};
            a.fmt = d->mat_fmt(w.wqkv), a.w = (const char *)w.wqkv, a.K = H, a.N = QD + 2 * KVD;
            a.x = d->h, a.norm_w = (const u16 *)w.attn_norm, a.eps = c.rms_eps;
            a.freqs = d->glob.rope_freqs, a.rope_cs = dense_embed || d->row_is_h ? nullptr : d->rope_cs /* filled by the quantised embedding kernel */, a.state = d->state, a.q_out = d->qbuf, a.kv_table = d->kv_table;
            a.layer = li, a.n_layers = c.n_layers, a.n_heads = c.n_heads, a.n_kv_heads = c.n_kv_heads, a.head_dim = D;
            a.lin_bias = (const u16 *)w.bqkv, a.rope_traditional = c.rope_traditional;
            a.block_table = d->block_table, a.n_pages = d->n_pages;
            const bool i8 = d->kv_i8 && d->block_table;  // int8 pages: the T rows go to the staging page, then get quantised into the sequence's page
            if (i8 || d->kv_quant || d->ring) a.kv_table = d->kv_table_stage, a.block_table = d->zero_table, a.n_pages = 1;
            a.prof = reinterpret_cast<unsigned long long *>(d->pf_sink) + PROF_QKV;
            if (embed_here) {  // the step's embedding launch folded into this one (embed_in_qkv): x = the token's row, dequantised by every workgroup
                a.x = nullptr, a.rope_cs = nullptr, a.rope_cs_out = d->rope_cs, a.h_out = d->h, a.token = token_ptr;
                a.emb_codes = (const u32 *)d->glob.embed_codes, a.emb_scales = (const u16 *)d->glob.embed_scales, a.emb_biases = (const u16 *)d->glob.embed_biases;
                a.emb_vocab = d->embed_vocab();
            }
            d->attn_form = attn_form(d);  // the one decision of this layer's attention; PIE_K_ATTN and PIE_K_OPROJ follow it
            if (d->attn_form != ATTN_TWO_LAUNCHES) a.fuse = 1, a.attn = attn_args(d, li), a.seam = d->seam, a.merge = d->attn_form == ATTN_FUSED_MERGED;  // the step's attention behind an XCD-local seam of this launch
            const int rc = w4s_gemv_launch(c.dtype, embed_here ? PRO_EMBED : PRO_RMSNORM, EPI_ROPE_KV, a, 1, st);
            if (rc || !i8) return rc;
            const size_t blk = (size_t)c.n_kv_heads * PIE_PAGE_TOKENS * D;
            return paged_kv_append_i8_staged_launch(c.dtype, d->kv_stage, d->kv_stage + blk, const_cast<void *>(d->slab_host[li]), d->n_pages, d->block_table, d->max_blocks,
                                                    &d->state->pos, c.n_kv_heads, D, st);
        }
        case PIE_K_ATTN: {  // scaled_dot_product_attention over keys[..., :offset+1, :]  (language.py:98-105, base.py:111-113)
            if (d->kv_i8 && d->block_table) {  // int8 pages: the batch paths' kernel with one sequence whose length comes from the device-side state
                AttnArgs a = {};
                a.q = d->qbuf, a.slab = (const u16 *)d->slab_host[li], a.block_table = d->block_table, a.state = d->state, a.bt_stride = 0, a.n_pages = d->n_pages;
                a.rows = 1, a.Hq = c.n_heads, a.Hkv = c.n_kv_heads, a.scale = 1.0f / sqrtf((float)D);
                int splits = d->kv_cap / 128;  // 4-wave workgroups, >= 128 positions each
                a.splits = splits < 1 ? 1 : (splits > ATTN_MAX_SPLITS ? ATTN_MAX_SPLITS : splits);
                a.part_acc = d->part_acc, a.part_ml = d->part_ml, a.out = d->attn;
                return paged_attn_i8_launch(c.dtype, D, a, st);  // merges its splits itself (k_attn_combine): o_proj reads d->attn
            }
            if (d->kv_quant) {  // quantized KV: the launch first quantises the staged rows into the cache, then scores the codes
                const void *const *p = &d->kvq_host[(size_t)6 * li];
                QAttnArgs a = {};
                a.q = d->qbuf, a.kc = (const u32 *)p[0], a.ks = (const u16 *)p[1], a.kb = (const u16 *)p[2];
                a.vc = (const u32 *)p[3], a.vs = (const u16 *)p[4], a.vb = (const u16 *)p[5];
                a.state = d->state, a.gs = d->kvq_gs, a.Hq = c.n_heads, a.Hkv = c.n_kv_heads, a.splits = d->splits, a.scale = 1.0f / sqrtf((float)D);
                a.part_acc = d->part_acc, a.part_ml = d->part_ml, a.stage = d->kv_stage;
                return attn_decode_quant_launch(c.dtype, D, d->kvq_bits, a, d->combine, d->attn, st);  // short caches: merged by the o_proj prologue
            }
            if (d->attn_form != ATTN_TWO_LAUNCHES) return PIE_OK;  // ran behind the q|k|v launch's seam
            AttnArgs a = attn_args(d, li);
            if (d->ring) a.ring_stage = d->kv_stage;  // rotating cache: the staged rows go to their ring slot inside this launch
            return attn_decode_launch(c.dtype, D, a, d->combine, st);  // short caches: partials are merged by the o_proj prologue
        }
        case PIE_K_OPROJ: {  // h = x + o_proj(attn)  (language.py:108,151)
            GemvArgs a = {};
            a.fmt = d->mat_fmt(w.wo), a.w = (const char *)w.wo, a.K = QD, a.N = H, a.resid = d->h, a.lin_bias = (const u16 *)w.bo;
            // tensor-parallel shard (row-parallel Linear over the local heads): un-rounded fp32 partial, summed over the ranks,
            // THEN the Linear's one rounding and the residual add
            // the one-shot communicator: the push half of the all-reduce rides in this epilogue (EPI_TP_PUSH); RCCL: fp32 partial in memory
            const bool push = d->tp() && tp_comm_push_args(d->comm, &a.tp_peers, &a.tp_epoch, &a.tp_stride);
            const int epi = d->tp() ? (push ? EPI_TP_PUSH : EPI_PARTIAL_F32) : EPI_RESIDUAL;
            a.y32 = d->tp_part, a.tp_rank = c.tp_rank, a.tp_world = c.tp_world;
            const bool merged_attn = d->combine || (d->kv_i8 && d->block_table) || d->attn_form == ATTN_FUSED_MERGED;  // the attention output is already one T vector
            if (merged_attn) a.x = d->attn;
            else a.part_acc = d->part_acc, a.part_ml = d->part_ml, a.splits = d->splits, a.state = d->state, a.head_dim = D;
            a.prof = reinterpret_cast<unsigned long long *>(d->pf_sink) + PROF_O;
            const int rc = w4s_gemv_launch(c.dtype, merged_attn ? PRO_NONE : PRO_ATTN, epi, a, 1, st);
            return rc || !d->tp() ? rc : tp_allreduce_launch(d->comm, c.dtype, d->tp_part, H, d->h, st, push);
        }
        case PIE_K_GATEUP: {  // silu(gate(post_attention_layernorm(h))) * up(...)  (language.py:127,152)
            GemvArgs a = {};
            a.fmt = d->mat_fmt(w.wgateup), a.w = (const char *)w.wgateup, a.K = H, a.N = 2 * c.inter, a.x = d->h, a.norm_w = (const u16 *)w.mlp_norm, a.eps = c.rms_eps;
            a.y = d->act, a.lin_bias = (const u16 *)w.bgateup;
            a.prof = reinterpret_cast<unsigned long long *>(d->pf_sink) + PROF_GU;
            return w4s_gemv_launch(c.dtype, PRO_RMSNORM, EPI_SWIGLU, a, 1, st);
        }
        case PIE_K_DOWN: {  // out = h + down_proj(...)  (language.py:127,153)
            GemvArgs a = {};
            a.fmt = d->mat_fmt(w.wdown), a.w = (const char *)w.wdown, a.K = c.inter, a.N = H, a.x = d->act, a.resid = d->h, a.lin_bias = (const u16 *)w.bdown;
            const bool push = d->tp() && tp_comm_push_args(d->comm, &a.tp_peers, &a.tp_epoch, &a.tp_stride);
            a.y32 = d->tp_part, a.tp_rank = c.tp_rank, a.tp_world = c.tp_world;
            a.prof = reinterpret_cast<unsigned long long *>(d->pf_sink) + PROF_DOWN;
            const int rc = w4s_gemv_launch(c.dtype, PRO_NONE, d->tp() ? (push ? EPI_TP_PUSH : EPI_PARTIAL_F32) : EPI_RESIDUAL, a, 1, st);
            return rc || !d->tp() ? rc : tp_allreduce_launch(d->comm, c.dtype, d->tp_part, H, d->h, st, push);
        }
        case PIE_K_LMHEAD: {  // lm_head(norm(h)) (language.py:187,206-209) with per-tile log-softmax partials
            GemvArgs a = {};
            a.fmt = d->mat_fmt(d->glob.lm_head), a.w = (const char *)d->glob.lm_head, a.K = H, a.N = c.vocab, a.x = d->h, a.norm_w = (const u16 *)d->glob.final_norm, a.eps = c.rms_eps;
            a.y = logits_dst, a.stats = d->stats;
            return w4s_gemv_launch(c.dtype, PRO_RMSNORM, EPI_LOGITS, a, 1, st);
        }
        case PIE_K_TAIL:  // log-softmax + greedy argmax, advances the device-side state (inference_engine.py:268-271)
            if (d->tp())  // vocabulary-parallel: (max, sum exp, argmax) of every shard -> global log-sum-exp and token
                return tp_tail_launch(d->comm, c.dtype, logits_dst, c.vocab, c.tp_rank * c.vocab, d->stats, d->n_stats, d->tp_part + H, d->logprobs, d->token_out,
                                      d->state, d->history, d->hist_cap, st);
            if (d->tail.configured() && logits_dst == d->logits && !d->tail_raw) return configured_tail(d, token_ptr == &d->state->token && !d->row_is_h, st);
            return logits_tail_launch(c.dtype, logits_dst, c.vocab, d->stats, d->n_stats, d->logprobs, d->token_out, d->state, d->history, d->hist_cap, st);
        default: return pie::fail(PIE_E_ARG, "pie_decoder: unknown kernel id");
    }
}

// The launch sequence of one step.  token_ptr: device int32 holding the input token id.
static int enqueue_step(pie_decoder *d, const int *token_ptr, bool with_logits, u16 *logits_dst, hipStream_t st) {
    // An int4 embedding table in front of an int4 q|k|v matrix: no embedding launch, layer 0's q|k|v launch dequantises the row itself
    // (4.4 us of kernel + a launch boundary per step; same bits: the same dequantisation, RMSNorm tree and RoPE table).
    const bool embed_in_qkv = !d->row_is_h && d->mat_fmt(d->glob.embed_codes) == PIE_W_INT4_G64 && d->mat_fmt(d->layers[0].wqkv) == PIE_W_INT4_G64 && !d->tp() && d->cfg.hidden <= 8 * 8 * GEMV_WAVES * 64;
    int rc = embed_in_qkv || d->row_is_h ? PIE_OK : enqueue_kernel(d, PIE_K_EMBED, 0, token_ptr, logits_dst, st);
    if (rc) return rc;
    for (int li = 0; li < d->cfg.n_layers; ++li)
        for (int k : {PIE_K_QKV, PIE_K_ATTN, PIE_K_OPROJ, PIE_K_GATEUP, PIE_K_DOWN})
            if ((rc = enqueue_kernel(d, k, li, token_ptr, logits_dst, st, embed_in_qkv && li == 0 && k == PIE_K_QKV))) return rc;
    if (!with_logits) {
        hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, st, d->state);
        PIE_LAUNCH_CHECK();
        return PIE_OK;
    }
    if ((rc = enqueue_kernel(d, PIE_K_LMHEAD, 0, token_ptr, logits_dst, st))) return rc;
    return enqueue_kernel(d, PIE_K_TAIL, 0, token_ptr, logits_dst, st);
}

int graph_kernel_nodes(hipGraph_t g) {
    size_t n_nodes = 0;
    if (hipGraphGetNodes(g, nullptr, &n_nodes) != hipSuccess || !n_nodes) return -1;
    std::vector<hipGraphNode_t> nodes(n_nodes);
    if (hipGraphGetNodes(g, nodes.data(), &n_nodes) != hipSuccess) return -1;
    int k = 0;
    for (size_t i = 0; i < n_nodes; ++i) {
        hipGraphNodeType t;
        if (hipGraphNodeGetType(nodes[i], &t) == hipSuccess && t == hipGraphNodeTypeKernel) ++k;
    }
    return k;
}

int capture_graph(const std::function<int(hipStream_t)> &enqueue, int *enqueue_rc, hipGraph_t *graph, hipError_t *end_err) {
    *enqueue_rc = PIE_OK, *graph = nullptr, *end_err = hipSuccess;
    hipStream_t cs = nullptr;
    PIE_HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    const hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(cs);
        return pie::fail(PIE_E_HIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(e));
    }
    *enqueue_rc = enqueue(cs);
    *end_err = hipStreamEndCapture(cs, graph);
    (void)hipStreamDestroy(cs);
    return PIE_OK;
}

extern "C" {

const char *pie_hello(void) { return "pie_core \xe2\x9c\x93"; }
#ifndef PIE_BUILD_HASH
#define PIE_BUILD_HASH "unhashed"
#endif
const char *pie_version(void) { return "pie_hip 0.3.0 (gfx950) " PIE_BUILD_HASH; }  // the hash of the sources: proxy_inference_engine_amd/build.py
const char *pie_last_error(void) { return g_last_error.c_str(); }

int pie_set_knob(int knob, int value) {
    PIE_REQUIRE(knob >= 0 && knob < PIE_KNOB_COUNT, PIE_E_ARG, "pie_set_knob: unknown knob");
    g_knobs[knob] = value < 0 ? PIE_KNOB_DEFAULT : value;
    return PIE_OK;
}
int pie_get_knob(int knob) { return pie_knob(knob); }

int pie_device_info(char *name, int name_len, int *n_cus, size_t *hbm_bytes) {
    int dev = 0;
    PIE_HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t p;
    PIE_HIP_TRY(hipGetDeviceProperties(&p, dev));
    if (name && name_len > 0) {
        strncpy(name, p.gcnArchName, (size_t)name_len - 1);
        name[name_len - 1] = 0;
    }
    if (n_cus) *n_cus = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = p.totalGlobalMem;
    return PIE_OK;
}

int pie_decoder_create(const pie_decoder_config *cfg, pie_decoder **out) {
    PIE_REQUIRE(cfg && out, PIE_E_ARG, "pie_decoder_create: null pointer");
    const pie_decoder_config &c = *cfg;
    PIE_REQUIRE(c.dtype == PIE_BF16 || c.dtype == PIE_F16, PIE_E_ARG, "pie_decoder_create: dtype must be PIE_BF16 or PIE_F16");
    PIE_REQUIRE(c.hidden > 0 && c.hidden % 64 == 0 && c.inter > 0 && c.inter % 64 == 0, PIE_E_SHAPE,
                "pie_decoder_create: hidden and intermediate sizes must be multiples of 64 (int4 group size)");
    PIE_REQUIRE(c.head_dim == 64 || c.head_dim == 128, PIE_E_SHAPE, "pie_decoder_create: head_dim must be 64 or 128");
    PIE_REQUIRE(c.n_layers > 0 && c.n_heads > 0 && c.n_kv_heads > 0 && c.n_heads % c.n_kv_heads == 0, PIE_E_SHAPE, "pie_decoder_create: bad head counts");
    PIE_REQUIRE(c.vocab > 0 && c.vocab % 2 == 0, PIE_E_SHAPE, "pie_decoder_create: vocab must be even");
    PIE_REQUIRE(c.hidden <= 32768 && c.inter <= 32768 && c.n_heads * c.head_dim <= 32768, PIE_E_SHAPE, "pie_decoder_create: K > 32768 not supported");
    PIE_REQUIRE(fmt_valid(c.weight_format), PIE_E_ARG, "pie_decoder_create: unknown weight_format");
    PIE_REQUIRE(c.tp_world >= 0 && c.tp_world <= 8 && c.tp_rank >= 0 && c.tp_rank < (c.tp_world > 0 ? c.tp_world : 1), PIE_E_ARG,
                "pie_decoder_create: 0 <= tp_rank < tp_world <= 8");
    pie_decoder *d = new (std::nothrow) pie_decoder();
    PIE_REQUIRE(d, PIE_E_HIP, "pie_decoder_create: out of host memory");
    d->cfg = c;
    d->layers.resize(c.n_layers);
    d->layer_set.assign(c.n_layers, 0);
    if (pie_knob(PIE_KNOB_ATTN_MERGE_MAX_CAP) >= 0) d->merge_max_cap = pie_knob(PIE_KNOB_ATTN_MERGE_MAX_CAP);  // capacity up to which o_proj merges the splits
    int rc = PIE_OK;
    d->n_stats = w4s_gemv_waves(c.vocab, c.hidden);
    const int QD = c.n_heads * c.head_dim;
#define PIE_ALLOC(ptr, bytes) if ((rc = dev_alloc((void **)&(ptr), (bytes)))) { pie_decoder_destroy(d); return rc; }
    PIE_ALLOC(d->state, sizeof(DecState));
    PIE_ALLOC(d->kv_table, sizeof(unsigned long long) * 2 * c.n_layers);
    PIE_ALLOC(d->qbuf, 2 * (size_t)QD);
    PIE_ALLOC(d->attn, 2 * (size_t)QD);
    PIE_ALLOC(d->act, 2 * (size_t)c.inter);
    PIE_ALLOC(d->part_acc, 4 * (size_t)c.n_heads * ATTN_MAX_SPLITS * c.head_dim);
    PIE_ALLOC(d->part_ml, 4 * (size_t)c.n_heads * ATTN_MAX_SPLITS * 2);
    PIE_ALLOC(d->stats, sizeof(LogitStat) * (size_t)d->n_stats);
    PIE_ALLOC(d->rope_cs, sizeof(float) * (size_t)c.head_dim);
    PIE_ALLOC(d->pf_sink, 8192);  // the developer builds' stamps (-DPIE_ATTN_PROF: words 2..9; -DPIE_GEMV_PROF: 16 + 4 kind ..)
    PIE_ALLOC(d->seam, sizeof(unsigned) * GEMV_SEAM_WORDS);  // 8 XCD counters 128 bytes apart, [256] the give-up flag, then 32 per-head counters 128 bytes apart (w4_gemv.hpp)
    d->xcd_ok = xcd_classes_hold();
    ++g_live_decoders, d->counted_live = true;
    if (d->tp()) PIE_ALLOC(d->tp_part, sizeof(float) * ((size_t)c.hidden + 4));  // RCCL backend: the fp32 partial; [hidden]: the step's log-sum-exp
#undef PIE_ALLOC
    plan_attention(d);
    *out = d;
    return PIE_OK;
}

int pie_decoder_destroy(pie_decoder *d) {
    if (!d) return PIE_OK;
    if (d->counted_live) --g_live_decoders, d->counted_live = false;  // (a create that failed before it was counted never was)
    drop_graphs(d);
    prefill_free(d);
    void *ptrs[] = {d->state, d->kv_table, d->qbuf, d->attn, d->act, d->part_acc, d->part_ml, d->stats, d->rope_cs, d->pf_sink, d->seam, d->tp_part, d->kv_stage, d->kv_table_stage,
                    d->zero_table, d->kvq_scratch, d->kvq_table, d->ring_rows, d->tail.tail_stats};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete d;
    return PIE_OK;
}

int pie_decoder_set_layer(pie_decoder *d, int layer, const pie_layer_weights *w) {
    PIE_REQUIRE(d && w, PIE_E_ARG, "pie_decoder_set_layer: null pointer");
    PIE_REQUIRE(layer >= 0 && layer < d->cfg.n_layers, PIE_E_ARG, "pie_decoder_set_layer: layer out of range");
    PIE_REQUIRE(w->attn_norm && w->mlp_norm && w->wqkv && w->wo && w->wgateup && w->wdown, PIE_E_ARG, "pie_decoder_set_layer: null weight");
    PIE_REQUIRE(pie_aligned(w->wqkv, 256) && pie_aligned(w->wo, 256) && pie_aligned(w->wgateup, 256) && pie_aligned(w->wdown, 256) &&
                    pie_aligned(w->attn_norm, 16) && pie_aligned(w->mlp_norm, 16),
                PIE_E_ALIGN, "pie_decoder_set_layer: W4S buffers need 256-byte, norm weights 16-byte alignment");
    PIE_REQUIRE(!d->tp() || (!w->bo && !w->bdown), PIE_E_ARG,
                "pie_decoder_set_layer: o_proj / down_proj biases are not supported on a tensor-parallel shard (they would be added once per rank)");
    {
        const int f[4] = {w->fmt_qkv, w->fmt_o, w->fmt_gateup, w->fmt_down};
        const void *m[4] = {w->wqkv, w->wo, w->wgateup, w->wdown};
        for (int i = 0; i < 4; ++i) {
            PIE_REQUIRE(f[i] == 0 || fmt_valid(f[i] - 1), PIE_E_ARG, "pie_decoder_set_layer: unknown per-matrix weight format");
            if (f[i]) d->fmt_map[m[i]] = f[i] - 1;
            else d->fmt_map.erase(m[i]);
        }
    }
    d->layers[layer] = *w;
    d->layer_set[layer] = 1;
    prefill_free(d);  // resident T copies of the previous weights are stale
    drop_graphs(d);
    return PIE_OK;
}

int pie_decoder_set_globals(pie_decoder *d, const pie_global_weights *w) {
    PIE_REQUIRE(d && w, PIE_E_ARG, "pie_decoder_set_globals: null pointer");
    PIE_REQUIRE(w->embed_codes && w->final_norm && w->lm_head && w->rope_freqs, PIE_E_ARG, "pie_decoder_set_globals: null weight");
    PIE_REQUIRE((w->fmt_embed == 0 || fmt_may_embed(w->fmt_embed - 1)) && (w->fmt_lm_head == 0 || fmt_valid(w->fmt_lm_head - 1)), PIE_E_ARG,
                "pie_decoder_set_globals: unknown per-matrix weight format");
    const int efmt = w->fmt_embed ? w->fmt_embed - 1 : d->cfg.weight_format;
    PIE_REQUIRE(efmt == PIE_W_DENSE || (w->embed_scales && w->embed_biases), PIE_E_ARG, "pie_decoder_set_globals: a quantised embedding needs scales and biases");
    PIE_REQUIRE(fmt_may_embed(efmt), PIE_E_ARG,
                "pie_decoder_set_globals: the embedding table of a 2- / 6-bit checkpoint is handed over as 4- / 8-bit codes (fmt_embed = PIE_W_INT4_G64 + 1 / PIE_W_INT8_G64 + 1); W2S and W6S are Linear formats");
    if (w->fmt_embed) d->fmt_map[w->embed_codes] = w->fmt_embed - 1;
    else d->fmt_map.erase(w->embed_codes);
    if (w->fmt_lm_head) d->fmt_map[w->lm_head] = w->fmt_lm_head - 1;
    else if (w->lm_head != w->embed_codes) d->fmt_map.erase(w->lm_head);
    PIE_REQUIRE(pie_aligned(w->lm_head, 256) && pie_aligned(w->final_norm, 16) && pie_aligned(w->embed_codes, 16), PIE_E_ALIGN,
                "pie_decoder_set_globals: misaligned weight");
    d->glob = *w;
    d->glob_set = true;
    drop_graphs(d);
    return PIE_OK;
}

// Any binding other than pie_decoder_set_kv_ring makes the cache unbounded again (window 0 in the device-side state); true if it was a ring.
static bool leave_ring(pie_decoder *d, hipStream_t st) {
    if (!d->ring) return false;
    hipLaunchKernelGGL(k_set_ring, dim3(1), dim3(1), 0, st, d->state, (DecState *)nullptr, 0, 0, 0, 0);
    d->ring = false, d->ring_w = 0;
    return true;
}

int pie_decoder_set_kv(pie_decoder *d, const void *const *k_ptrs, const void *const *v_ptrs, int capacity, void *stream) {
    PIE_REQUIRE(d && k_ptrs && v_ptrs, PIE_E_ARG, "pie_decoder_set_kv: null pointer");
    PIE_REQUIRE(capacity > 0, PIE_E_SHAPE, "pie_decoder_set_kv: capacity must be positive");
    const int L = d->cfg.n_layers;
    std::vector<unsigned long long> tab(2 * (size_t)L);
    for (int i = 0; i < L; ++i) {
        PIE_REQUIRE(k_ptrs[i] && v_ptrs[i] && pie_aligned(k_ptrs[i], 16) && pie_aligned(v_ptrs[i], 16), PIE_E_ALIGN,
                    "pie_decoder_set_kv: null or misaligned cache buffer");
        tab[i] = (unsigned long long)(uintptr_t)k_ptrs[i];
        tab[L + i] = (unsigned long long)(uintptr_t)v_ptrs[i];
    }
    hipStream_t st = (hipStream_t)stream;
    // pageable source: the copy is staged before the call returns, so `tab` may go out of scope
    PIE_HIP_TRY(hipMemcpyAsync(d->kv_table, tab.data(), tab.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(1), 0, st, d->state, -1, -1, capacity);
    PIE_LAUNCH_CHECK();
    d->kv_set = true;
    d->kv_cap = capacity;
    const bool was_paged = d->block_table != nullptr, was_quant = d->kv_quant, was_ring = leave_ring(d, st);
    d->block_table = nullptr, d->n_pages = 0, d->kv_quant = false;
    if (plan_attention(d) || was_paged || was_quant || was_ring) drop_graphs(d);  // the launch sequence changed: captured graphs are stale
    return PIE_OK;
}

// The staging page of the q|k|v epilogue (int8 pages, quantized KV): K block then V block [n_kv_heads, 64, head_dim] T, the table that points
// every layer at it, and a block table of `blocks` zeros (position p -> page 0, row p % 64).
static int ensure_staging(pie_decoder *d, int blocks) {
    const int L = d->cfg.n_layers;
    const size_t v_off = (size_t)d->cfg.n_kv_heads * PIE_PAGE_TOKENS * d->cfg.head_dim * 2;
    if (!d->kv_stage) {
        PIE_HIP_TRY(hipMalloc((void **)&d->kv_stage, 2 * v_off));
        PIE_HIP_TRY(hipMemset(d->kv_stage, 0, 2 * v_off));
        PIE_HIP_TRY(hipMalloc((void **)&d->kv_table_stage, sizeof(unsigned long long) * 2 * L));
        std::vector<unsigned long long> stab(2 * (size_t)L);
        for (int i = 0; i < L; ++i) stab[i] = (unsigned long long)(uintptr_t)d->kv_stage, stab[L + i] = stab[i] + v_off;
        PIE_HIP_TRY(hipMemcpy(d->kv_table_stage, stab.data(), stab.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    }
    if (d->zero_blocks < blocks) {
        if (d->zero_table) (void)hipFree(d->zero_table);
        d->zero_table = nullptr, d->zero_blocks = 0;
        PIE_HIP_TRY(hipMalloc((void **)&d->zero_table, sizeof(int) * (size_t)blocks));
        PIE_HIP_TRY(hipMemset(d->zero_table, 0, sizeof(int) * (size_t)blocks));
        d->zero_blocks = blocks;
        drop_graphs(d);  // the table's address is a launch argument
    }
    return PIE_OK;
}

int pie_decoder_set_kv_ring(pie_decoder *d, int window, int keep, int rot0, int row0, int positions, void *stream) {
    PIE_REQUIRE(d, PIE_E_ARG, "pie_decoder_set_kv_ring: null decoder");
    PIE_REQUIRE(!d->tp(), PIE_E_STATE, "pie_decoder_set_kv_ring: a rotating KV cache is not available on a tensor-parallel decoder");
    PIE_REQUIRE(d->kv_set && !d->block_table && !d->kv_quant, PIE_E_STATE, "pie_decoder_set_kv_ring: bind the ring's buffers with pie_decoder_set_kv first");
    hipStream_t st = (hipStream_t)stream;
    if (window == 0) {
        if (leave_ring(d, st)) {
            PIE_LAUNCH_CHECK();
            plan_attention(d);
            drop_graphs(d);
        }
        return PIE_OK;
    }
    PIE_REQUIRE(window >= 1 && keep >= 0 && keep < window, PIE_E_ARG, "pie_decoder_set_kv_ring: need 0 <= keep < window");
    // (the buffers grow with the ring until it is full: a step's row and length stay below the rows the host has allocated)
    PIE_REQUIRE(row0 >= 0 && row0 <= d->kv_cap && rot0 >= 0 && positions >= 1, PIE_E_SHAPE, "pie_decoder_set_kv_ring: the prompt row base lies outside the buffers");
    if (!d->ring_rows) {
        PIE_HIP_TRY(hipMalloc((void **)&d->ring_rows, sizeof(DecState)));
        PIE_HIP_TRY(hipMemset(d->ring_rows, 0, sizeof(DecState)));
    }
    // the staging page's block table is indexed by the position: it must cover every position a step (graph replay included) writes
    const int rc = ensure_staging(d, (positions + PIE_PAGE_TOKENS - 1) / PIE_PAGE_TOKENS);
    if (rc) return rc;
    hipLaunchKernelGGL(k_set_ring, dim3(1), dim3(1), 0, st, d->state, d->ring_rows, window, keep, rot0, row0);
    PIE_LAUNCH_CHECK();
    const bool changed = !d->ring || d->ring_w != window;  // (keep, rot0, row0 are device-side values, not launch arguments)
    d->ring = true, d->ring_w = window, d->ring_row0 = row0;
    if (plan_attention(d) || changed) drop_graphs(d);
    return PIE_OK;
}

int pie_decoder_set_kv_quant(pie_decoder *d, const void *const *k_codes, const void *const *k_scales, const void *const *k_biases,
                             const void *const *v_codes, const void *const *v_scales, const void *const *v_biases, int capacity, int group_size,
                             int bits, void *stream) {
    PIE_REQUIRE(d && k_codes && k_scales && k_biases && v_codes && v_scales && v_biases, PIE_E_ARG, "pie_decoder_set_kv_quant: null pointer");
    PIE_REQUIRE(!d->tp(), PIE_E_STATE, "pie_decoder_set_kv_quant: a quantized KV cache is not available on a tensor-parallel decoder");
    if (int rc = kv_quant_check("pie_decoder_set_kv_quant", d->cfg.dtype, d->cfg.head_dim, group_size, bits)) return rc;
    const int rep = d->cfg.n_heads / d->cfg.n_kv_heads;
    PIE_REQUIRE(rep == 1 || rep == 2 || rep == 4 || rep == 8, PIE_E_SHAPE, "pie_decoder_set_kv_quant: n_heads / n_kv_heads must be 1, 2, 4 or 8");
    PIE_REQUIRE(capacity > 0 && capacity <= (1 << 30), PIE_E_SHAPE, "pie_decoder_set_kv_quant: capacity must be positive");
    const int L = d->cfg.n_layers;
    std::vector<const void *> host((size_t)6 * L);
    for (int i = 0; i < L; ++i) {
        const void *p[6] = {k_codes[i], k_scales[i], k_biases[i], v_codes[i], v_scales[i], v_biases[i]};
        for (int j = 0; j < 6; ++j) {
            PIE_REQUIRE(p[j] && pie_aligned(p[j], j % 3 == 0 ? 8 : 2), PIE_E_ALIGN, "pie_decoder_set_kv_quant: null or misaligned cache buffer");
            host[(size_t)6 * i + j] = p[j];
        }
    }
    int rc = ensure_staging(d, (capacity + PIE_PAGE_TOKENS - 1) / PIE_PAGE_TOKENS);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(1), 0, st, d->state, -1, -1, capacity);
    PIE_LAUNCH_CHECK();
    // the buffers, group and width are arguments of the attention launches: a captured graph is stale when any of them changes
    const bool changed = leave_ring(d, st) || !d->kv_quant || d->kvq_host != host || d->kvq_gs != group_size || d->kvq_bits != bits || d->block_table != nullptr;
    d->kvq_host = std::move(host), d->kvq_gs = group_size, d->kvq_bits = bits, d->kv_quant = true;
    d->block_table = nullptr, d->n_pages = 0;
    d->kv_set = true;
    d->kv_cap = capacity;
    if (plan_attention(d) || changed) drop_graphs(d);
    return PIE_OK;
}

int pie_decoder_set_paged_kv(pie_decoder *d, const void *const *slabs, size_t n_pages, const int32_t *block_table, int max_blocks,
                             void *stream) {
    PIE_REQUIRE(d && slabs && block_table, PIE_E_ARG, "pie_decoder_set_paged_kv: null pointer");
    PIE_REQUIRE(n_pages > 0 && n_pages < 0x7FFFFFFFu && max_blocks > 0 && max_blocks <= (1 << 24), PIE_E_SHAPE,
                "pie_decoder_set_paged_kv: n_pages and max_blocks must be positive");
    const int L = d->cfg.n_layers;
    const size_t v_off = (size_t)d->cfg.n_kv_heads * PIE_PAGE_TOKENS * d->cfg.head_dim * 2;  // bytes: K block, then V block
    std::vector<unsigned long long> tab(2 * (size_t)L);
    // int8 pages: the single-sequence step passes the slab bases as launch arguments (baked into a captured graph), so new slabs under an
    // unchanged table, pool size and width must drop the graphs too (T pages are reached through the device-side kv_table)
    bool slabs_changed = (int)d->slab_host.size() != L;
    for (int i = 0; i < L; ++i) {
        PIE_REQUIRE(slabs[i] && pie_aligned(slabs[i], 16), PIE_E_ALIGN, "pie_decoder_set_paged_kv: null or misaligned slab");
        tab[i] = (unsigned long long)(uintptr_t)slabs[i];
        tab[L + i] = tab[i] + v_off;
        slabs_changed = slabs_changed || d->slab_host[i] != slabs[i];
    }
    d->slab_host.assign(slabs, slabs + L);
    hipStream_t st = (hipStream_t)stream;
    if (d->kv_i8) {  // int8 pages (PIE_OPT_KV_I8): the staging page, the table that points every layer at it, and a block table of zeros
        const int rc = ensure_staging(d, max_blocks);
        if (rc) return rc;
    }
    const bool blocks_changed = d->max_blocks != max_blocks;
    d->max_blocks = max_blocks;
    const int capacity = max_blocks * PIE_PAGE_TOKENS;
    PIE_HIP_TRY(hipMemcpyAsync(d->kv_table, tab.data(), tab.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(1), 0, st, d->state, -1, -1, capacity);
    PIE_LAUNCH_CHECK();
    d->kv_set = true;
    d->kv_cap = capacity;
    // kernel arguments are baked into captured graphs: a new table pointer or pool size invalidates them
    const bool changed = leave_ring(d, st) | (d->block_table != block_table || d->n_pages != (int)n_pages || blocks_changed || (d->kv_i8 && slabs_changed) || d->kv_quant);
    d->block_table = block_table, d->n_pages = (int)n_pages, d->kv_quant = false;
    if (plan_attention(d) || changed) drop_graphs(d);
    return PIE_OK;
}

int pie_decoder_set_state(pie_decoder *d, int offset, int token, void *stream) {
    PIE_REQUIRE(d, PIE_E_ARG, "pie_decoder_set_state: null decoder");
    PIE_REQUIRE(offset >= 0, PIE_E_ARG, "pie_decoder_set_state: negative offset");
    PIE_REQUIRE(token < d->embed_vocab(), PIE_E_ARG, "pie_decoder_set_state: token id out of range");
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(1), 0, (hipStream_t)stream, d->state, offset, token, -1);
    PIE_LAUNCH_CHECK();
    return PIE_OK;
}

static int ready(pie_decoder *d) {
    PIE_REQUIRE(d, PIE_E_ARG, "pie_decoder: null decoder");
    PIE_REQUIRE(d->glob_set && d->kv_set && d->out_set, PIE_E_STATE, "pie_decoder: set_globals, set_kv and bind_outputs must be called before stepping");
    for (char s : d->layer_set) PIE_REQUIRE(s, PIE_E_STATE, "pie_decoder: a layer has no weights (pie_decoder_set_layer)");
    PIE_REQUIRE(!d->tp() || d->comm, PIE_E_STATE, "pie_decoder: a tensor-parallel shard needs a communicator (pie_decoder_set_comm)");
    return PIE_OK;
}

int pie_decoder_step(pie_decoder *d, int flags, void *stream) {
    int rc = ready(d);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool with_logits = (flags & PIE_STEP_LOGITS) != 0;
    if (!(flags & PIE_STEP_GRAPH)) return enqueue_step(d, &d->state->token, with_logits, d->logits, st);
    const int gi = with_logits ? 1 : 0;
    if (d->graph[gi] && d->graph_form[gi] > attn_form(d)) drop_graphs(d);  // the captured form was withdrawn (a knob, more than four live decoders): capture what is allowed now
    if (!d->graph[gi]) {
        // captured on a private stream, launched on the caller's
        hipGraph_t g = nullptr;
        hipError_t e = hipSuccess;
        int erc = PIE_OK;
        if ((rc = capture_graph([&](hipStream_t cs) { return enqueue_step(d, &d->state->token, with_logits, d->logits, cs); }, &erc, &g, &e)))
            return rc;
        if (erc) {
            if (g) (void)hipGraphDestroy(g);
            return erc;
        }
        if (e != hipSuccess) return pie::fail(PIE_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        d->graph_form[gi] = d->attn_form;  // what the capture's q|k|v launches decided, not a second look at the knobs
        d->graph_kernels[gi] = graph_kernel_nodes(g);  // what the graph really holds, for the benchmark's launches_per_step (not a formula)
        e = hipGraphInstantiate(&d->graph[gi], g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) return pie::fail(PIE_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    }
    PIE_HIP_TRY(hipGraphLaunch(d->graph[gi], st));
    return PIE_OK;
}

int pie_decoder_graph_launches(const pie_decoder *d, int flags) {
    if (!d) return -1;
    const int gi = (flags & PIE_STEP_LOGITS) ? 1 : 0;
    return d->graph[gi] ? d->graph_kernels[gi] : -1;
}

}  // extern "C"
namespace {
struct RawTail {  // pie_decoder::tail_raw for the duration of one prompt pass
    pie_decoder *d;
    RawTail(pie_decoder *dec, bool raw) : d(dec) { d->tail_raw = raw; }
    ~RawTail() { d->tail_raw = false; }
};

// Row l of a prompt that runs as decode steps.  Scored (pie_decoder_set_prompt_logprobs): every row computes its logits, as with logits on
// every position, and the op runs on that one row; a row before the last ends in the raw tail, so a configured sampler draws nothing for it.
int enqueue_scored_step(pie_decoder *d, const int *token_ptr, int l, bool last, bool every_logits, u16 *dst, hipStream_t st) {
    if (!d->prompt.n) return enqueue_step(d, token_ptr, last || every_logits, dst, st);
    const bool raw = d->tail_raw;
    d->tail_raw = raw || !last;
    int rc = enqueue_step(d, token_ptr, true, dst, st);
    d->tail_raw = raw;
    return rc ? rc : d->prompt.score_rows(d->cfg, dst, l, 1, st);
}

// What every setter of a tail begins with -- the nine of the step's and the eight of the multi-sequence passes'
static int tail_entry(const pie_decoder *d, const char *entry) {
    PIE_REQUIRE(d, PIE_E_ARG, std::string(entry) + ": null decoder");
    PIE_REQUIRE(!d->tp(), PIE_E_STATE, std::string(entry) + ": the tail of a tensor-parallel decoder is vocabulary-parallel and not configurable");
    return PIE_OK;
}

// One part of the step's tail (decoder.hpp: StepTail), assigned as a whole: every field is a launch argument, so the captured graphs go exactly
// when the part compares unequal; once some part edits the logits the fresh partials need their scratch (without it the part stays as it was).
template <class Part>
static int set_part(pie_decoder *d, Part &slot, const Part &v) {
    const Part old = slot;
    slot = v;
    if (d->tail.edits_logits() && !d->tail.tail_stats)
        if (int rc = dev_alloc((void **)&d->tail.tail_stats, sizeof(LogitStat) * TAIL_STAT_TILES)) return slot = old, rc;
    if (!(old == v)) drop_graphs(d);
    return PIE_OK;
}
}  // namespace
extern "C" {

int pie_decoder_prefill(pie_decoder *d, const int32_t *ids, int L, void *logits_all, void *stream) {
    int rc = ready(d);
    if (rc) return rc;
    PIE_REQUIRE(ids && L > 0, PIE_E_ARG, "pie_decoder_prefill: need at least one token");
    hipStream_t st = (hipStream_t)stream;
    PIE_REQUIRE(!d->prompt.n || L <= d->prompt.rows_cap, PIE_E_SHAPE, "pie_decoder_prefill: more rows than the prompt log-probabilities' rows_cap");
    const RawTail raw(d, logits_all != nullptr);  // logits on every position: raw, whatever tail is configured
    // a tensor-parallel shard feeds its prompt through the step kernels (2 all-reduces per layer and token); the many-row GEMM
    // path has no collective yet
    // int8 pages: the batched prompt path of ONE sequence reads and writes T pages; such prompts run as decode steps here (fresh prompts go
    // through pie_decoder_prefill_batch, which the Python host does)
    // a rotating cache takes every multi-row update through the windowed pass: a chunk is not a run of single-row updates there
    // (rotating.py: the chunk sees the retained window plus itself, a step only the newest rows)
    if ((L >= prefill_min_rows() || (d->ring && L >= 2)) && !d->tp() && !(d->kv_i8 && d->block_table)) return prefill_batched(d, ids, nullptr, L, logits_all, st);  // MLX's qmm regime
    for (int l = 0; l < L; ++l) {
        const bool last = l == L - 1;
        u16 *dst = logits_all ? (u16 *)logits_all + (size_t)l * d->cfg.vocab : d->logits;
        if ((rc = enqueue_scored_step(d, ids + l, l, last, logits_all != nullptr, dst, st))) return rc;
    }
    if (logits_all)  // keep pie_decoder_outputs()'s logits pointer meaningful: last row
        PIE_HIP_TRY(hipMemcpyAsync(d->logits, (u16 *)logits_all + (size_t)(L - 1) * d->cfg.vocab, 2 * (size_t)d->cfg.vocab,
                                   hipMemcpyDeviceToDevice, st));
    return PIE_OK;
}

int pie_decoder_prefill_embeds(pie_decoder *d, const void *embeds, int L, void *logits_all, void *stream) {
    int rc = ready(d);
    if (rc) return rc;
    PIE_REQUIRE(embeds && L > 0, PIE_E_ARG, "pie_decoder_prefill_embeds: need at least one row");
    PIE_REQUIRE(pie_aligned(embeds, 16), PIE_E_ALIGN, "pie_decoder_prefill_embeds: 16-byte alignment required");
    PIE_REQUIRE(!d->tp(), PIE_E_STATE, "pie_decoder_prefill_embeds: not available on a tensor-parallel shard");
    hipStream_t st = (hipStream_t)stream;
    PIE_REQUIRE(!d->prompt.n || L <= d->prompt.rows_cap, PIE_E_SHAPE, "pie_decoder_prefill_embeds: more rows than the prompt log-probabilities' rows_cap");
    const RawTail raw(d, logits_all != nullptr);
    // (one row on a rotating cache is a single-row update: the decode step below, as in rotating.py)
    if (!(d->kv_i8 && d->block_table) && !(d->ring && L == 1)) return prefill_batched(d, nullptr, embeds, L, logits_all, st);
    // int8 pages: the batched prompt path of one sequence reads and writes T pages, so -- like a prompt of tokens (pie_decoder_prefill) -- the rows
    // run as decode steps, each with its row copied into the residual stream instead of an embedding launch (no RoPE table either: the
    // q|k|v epilogue computes its own angles).  The greedy token the tail leaves in the device-side state is that of the last row.
    const size_t row_bytes = 2 * (size_t)d->cfg.hidden;
    d->row_is_h = true;
    for (int l = 0; l < L && !rc; ++l) {
        u16 *dst = logits_all ? (u16 *)logits_all + (size_t)l * d->cfg.vocab : d->logits;
        if (hipMemcpyAsync(d->h, (const char *)embeds + (size_t)l * row_bytes, row_bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = pie::fail(PIE_E_HIP, "pie_decoder_prefill_embeds: copying a row failed");
        else rc = enqueue_scored_step(d, &d->state->token, l, l == L - 1, logits_all != nullptr, dst, st);
    }
    d->row_is_h = false;
    if (rc) return rc;
    if (logits_all)
        PIE_HIP_TRY(hipMemcpyAsync(d->logits, (u16 *)logits_all + (size_t)(L - 1) * d->cfg.vocab, 2 * (size_t)d->cfg.vocab, hipMemcpyDeviceToDevice, st));
    return PIE_OK;
}

int pie_decoder_bind_outputs(pie_decoder *d, void *logits, float *logprobs, int32_t *token, void *hidden, int32_t *history,
                             int history_len) {
    PIE_REQUIRE(d && logits && logprobs && token && hidden, PIE_E_ARG, "pie_decoder_bind_outputs: null pointer");
    PIE_REQUIRE(pie_aligned(logits, 16) && pie_aligned(hidden, 16) && pie_aligned(logprobs, 4) && pie_aligned(token, 4), PIE_E_ALIGN,
                "pie_decoder_bind_outputs: logits/hidden need 16-byte alignment");
    PIE_REQUIRE(history_len >= 0 && (history || history_len == 0), PIE_E_ARG, "pie_decoder_bind_outputs: bad history buffer");
    d->logits = (u16 *)logits, d->logprobs = logprobs, d->token_out = token, d->h = (u16 *)hidden;
    d->history = history, d->hist_cap = history_len;
    d->out_set = true;
    drop_graphs(d);
    return PIE_OK;
}

int pie_decoder_set_token_from(pie_decoder *d, const int32_t *token_dev, void *stream) {
    PIE_REQUIRE(d && token_dev, PIE_E_ARG, "pie_decoder_set_token_from: null pointer");
    if (token_dev == d->token_out) return PIE_OK;  // the tail kernel already stored it in the device-side state
    PIE_HIP_TRY(hipMemcpyAsync(&d->state->token, token_dev, sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PIE_OK;
}

int pie_decoder_launch_kernel(pie_decoder *d, int which, int layer, void *stream) {
    int rc = ready(d);
    if (rc) return rc;
    PIE_REQUIRE(layer >= 0 && layer < d->cfg.n_layers, PIE_E_ARG, "pie_decoder_launch_kernel: layer out of range");
    PIE_REQUIRE(which != PIE_K_TAIL, PIE_E_ARG, "pie_decoder_launch_kernel: the tail advances the decode state; not launchable alone");
    return enqueue_kernel(d, which, layer, &d->state->token, d->logits, (hipStream_t)stream);
}

// Developer hook (not in the public header): the decoder's internal scratch vectors, for tools/step_bench's bisection.
void *pie_debug_buffer(pie_decoder *d, int which) {
    if (which == 7) return d->pf_sink;
    void *p[] = {d->qbuf, d->attn, d->act, d->part_acc, d->part_ml};
    return which >= 0 && which < 5 ? p[which] : nullptr;
}

int pie_decoder_configure(pie_decoder *d, int option, int value) {
    PIE_REQUIRE(d, PIE_E_ARG, "pie_decoder_configure: null decoder");
    PIE_REQUIRE(option == PIE_OPT_KV_I8, PIE_E_ARG, "pie_decoder_configure: unknown option");
    d->kv_i8 = value != 0;
    plan_attention(d);
    drop_graphs(d);
    return PIE_OK;
}

// the T [block_rows, vocab] logits block at the head of the prompt log-probabilities' workspace, padded so that the op's part stays 16-byte aligned
static size_t prompt_block_bytes(const pie_decoder *d, int block_rows) { return ((size_t)block_rows * d->cfg.vocab * 2 + 15) & ~(size_t)15; }

int pie_decoder_set_logits_penalty(pie_decoder *d, double penalty, int context_size, int32_t *ids_by_pos, int ids_cap) {
    if (int rc = tail_entry(d, "pie_decoder_set_logits_penalty")) return rc;
    PIE_REQUIRE(penalty >= 0.0 && std::isfinite(penalty), PIE_E_ARG, "pie_decoder_set_logits_penalty: the penalty must be finite and non-negative");
    PIE_REQUIRE(context_size >= 0 && context_size <= PEN_MAX_IDS, PIE_E_ARG, "pie_decoder_set_logits_penalty: context_size must be 1..1024 (0: off)");
    if (penalty == 1.0 || context_size == 0) penalty = 1.0, context_size = 0, ids_by_pos = nullptr, ids_cap = 0;
    else PIE_REQUIRE(ids_by_pos && ids_cap >= 1 && pie_aligned(ids_by_pos, 4), PIE_E_ARG, "pie_decoder_set_logits_penalty: ids_by_pos must hold at least one id");
    return set_part(d, d->tail.penalty, {penalty, context_size, ids_by_pos, ids_cap});
}

int pie_decoder_set_logits_mask(pie_decoder *d, const uint32_t *mask, int mask_words) {
    if (int rc = tail_entry(d, "pie_decoder_set_logits_mask")) return rc;
    if (mask) {
        PIE_REQUIRE(mask_words >= (d->cfg.vocab + 31) / 32, PIE_E_SHAPE, "pie_decoder_set_logits_mask: the mask needs ceil(vocab / 32) words");
        PIE_REQUIRE(pie_aligned(mask, 4), PIE_E_ALIGN, "pie_decoder_set_logits_mask: the mask needs 4-byte alignment");
        PIE_REQUIRE(!d->tail.dfa.on(), PIE_E_STATE, "pie_decoder_set_logits_mask: a token automaton is set (pie_decoder_set_token_dfa), and it writes the step's mask");
    }
    return set_part(d, d->tail.mask, {mask});
}

int pie_decoder_set_token_dfa(pie_decoder *d, const pie_row_dfa *record, int32_t *state, const int32_t *tables, int tables_len, uint32_t *mask, int mask_words) {
    if (int rc = tail_entry(d, "pie_decoder_set_token_dfa")) return rc;
    if (!record) return set_part(d, d->tail.dfa, {});  // off, whatever the other arguments say
    PIE_REQUIRE(mask, PIE_E_ARG, "pie_decoder_set_token_dfa: null pointer");
    if (int rc = token_dfa_check("pie_decoder_set_token_dfa", record, state, tables, tables_len, 1, d->cfg.vocab)) return rc;
    PIE_REQUIRE(mask_words >= (d->cfg.vocab + 31) / 32, PIE_E_SHAPE, "pie_decoder_set_token_dfa: the mask needs ceil(vocab / 32) words");
    PIE_REQUIRE(pie_aligned(mask, 4), PIE_E_ALIGN, "pie_decoder_set_token_dfa: the mask needs 4-byte alignment");
    PIE_REQUIRE(!d->tail.mask.on(), PIE_E_STATE, "pie_decoder_set_token_dfa: a token mask is set (pie_decoder_set_logits_mask), and the automaton writes a mask of its own");
    return set_part(d, d->tail.dfa, {record, state, tables, tables_len, mask, mask_words});
}

int pie_decoder_set_batch_token_dfa(pie_decoder *d, int rows_cap, const pie_row_dfa *records, int32_t *states, const int32_t *tables, int tables_len) {
    if (int rc = tail_entry(d, "pie_decoder_set_batch_token_dfa")) return rc;
    if (rows_cap == 0) return d->rows.dfa = {}, PIE_OK;  // off
    if (int rc = token_dfa_check("pie_decoder_set_batch_token_dfa", records, states, tables, tables_len, rows_cap, d->cfg.vocab)) return rc;
    PIE_REQUIRE(d->rows.edits.masks, PIE_E_STATE, "pie_decoder_set_batch_token_dfa: set the batch logits edits with a mask part first (pie_decoder_set_batch_logits_edits): the automata write its masks");
    d->rows.dfa = {records, states, tables, tables_len, rows_cap};  // (the batch graph's key holds them: no graph to drop)
    return PIE_OK;
}

int pie_decoder_set_logit_bias(pie_decoder *d, const int32_t *ids, const float *bias, int n) {
    if (int rc = tail_entry(d, "pie_decoder_set_logit_bias")) return rc;
    PIE_REQUIRE(n >= 0 && n <= PEN_MAX_IDS, PIE_E_ARG, "pie_decoder_set_logit_bias: 1 <= n <= 1024 entries (0: off)");
    if (n == 0) ids = nullptr, bias = nullptr;
    else {
        PIE_REQUIRE(ids && bias, PIE_E_ARG, "pie_decoder_set_logit_bias: null pointer");
        PIE_REQUIRE(pie_aligned(ids, 4) && pie_aligned(bias, 4), PIE_E_ALIGN, "pie_decoder_set_logit_bias: ids and bias need 4-byte alignment");
    }
    return set_part(d, d->tail.bias, {ids, bias, n});
}

int pie_decoder_set_sampler(pie_decoder *d, int mode, double temp, double p, int k, unsigned long long seed, unsigned long long *counter,
                            void *workspace, size_t workspace_bytes) {
    if (int rc = tail_entry(d, "pie_decoder_set_sampler")) return rc;
    if (mode == PIE_SAMPLE_GREEDY) return set_part(d, d->tail.sampler, {});  // off, whatever the other arguments say
    PIE_REQUIRE(counter && workspace, PIE_E_ARG, "pie_decoder_set_sampler: null pointer");
    if (int rc = sample_check("pie_decoder_set_sampler", d->cfg.vocab, mode, temp, p, k, workspace)) return rc;
    PIE_REQUIRE(workspace_bytes >= pie_sample_workspace_bytes(1, d->cfg.vocab), PIE_E_SHAPE, "pie_decoder_set_sampler: the workspace is smaller than pie_sample_workspace_bytes(1, vocab)");
    return set_part(d, d->tail.sampler, {mode, k, temp, p, seed, counter, workspace});
}

int pie_decoder_set_xtc(pie_decoder *d, const pie_xtc *record) {
    if (int rc = tail_entry(d, "pie_decoder_set_xtc")) return rc;
    PIE_REQUIRE(pie_aligned(record, 4), PIE_E_ALIGN, "pie_decoder_set_xtc: the record needs 4-byte alignment");
    return set_part(d, d->tail.xtc, {record});
}

int pie_decoder_set_batch_xtc(pie_decoder *d, const pie_xtc *records, int rows_cap) {
    if (int rc = tail_entry(d, "pie_decoder_set_batch_xtc")) return rc;
    if (!records) return d->rows.xtc = {}, PIE_OK;  // off
    PIE_REQUIRE(rows_cap >= 1, PIE_E_ARG, "pie_decoder_set_batch_xtc: rows_cap >= 1");
    PIE_REQUIRE(pie_aligned(records, 4), PIE_E_ALIGN, "pie_decoder_set_batch_xtc: the records need 4-byte alignment");
    d->rows.xtc = {records, rows_cap};  // (the batch graph's key holds them: no graph to drop)
    return PIE_OK;
}

int pie_decoder_set_top_logprobs(pie_decoder *d, int n, int32_t *out_ids, float *out_vals, void *workspace, size_t workspace_bytes) {
    if (int rc = tail_entry(d, "pie_decoder_set_top_logprobs")) return rc;
    if (n == 0) out_ids = nullptr, out_vals = nullptr, workspace = nullptr;
    else {
        PIE_REQUIRE(d->out_set, PIE_E_STATE, "pie_decoder_set_top_logprobs: bind_outputs must be called first");
        if (int rc = top_logprobs_check("pie_decoder_set_top_logprobs", 1, d->cfg.vocab, n, true, d->logprobs, d->token_out, nullptr, out_ids, out_vals, workspace)) return rc;
        PIE_REQUIRE(workspace_bytes >= pie_top_logprobs_workspace_bytes(1, d->cfg.vocab, n), PIE_E_SHAPE,
                    "pie_decoder_set_top_logprobs: the workspace is smaller than pie_top_logprobs_workspace_bytes(1, vocab, n)");
    }
    return set_part(d, d->tail.top, {n, out_ids, out_vals, workspace});
}

int pie_decoder_set_batch_top_logprobs(pie_decoder *d, int n, int rows_cap, int32_t *out_ids, float *out_vals, const int32_t *count, void *workspace) {
    if (int rc = tail_entry(d, "pie_decoder_set_batch_top_logprobs")) return rc;
    if (n == 0) return d->rows.top = {}, PIE_OK;  // off
    // (a pass is handed its logprobs per call: their alignment is checked there, with rows <= rows_cap)
    if (int rc = top_logprobs_check("pie_decoder_set_batch_top_logprobs", rows_cap, d->cfg.vocab, n, false, nullptr, nullptr, count, out_ids, out_vals, workspace)) return rc;
    d->rows.top = {n, rows_cap, out_ids, out_vals, count, workspace};  // (the batch graph's key holds them: no graph to drop)
    return PIE_OK;
}

size_t pie_decoder_prompt_logprobs_workspace_bytes(const pie_decoder *d, int n, int block_rows) {
    if (!d || block_rows < 8 || block_rows > 1024) return 0;
    const size_t op = pie_prompt_logprobs_workspace_bytes(block_rows, d->cfg.vocab, n);
    return op ? prompt_block_bytes(d, block_rows) + op : 0;
}

int pie_decoder_set_prompt_logprobs(pie_decoder *d, int n, int rows_cap, int block_rows, const int32_t *targets, const int32_t *count, int32_t *out_ids,
                                    float *out_vals, void *workspace, size_t workspace_bytes) {
    if (int rc = tail_entry(d, "pie_decoder_set_prompt_logprobs")) return rc;
    if (n == 0) return d->prompt = {}, PIE_OK;  // off
    PIE_REQUIRE(n >= 1 && n <= PIE_TOP_LOGPROBS_MAX, PIE_E_ARG, "pie_decoder_set_prompt_logprobs: n must be 1..20 (0: off)");
    PIE_REQUIRE(block_rows >= 8 && block_rows <= 1024, PIE_E_ARG, "pie_decoder_set_prompt_logprobs: block_rows must be 8..1024");
    PIE_REQUIRE(targets && count, PIE_E_ARG, "pie_decoder_set_prompt_logprobs: null pointer");
    if (int rc = prompt_logprobs_check("pie_decoder_set_prompt_logprobs", rows_cap, d->cfg.vocab, d->cfg.dtype, n, false, nullptr, targets, count, out_ids, out_vals, workspace)) return rc;
    PIE_REQUIRE(pie_aligned(workspace, 16), PIE_E_ALIGN, "pie_decoder_set_prompt_logprobs: the workspace needs 16-byte alignment (it starts with the logits block)");
    PIE_REQUIRE(workspace_bytes >= pie_decoder_prompt_logprobs_workspace_bytes(d, n, block_rows), PIE_E_SHAPE,
                "pie_decoder_set_prompt_logprobs: the workspace is smaller than pie_decoder_prompt_logprobs_workspace_bytes(n, block_rows)");
    d->prompt = {n, rows_cap, block_rows, targets, count, out_ids, out_vals, (u16 *)workspace, (char *)workspace + prompt_block_bytes(d, block_rows)};
    return PIE_OK;
}

int pie_decoder_set_batch_tail(pie_decoder *d, pie_row_tail *table, int rows_cap, int32_t *recent_ids, void *workspace) {
    if (int rc = tail_entry(d, "pie_decoder_set_batch_tail")) return rc;
    if (!table) return d->rows.sampler = {}, PIE_OK;  // off
    PIE_REQUIRE(recent_ids && workspace, PIE_E_ARG, "pie_decoder_set_batch_tail: null pointer");
    PIE_REQUIRE(pie_aligned(recent_ids, 4), PIE_E_ALIGN, "pie_decoder_set_batch_tail: the ring needs 4-byte alignment");
    if (int rc = sample_rows_check("pie_decoder_set_batch_tail", rows_cap, d->cfg.vocab, table, workspace)) return rc;
    d->rows.sampler = {table, rows_cap, recent_ids, workspace};  // (the batch graph's key holds them: no graph to drop)
    return PIE_OK;
}

int pie_decoder_set_batch_logits_edits(pie_decoder *d, int rows_cap, const uint32_t *masks, int mask_words, const int32_t *mask_on,
                                       const int32_t *bias_ids, const float *bias_vals, const int32_t *bias_n, int bias_cap) {
    if (int rc = tail_entry(d, "pie_decoder_set_batch_logits_edits")) return rc;
    if (rows_cap == 0) return d->rows.edits = {}, PIE_OK;  // off
    PIE_REQUIRE(rows_cap >= 1, PIE_E_ARG, "pie_decoder_set_batch_logits_edits: rows_cap >= 1 (0: off)");
    PIE_REQUIRE(bias_cap >= 0 && bias_cap <= PEN_MAX_IDS, PIE_E_ARG, "pie_decoder_set_batch_logits_edits: bias_cap must be 1..1024 (0: no bias part)");
    PIE_REQUIRE(masks || bias_cap, PIE_E_ARG, "pie_decoder_set_batch_logits_edits: neither a mask part nor a bias part");
    PIE_REQUIRE((masks != nullptr) == (mask_on != nullptr), PIE_E_ARG, "pie_decoder_set_batch_logits_edits: masks and mask_on come together");
    if (masks) {
        PIE_REQUIRE(mask_words >= (d->cfg.vocab + 31) / 32, PIE_E_SHAPE, "pie_decoder_set_batch_logits_edits: every row's mask needs ceil(vocab / 32) words");
        PIE_REQUIRE(pie_aligned(masks, 4) && pie_aligned(mask_on, 4), PIE_E_ALIGN, "pie_decoder_set_batch_logits_edits: masks and mask_on need 4-byte alignment");
    } else {
        mask_words = 0;
    }
    if (bias_cap) {
        PIE_REQUIRE(bias_ids && bias_vals && bias_n, PIE_E_ARG, "pie_decoder_set_batch_logits_edits: null pointer");
        PIE_REQUIRE(pie_aligned(bias_ids, 4) && pie_aligned(bias_vals, 4) && pie_aligned(bias_n, 4), PIE_E_ALIGN,
                    "pie_decoder_set_batch_logits_edits: bias_ids, bias_vals and bias_n need 4-byte alignment");
    } else {
        bias_ids = nullptr, bias_vals = nullptr, bias_n = nullptr;
    }
    d->rows.edits = {rows_cap, masks, mask_words, mask_on, bias_ids, bias_vals, bias_n, bias_cap};  // (the batch graph's key holds them: no graph to drop)
    return PIE_OK;
}

int pie_decoder_set_count_penalty(pie_decoder *d, pie_count_penalty *record, int32_t *counts) {
    if (int rc = tail_entry(d, "pie_decoder_set_count_penalty")) return rc;
    if (!record) counts = nullptr;
    else {
        PIE_REQUIRE(counts, PIE_E_ARG, "pie_decoder_set_count_penalty: a record needs its counts");
        PIE_REQUIRE(pie_aligned(record, 4) && pie_aligned(counts, 4), PIE_E_ALIGN, "pie_decoder_set_count_penalty: the record and the counts need 4-byte alignment");
    }
    return set_part(d, d->tail.counts, {record, counts});
}

int pie_decoder_set_dry_penalty(pie_decoder *d, const pie_dry_penalty *record, const int32_t *breakers, int32_t *ids_by_pos, int ids_cap) {
    if (int rc = tail_entry(d, "pie_decoder_set_dry_penalty")) return rc;
    if (!record) breakers = nullptr, ids_by_pos = nullptr, ids_cap = 0;
    else {
        PIE_REQUIRE(breakers && ids_by_pos && ids_cap >= 1, PIE_E_ARG, "pie_decoder_set_dry_penalty: a record needs its breakers and ids_by_pos [ids_cap >= 1]");
        PIE_REQUIRE(pie_aligned(record, 4) && pie_aligned(breakers, 4) && pie_aligned(ids_by_pos, 4), PIE_E_ALIGN,
                    "pie_decoder_set_dry_penalty: the record, the breakers and ids_by_pos need 4-byte alignment");
    }
    return set_part(d, d->tail.dry, {record, breakers, ids_by_pos, ids_cap});
}

int pie_decoder_set_batch_dry_penalty(pie_decoder *d, const pie_dry_penalty *records, const int32_t *breakers, int32_t *recent_ids, int rows_cap) {
    if (int rc = tail_entry(d, "pie_decoder_set_batch_dry_penalty")) return rc;
    if (!records) return d->rows.dry = {}, PIE_OK;  // off
    PIE_REQUIRE(breakers && recent_ids && rows_cap >= 1, PIE_E_ARG, "pie_decoder_set_batch_dry_penalty: the records need their breakers, their rings and rows_cap >= 1");
    PIE_REQUIRE(pie_aligned(records, 4) && pie_aligned(breakers, 4) && pie_aligned(recent_ids, 4), PIE_E_ALIGN,
                "pie_decoder_set_batch_dry_penalty: the records, the breakers and the rings need 4-byte alignment");
    d->rows.dry = {records, breakers, recent_ids, rows_cap};  // (the batch graph's key holds them: no graph to drop)
    return PIE_OK;
}

int pie_decoder_set_batch_count_penalty(pie_decoder *d, pie_count_penalty *records, int32_t *counts, int rows_cap) {
    if (int rc = tail_entry(d, "pie_decoder_set_batch_count_penalty")) return rc;
    if (!records) return d->rows.counts = {}, PIE_OK;  // off
    PIE_REQUIRE(counts && rows_cap >= 1, PIE_E_ARG, "pie_decoder_set_batch_count_penalty: the records need their counts and rows_cap >= 1");
    PIE_REQUIRE(pie_aligned(records, 4) && pie_aligned(counts, 4), PIE_E_ALIGN, "pie_decoder_set_batch_count_penalty: the records and the counts need 4-byte alignment");
    d->rows.counts = {records, counts, rows_cap};  // (the batch graph's key holds them: no graph to drop)
    return PIE_OK;
}

unsigned long long pie_decoder_batch_graph_replays(const pie_decoder *d) { return d ? d->batch_replays : 0; }
int pie_decoder_batch_graph_launches(const pie_decoder *d) { return d ? d->batch_graph_kernels : -1; }

int pie_decoder_set_comm(pie_decoder *d, pie_comm *c) {
    PIE_REQUIRE(d && c, PIE_E_ARG, "pie_decoder_set_comm: null pointer");
    int rank = 0, world = 0;
    size_t max_elems = 0;
    PIE_REQUIRE(tp_comm_geometry(c, &rank, &world, &max_elems) == PIE_OK, PIE_E_STATE, "pie_decoder_set_comm: the communicator is not connected");
    PIE_REQUIRE(d->tp() && rank == d->cfg.tp_rank && world == d->cfg.tp_world, PIE_E_ARG,
                "pie_decoder_set_comm: rank / world differ from the decoder's tp_rank / tp_world");
    PIE_REQUIRE(max_elems >= (size_t)d->cfg.hidden, PIE_E_SHAPE, "pie_decoder_set_comm: the communicator's slots are shorter than the hidden size");
    d->comm = c;
    drop_graphs(d);
    return PIE_OK;
}

int pie_decoder_status(pie_decoder *d, unsigned *error) {
    PIE_REQUIRE(d && error, PIE_E_ARG, "pie_decoder_status: null pointer");
    PIE_HIP_TRY(hipDeviceSynchronize());
    *error = 0;
    const int rc = d->comm ? pie_comm_status(d->comm, error) : PIE_OK;
    if (!rc && d->seam) {  // the fused q|k|v + attention launch: a kv-group's workgroups were not co-resident within its bounded wait (w4_gemv.hpp, FUSE)
        unsigned gave_up = 0;
        PIE_HIP_TRY(hipMemcpy(&gave_up, d->seam + 256, sizeof(unsigned), hipMemcpyDeviceToHost));
        if (gave_up) *error |= 0x80000000u;
    }
    return rc;
}

static size_t lin_bytes(const pie_decoder *d, const void *m, size_t n, size_t k) {  // algorithmic bytes of one Linear's weights
    const WeightFormat f = weight_format(d->mat_fmt(m));
    return n * k * f.bits / 8 + (f.group ? 2 * (n * k / f.group) * 2 : 0);  // codes + the group's 16-bit scale and bias (dense: the 16-bit weights)
}

size_t pie_decoder_kernel_bytes(const pie_decoder *d, int which, int T) {
    if (!d) return 0;
    const pie_decoder_config &c = d->cfg;
    const size_t H = c.hidden, I = c.inter, QD = (size_t)c.n_heads * c.head_dim, KVD = (size_t)c.n_kv_heads * c.head_dim;
    const pie_layer_weights &w = d->layers[0];  // per-kernel figure of layer 0 (layers of one checkpoint normally share their formats)
    switch (which) {
        case PIE_K_QKV: return lin_bytes(d, w.wqkv, QD + 2 * KVD, H) + H * 2 + 2 * KVD * 2;
        case PIE_K_ATTN: return 2 * KVD * 2 * (size_t)T;
        case PIE_K_OPROJ: return lin_bytes(d, w.wo, H, QD);
        case PIE_K_GATEUP: return lin_bytes(d, w.wgateup, 2 * I, H) + H * 2;
        case PIE_K_DOWN: return lin_bytes(d, w.wdown, H, I);
        case PIE_K_LMHEAD: return lin_bytes(d, d->glob.lm_head, c.vocab, H) + H * 2;
        case PIE_K_TAIL: return (size_t)c.vocab * 4;
        default: return 0;
    }
}

size_t pie_decoder_step_bytes(const pie_decoder *d, int T, int with_logits) {
    if (!d) return 0;
    const pie_decoder_config &c = d->cfg;
    const size_t H = c.hidden, I = c.inter, QD = (size_t)c.n_heads * c.head_dim, KVD = (size_t)c.n_kv_heads * c.head_dim;
    // int4 codes + 16-bit scale and bias per group of 64 = 0.5625 B / parameter  (SURVEY.md 8d); dense: 2 B / parameter
    size_t bytes = 0;
    for (const pie_layer_weights &w : d->layers)
        bytes += lin_bytes(d, w.wqkv, QD + 2 * KVD, H) + lin_bytes(d, w.wo, H, QD) + lin_bytes(d, w.wgateup, 2 * I, H) + lin_bytes(d, w.wdown, H, I) +
                 2 * H * 2 /* norm weights */ + 2 * KVD * 2 * (size_t)T /* KV read */ + 2 * KVD * 2 /* KV write */;
    if (with_logits) bytes += lin_bytes(d, d->glob.lm_head, c.vocab, H) + H * 2 + (size_t)c.vocab * 4 /* fp32 logprobs */;
    return bytes;
}

}  // extern "C"
