// decoder.hpp -- the decoder object shared by decoder.hip (single-token step) and prefill.hip (batched prompt).
#pragma once
#include <functional>
#include <unordered_map>
#include <vector>

#include "attention.hpp"
#include "kv_quant.hpp"
#include "sampler.hpp"
#include "tail.hpp"
#include "token_dfa.hpp"
#include "top_logprobs.hpp"
#include "prompt_logprobs.hpp"
#include "w4_gemv.hpp"

// The step's attention: its own launch | behind the q|k|v launch's seam, merged by o_proj's prologue | behind the seam and merged there
enum { ATTN_TWO_LAUNCHES = 0, ATTN_FUSED = 1, ATTN_FUSED_MERGED = 2 };

// The multi-sequence passes' per-row tail state (pie_decoder_step_batch, _prefill_batch, _step_mixed): four parts, each set as a
// whole by its own entry and off in its value-initialised state.  Caller-owned device memory, read on the device only, whose CONTENTS may
// change between calls; the addresses and sizes are launch arguments, so a captured batch graph bakes them in.  key(), check_rows() and
// edits_logits() are the only readers of "what is configured" besides the launches: a field that joins a part joins key() below it.
struct RowsTail {
    struct Sampler {  // pie_decoder_set_batch_tail: per-row records, rings of fed ids, the sampler's workspace
        pie_row_tail *table = nullptr;  // nullptr: off
        int rows_cap = 0;
        int *recent = nullptr;
        void *ws = nullptr;
    } sampler;
    struct Top {  // pie_decoder_set_batch_top_logprobs: pie_top_logprobs' launches behind the passes' tail
        int n = 0, rows_cap = 0;  // n == 0: off
        int *ids = nullptr;
        float *vals = nullptr;
        const int *count = nullptr;
        void *ws = nullptr;
    } top;
    struct Edits {  // pie_decoder_set_batch_logits_edits: per-row token masks and logit biases
        int rows_cap = 0;                 // 0: off
        const unsigned *masks = nullptr;  // [rows_cap, mask_words], nullptr: no mask part
        int mask_words = 0;
        const int *mask_on = nullptr, *bias_ids = nullptr;  // bias_ids, bias_vals: [rows_cap, bias_cap]
        const float *bias_vals = nullptr;
        const int *bias_n = nullptr;
        int bias_cap = 0;  // 0: no bias part
    } edits;
    struct Counts {  // pie_decoder_set_batch_count_penalty: per-row frequency / presence records and counts
        pie_count_penalty *records = nullptr;  // [rows_cap], nullptr: off
        int *counts = nullptr;                 // [rows_cap, vocab]
        int rows_cap = 0;
    } counts;
    struct Dry {  // pie_decoder_set_batch_dry_penalty: per-row DRY records, breaker tables and rings of fed ids (its own rings)
        const pie_dry_penalty *records = nullptr;  // [rows_cap], nullptr: off
        const int *breakers = nullptr;             // [rows_cap, PIE_DRY_BREAKERS_MAX]
        int *recent = nullptr;                     // [rows_cap, 1024]
        int rows_cap = 0;
    } dry;
    struct Xtc {  // pie_decoder_set_batch_xtc: per-row XTC records, read by the batch tail's sampler (nothing without one)
        const pie_xtc *records = nullptr;  // [rows_cap], nullptr: off
        int rows_cap = 0;
    } xtc;
    struct Dfa {  // pie_decoder_set_batch_token_dfa: per-row automaton records and states over one arena; writes the edits' masks
        const pie_row_dfa *records = nullptr;  // [rows_cap], nullptr: off
        int *states = nullptr;                 // [rows_cap]
        const int *tables = nullptr;           // [tables_len]
        int tables_len = 0, rows_cap = 0;
    } dfa;
    // everything a captured batch graph bakes in (pie_decoder_step_batch's key): a setter drops no graph, a changed key captures a new one
    void key(std::vector<uintptr_t> &k) const {
        for (uintptr_t v : {(uintptr_t)sampler.table, (uintptr_t)sampler.recent, (uintptr_t)sampler.ws, (uintptr_t)sampler.rows_cap,
                            (uintptr_t)top.n, (uintptr_t)top.rows_cap, (uintptr_t)top.ids, (uintptr_t)top.vals, (uintptr_t)top.count, (uintptr_t)top.ws,
                            (uintptr_t)edits.rows_cap, (uintptr_t)edits.masks, (uintptr_t)edits.mask_words, (uintptr_t)edits.mask_on, (uintptr_t)edits.bias_ids,
                            (uintptr_t)edits.bias_vals, (uintptr_t)edits.bias_n, (uintptr_t)edits.bias_cap,
                            (uintptr_t)counts.records, (uintptr_t)counts.counts, (uintptr_t)counts.rows_cap,
                            (uintptr_t)dry.records, (uintptr_t)dry.breakers, (uintptr_t)dry.recent, (uintptr_t)dry.rows_cap,
                            (uintptr_t)xtc.records, (uintptr_t)xtc.rows_cap,
                            (uintptr_t)dfa.records, (uintptr_t)dfa.states, (uintptr_t)dfa.tables, (uintptr_t)dfa.tables_len, (uintptr_t)dfa.rows_cap})
            k.push_back(v);
    }
    // a pass with `out_rows` output rows fits every configured part (checked before any launch)
    int check_rows(int out_rows, const char *entry) const {
        if (dfa.records && !edits.masks) return pie::fail(PIE_E_STATE, std::string(entry) + ": the batch token automata need the batch logits edits' mask part");
        const char *over = sampler.table && out_rows > sampler.rows_cap   ? "batch tail"
                           : edits.rows_cap && out_rows > edits.rows_cap  ? "batch logits edits"
                           : top.n && out_rows > top.rows_cap             ? "top log-probabilities"
                           : counts.records && out_rows > counts.rows_cap ? "batch count penalty"
                           : dry.records && out_rows > dry.rows_cap       ? "batch DRY penalty"
                           : xtc.records && out_rows > xtc.rows_cap       ? "batch XTC"
                           : dfa.records && out_rows > dfa.rows_cap       ? "batch token automata" : nullptr;
        return over ? pie::fail(PIE_E_SHAPE, std::string(entry) + ": more output rows than the " + over + "'s rows_cap") : PIE_OK;
    }
    // some part rewrites or masks the logits behind the lm_head: partials its epilogue left are stale
    bool edits_logits() const { return sampler.table || edits.rows_cap || counts.records || dry.records || dfa.records; }
    // The batched speculative pass (pie_decoder_spec_step_batch) is greedy and raw: every configured part is refused by name.
    const char *spec_refused() const {
        return sampler.table ? "a batch tail" : dfa.records ? "batch token automata" : edits.rows_cap ? "batch logits edits" : counts.records ? "a batch count penalty"
               : dry.records ? "a batch DRY penalty" : xtc.records ? "batch XTC records" : top.n ? "batch top log-probabilities" : nullptr;
    }
    // The pass under the seats' tails (pie_decoder_spec_step_batch_tail) admits the batch tail, the edits' bias part and the
    // XTC records; every other configured part is refused by name.
    const char *spec_tail_refused() const {
        return dfa.records ? "batch token automata" : edits.masks ? "a mask part of the batch logits edits" : counts.records ? "a batch count penalty"
               : dry.records ? "a batch DRY penalty" : top.n ? "batch top log-probabilities" : nullptr;
    }
};

// The single-sequence step's configured tail, applied where the tail writes the bound outputs and pie_decoder::tail_raw is
// false: nine parts, each set as a whole by its own entry and off in its value-initialised state.  Caller-owned device memory whose CONTENTS
// may change between steps; every field is a launch argument that a captured step graph bakes in, so a setter drops the graphs exactly when
// its part compares unequal (decoder.hip: set_part): a field that joins a part joins the operator== beside it.
struct StepTail {
    struct Penalty {  // pie_decoder_set_logits_penalty: the repetition penalty over the last `context` of ids_by_pos [ids_cap]
        double value = 1.0;  // 1.0: off
        int context = 0, *ids_by_pos = nullptr, ids_cap = 0;
        bool on() const { return value != 1.0; }
        bool operator==(const Penalty &o) const { return value == o.value && context == o.context && ids_by_pos == o.ids_by_pos && ids_cap == o.ids_cap; }
    } penalty;
    struct Sampler {  // pie_decoder_set_sampler: pie_sample's launches behind the finish
        int mode = PIE_SAMPLE_GREEDY, k = 0;  // PIE_SAMPLE_GREEDY: off
        double temp = 1.0, p = 0.0;
        unsigned long long seed = 0, *counter = nullptr;
        void *ws = nullptr;
        bool on() const { return mode != PIE_SAMPLE_GREEDY; }
        bool operator==(const Sampler &o) const { return mode == o.mode && k == o.k && temp == o.temp && p == o.p && seed == o.seed && counter == o.counter && ws == o.ws; }
    } sampler;
    struct Mask {  // pie_decoder_set_logits_mask: the token mask, applied by the fresh partials on their way
        const unsigned *words = nullptr;  // [>= ceil(vocab / 32)], nullptr: off
        bool on() const { return words != nullptr; }
        bool operator==(const Mask &o) const { return words == o.words; }
    } mask;
    struct Bias {  // pie_decoder_set_logit_bias
        const int *ids = nullptr;
        const float *vals = nullptr;
        int n = 0;  // 0: off
        bool on() const { return n != 0; }
        bool operator==(const Bias &o) const { return ids == o.ids && vals == o.vals && n == o.n; }
    } bias;
    struct Top {  // pie_decoder_set_top_logprobs: pie_top_logprobs' launches, last
        int n = 0, *ids = nullptr;  // n == 0: off
        float *vals = nullptr;
        void *ws = nullptr;
        bool on() const { return n != 0; }
        bool operator==(const Top &o) const { return n == o.n && ids == o.ids && vals == o.vals && ws == o.ws; }
    } top;
    struct Counts {  // pie_decoder_set_count_penalty: the frequency / presence record and its counts [vocab]
        pie_count_penalty *record = nullptr;  // nullptr: off
        int *counts = nullptr;
        bool on() const { return record != nullptr; }
        bool operator==(const Counts &o) const { return record == o.record && counts == o.counts; }
    } counts;
    struct Dry {  // pie_decoder_set_dry_penalty: the DRY record, breaker table [PIE_DRY_BREAKERS_MAX] and ids_by_pos [ids_cap]
        const pie_dry_penalty *record = nullptr;  // nullptr: off
        const int *breakers = nullptr;
        int *ids_by_pos = nullptr, ids_cap = 0;
        bool on() const { return record != nullptr; }
        bool operator==(const Dry &o) const { return record == o.record && breakers == o.breakers && ids_by_pos == o.ids_by_pos && ids_cap == o.ids_cap; }
    } dry;
    struct Xtc {  // pie_decoder_set_xtc: a launch argument of the sampler's launches, read only when a sampler is set
        const pie_xtc *record = nullptr;  // nullptr: off
        bool on() const { return record != nullptr; }
        bool operator==(const Xtc &o) const { return record == o.record; }
    } xtc;
    struct Dfa {  // pie_decoder_set_token_dfa: the automaton's record, state and arena, and the mask words the part writes
        const pie_row_dfa *record = nullptr;  // nullptr: off
        int *state = nullptr;
        const int *tables = nullptr;
        int tables_len = 0;
        unsigned *mask = nullptr;  // [mask_words >= ceil(vocab / 32)]: written by the mask op, read by the masked partials
        int mask_words = 0;
        bool on() const { return record != nullptr; }
        bool operator==(const Dfa &o) const { return record == o.record && state == o.state && tables == o.tables && tables_len == o.tables_len && mask == o.mask && mask_words == o.mask_words; }
    } dfa;
    LogitStat *tail_stats = nullptr;  // owned scratch, not configuration: [TAIL_STAT_TILES] partials of the edited logits (decoder.hip: set_part)
    // The only readers of "what is configured" besides the launches:
    // some part wants more than the greedy tail over the lm_head's own partials.  XTC is missing on purpose: it only changes a sampler's
    // draw, so alone it configures nothing (and with a sampler, the sampler answers).
    bool configured() const { return penalty.on() || sampler.on() || mask.on() || bias.on() || top.on() || counts.on() || dry.on() || dfa.on(); }
    // some part rewrites or masks the logits behind the lm_head: partials its epilogue left are stale.  The sampler, XTC and top-n are
    // missing on purpose: they read the finished log-probabilities and change no logit.
    bool edits_logits() const { return penalty.on() || mask.on() || bias.on() || counts.on() || dry.on() || dfa.on(); }
    // Speculation under a tail (speculative.hip: spec_prologue) admits the penalty, the bias, the sampler and XTC -- what its per-row edit
    // and its sampled verify apply -- and refuses every other part by name.  (The greedy and raw pass asks !configured() and !xtc.on().)
    const char *spec_tail_refused() const { return mask.on() ? "a token mask" : dfa.on() ? "a token automaton" : top.on() ? "a top-logprobs record" : counts.on() ? "frequency / presence counts" : dry.on() ? "a DRY penalty" : nullptr; }
    bool spec_tail_admitted() const { return penalty.on() || sampler.on() || bias.on() || xtc.on(); }
    // Speculation under a token automaton (pie_decoder_spec_step_dfa) admits what the tail's pass admits plus the automaton,
    // which alone is enough; every other part is refused under the name spec_tail_refused gives it.
    const char *spec_dfa_refused() const { return mask.on() ? "a token mask" : top.on() ? "a top-logprobs record" : counts.on() ? "frequency / presence counts" : dry.on() ? "a DRY penalty" : nullptr; }
};

// Log-probabilities of prompt tokens (pie_decoder_set_prompt_logprobs): the prompt passes score their rows in blocks of at most
// `block` rows -- lm_head into the logits block at the head of ws, then pie_prompt_logprobs' launches on the op's workspace behind it (op_ws).
// Caller-owned; record i belongs to row i of the call (ALL its N rows, not RowsTail's S output rows); n == 0: off.  In no graph's key.
struct PromptScores {
    int n = 0, rows_cap = 0, block = 0;
    const int *targets = nullptr, *count = nullptr;
    int *ids = nullptr;
    float *vals = nullptr;
    u16 *ws = nullptr;
    void *op_ws = nullptr;
    // the op on `rows` rows of logits, whose first row is row `row0` of the call
    int score_rows(const pie_decoder_config &cfg, const u16 *logits, int row0, int rows, hipStream_t st) const {
        return prompt_logprobs_launch(logits, rows, cfg.vocab, cfg.dtype, n, targets + row0, count + row0, ids + (size_t)row0 * (n + 1), vals + (size_t)row0 * (n + 1), op_ws, st);
    }
};

struct pie_decoder {
    pie_decoder_config cfg;
    std::vector<pie_layer_weights> layers;
    std::vector<char> layer_set;
    pie_global_weights glob;
    bool glob_set = false, kv_set = false;
    // device-side state and scratch (owned)
    DecState *state = nullptr;
    unsigned long long *kv_table = nullptr;  // [2*n_layers]
    // paged KV (pie_decoder_set_paged_kv): kv_table holds the layers' slab K / V bases, the caller-owned device block table
    // maps position p to page block_table[p / 64]; nullptr = contiguous per-layer buffers (pie_decoder_set_kv)
    const int *block_table = nullptr;
    int n_pages = 0;
    u16 *qbuf = nullptr, *attn = nullptr, *act = nullptr;
    float *part_acc = nullptr, *part_ml = nullptr, *rope_cs = nullptr;
    unsigned *pf_sink = nullptr;  // scratch for the developer builds' in-kernel stamps
    unsigned *seam = nullptr;     // the fused q|k|v + attention launch's per-XCD arrival counters / generations (w4_gemv.hpp, FUSE); zeroed once
    bool xcd_ok = false;          // the dispatcher places workgroups with equal blockIdx.x % 8 on one XCD (checked at creation)
    bool counted_live = false;    // this decoder is in g_live_decoders (decoder.hip)
    // How the step's attention runs (decoder.hip: attn_form).  Decided ONCE, where the q|k|v launch is enqueued; the ATTN and OPROJ launches that
    // follow it -- in a step, a capture or by name -- read this record, never the knobs: o_proj must take the input that was really written.
    int attn_form = ATTN_TWO_LAUNCHES;
    // caller-owned outputs (pie_decoder_bind_outputs)
    u16 *h = nullptr, *logits = nullptr;
    float *logprobs = nullptr;
    bool out_set = false;
    LogitStat *stats = nullptr;
    int *token_out = nullptr, *history = nullptr;
    int hist_cap = 0;
    int n_stats = 0, splits = GEMV_ATTN_SPLITS;
    // Attention plan, chosen from the cache capacity (host-known): short caches use <= 4 splits whose partials the o_proj
    // prologue merges (one launch less); long ones spread up to 32 splits per kv-head over the chip and merge them with
    // k_attn_combine -- the scoring loop is VALU work, 4 splits leave it on 32 CUs (83 us per layer at T = 8k, measured).
    bool combine = false;
    int merge_max_cap = 1024, kv_cap = 0;  // measured: merged wins at capacities 512 and 1024, the combine launch from 2048
    bool kv_i8 = false;  // PIE_OPT_KV_I8: the page slabs hold int8 pages (paged_i8.hip)
    bool row_is_h = false;  // the step's input row already sits in `h` (a row of caller-made embeddings): no embedding launch, no RoPE table
    // single-sequence step on int8 pages: the q|k|v GEMV's RoPE + append epilogue writes the new T rows into ONE staging page through a table of
    // staging pointers and an all-zero block table (the kernel is untouched), k_paged_kv_append_i8 quantises them into the sequence's page
    u16 *kv_stage = nullptr;                      // [2][n_kv, 64, D] T
    unsigned long long *kv_table_stage = nullptr;  // [2 * n_layers]: every layer -> the staging K / V block
    int *zero_table = nullptr;                     // [zero_blocks] zeros
    int zero_blocks = 0, max_blocks = 0;
    std::vector<const void *> slab_host;           // the layers' slab bases (host copy of kv_table's first half)
    // quantized KV (pie_decoder_set_kv_quant): the layers' K codes / scales / biases, V codes / scales / biases ([6 * n_layers], launch arguments of
    // the attention launch); the q|k|v epilogue stages the new T rows as for int8 pages and the attention launch quantizes them into the cache
    bool kv_quant = false;
    int kvq_gs = 0, kvq_bits = 0;
    std::vector<const void *> kvq_host;
    // the prompt pass on a quantized cache (prefill.hip): one layer's K and V as T [n_kv, kvq_scratch_cap, D] each, and a pointer table
    // [2 * n_layers] that points every layer at them
    u16 *kvq_scratch = nullptr;
    unsigned long long *kvq_table = nullptr;
    int kvq_scratch_cap = 0;
    // RotatingKVCache (pie_decoder_set_kv_ring) over the contiguous buffers of pie_decoder_set_kv: the window / sink rows live in the
    // device-side state (the step finds its row and length from pos); the q|k|v epilogue stages the new rows as for quantized KV and the
    // attention launch (RING) moves them into their ring slot.  ring_rows: a second DecState whose pos is the buffer row of the prompt
    // pass's first row (the retained window's length) and whose cap is the buffers' -- what the prompt pass's append and attention read.
    bool ring = false;
    int ring_w = 0, ring_row0 = 0;  // window; buffer row of the next prompt pass's first row (host copy of ring_rows->pos at bind time)
    DecState *ring_rows = nullptr;
    StepTail tail;          // the single-sequence step's configured tail
    bool tail_raw = false;  // per pass, not configuration: a prompt pass asked for logits on every position keeps raw logits and the greedy tail
    RowsTail rows;        // the multi-sequence passes' per-row tail state
    PromptScores prompt;  // the prompt passes' log-probabilities of prompt tokens
    unsigned long long batch_replays = 0;  // pie_decoder_step_batch calls served by the captured graph
    int batch_graph_kernels = -1;          // kernel nodes of the batch graph captured last
    hipGraphExec_t graph[2] = {nullptr, nullptr};  // [with_logits]
    int graph_kernels[2] = {-1, -1};                // kernel nodes of each captured graph (hipGraphGetNodes)
    int graph_form[2] = {ATTN_TWO_LAUNCHES, ATTN_TWO_LAUNCHES};  // the attn_form each graph was captured with (re-captured when that form is withdrawn)
    struct PrefillScratch *prefill = nullptr;       // batched prompt processing (prefill.hip), allocated on first use
    // tensor parallelism (cfg.tp_world > 1): this decoder is one rank's shard; comm is caller-owned (pie_decoder_set_comm)
    pie_comm *comm = nullptr;
    float *tp_part = nullptr;  // [hidden] fp32 partial of the row-parallel Linears, [hidden] = log-sum-exp of the step
    bool tp() const { return cfg.tp_world >= 1; }  // tp_world = 1: the tensor-parallel code path on one rank (tests; the RCCL backend's only test on one card)
    // per-matrix weight format (PIE_W_*), keyed by the packed matrix pointer; matrices not listed use cfg.weight_format
    std::unordered_map<const void *, int> fmt_map;
    int mat_fmt(const void *packed) const {
        auto it = fmt_map.find(packed);
        return it == fmt_map.end() ? cfg.weight_format : it->second;
    }
    bool uniform_int4() const {
        if (cfg.weight_format != PIE_W_INT4_G64) return false;
        for (const auto &kv : fmt_map)
            if (kv.second != PIE_W_INT4_G64) return false;
        return true;
    }
    int embed_vocab() const { return tp() ? cfg.vocab * cfg.tp_world : cfg.vocab; }
};

// tp_comm.hip: sum over the ranks of data[n] (rank order), then h = T(h + T(sum)) when resid != nullptr
int tp_allreduce_launch(pie_comm *c, int dtype, float *data, int n, u16 *resid, hipStream_t st, bool pushed);
bool tp_comm_push_args(const pie_comm *c, unsigned long long *const **peers, const unsigned **epoch, unsigned *stride);
int tp_tail_launch(pie_comm *c, int dtype, const u16 *logits, int V_local, int vocab_offset, const LogitStat *stats, int n_stats, float *lse, float *logprobs,
                   int *token, DecState *state, int *history, int hist_cap, hipStream_t st);
int tp_comm_geometry(const pie_comm *c, int *rank, int *world, size_t *max_elems);

int paged_kv_append_i8_staged_launch(int dtype, const void *stage_k, const void *stage_v, void *slab, int n_pages, const int *block_table, int max_blocks,
                                     const int *position, int Hkv, int D, hipStream_t st);
// paged_i8.hip: split-KV decode attention over int8 pages (a.slab = the layer's int8 slab, a.ctx_len / a.block_table as for T pages)
int paged_attn_i8_launch(int dtype, int D, const AttnArgs &a, hipStream_t st);

// decoder.hip: captures the launches enqueue(stream) queues into a graph, on a private non-blocking stream (the caller's may be the legacy default
// stream, which cannot be captured) in thread-local mode.  Returns the failure to begin the capture (enqueue did not run), else PIE_OK with
// enqueue's result in *enqueue_rc and the graph (the caller's to destroy) in *graph, or hipStreamEndCapture's error in *end_err.
int capture_graph(const std::function<int(hipStream_t)> &enqueue, int *enqueue_rc, hipGraph_t *graph, hipError_t *end_err);
int graph_kernel_nodes(hipGraph_t g);  // the kernel nodes `g` holds, -1 where the runtime does not tell

// prefill.hip: batched prompt processing (L >= prefill_min_rows() tokens): per layer many-row GEMMs on the weights' W4M tiles (int4) or
// W16M copies (the other formats), with hand-written HIP kernels for RoPE + cache append, causal attention and SwiGLU.
int prefill_min_rows();
int prefill_batched(pie_decoder *d, const int32_t *ids, const void *embeds, int L, void *logits_all, hipStream_t st);
void prefill_free(pie_decoder *d);
int enqueue_kernel(pie_decoder *d, int which, int li, const int *token_ptr, u16 *logits_dst, hipStream_t st, bool embed_here = false);  // embed_here: PIE_K_QKV of layer 0 also embeds the token
