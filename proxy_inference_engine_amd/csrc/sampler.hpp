// sampler.hpp -- pie_sample's launch sequence for callers inside the library (sampler.hip): the decode step's tail draws with it.
#pragma once
#include "common.hpp"

// order-preserving key of a float (larger float <-> larger key); shared with top_logprobs.hip, whose rank order is this key's
__device__ __forceinline__ unsigned okey(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float okey_inv(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// A row's workspace starts with a header of 64-bit words.  A call clears every word it reads except these two, which it expects to be zero
// and leaves zero (the host zeroes the workspace once); a caller that moves rows about inside one allocation re-arms them itself
// (speculative.hip).  A row's stride is pie_sample_workspace_bytes(1, V).
constexpr int SMP_WS_MAXKEY_WORD = 0, SMP_WS_XTC_WORD = 3;

// Where the decode step's tail wants the drawn id besides `tokens` (rows = 1): the device-side state's fed-back token and the token history
// at the (already advanced) position *pos.  All null: a plain pie_sample.
struct SampleFeed {
    int *token;
    const int *pos;
    int *history;
    int hist_cap;
};

// XTC for a launch sequence (pie_sample_xtc's): device records -- one shared by the rows of sample_launch, one per row of
// sample_rows_launch -- and the nullable [rows] count of removed ids.  records == nullptr: off, the sequence is pie_sample's own.
struct SampleXtc {
    const pie_xtc *records;
    int *removed;
};

// a pie_row_tail's mode draws: one of sampler.hip's four modes; anything else acts as PIE_SAMPLE_GREEDY and leaves the record alone
__host__ __device__ inline bool sample_mode_draws(int mode) { return mode >= 0 && mode <= 3; }

// pie_sample's argument checks, reported under `who`; nothing is launched
int sample_check(const char *who, int V, int mode, double temp, double p, int k, const void *workspace);
// what the launches compute with, from pie_sample's parameters: the ONE place (pie_row_tail_pack's and the speculative verify's records draw as sample_launch does)
void sample_derive(int mode, double temp, double p, int k, float *inv_temp, float *thr, int *k_out);
int sample_launch(const float *logprobs, int rows, int V, int mode, double temp, double p, int k, unsigned long long seed, unsigned long long *counter,
                  void *workspace, int *tokens, int *kept_count, unsigned char *kept_mask, const SampleFeed &feed, hipStream_t st,
                  const SampleXtc &xtc = {});
// pie_sample_rows' checks and launches (per-row records in device memory): the multi-sequence passes' tail draws with them
int sample_rows_check(const char *who, int rows, int V, const void *table, const void *workspace);
int sample_rows_launch(const float *logprobs, int rows, int V, pie_row_tail *table, void *workspace, int *tokens, int *kept_count, unsigned char *kept_mask,
                       hipStream_t st, const SampleXtc &xtc = {});
