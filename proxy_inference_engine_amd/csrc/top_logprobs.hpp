// top_logprobs.hpp -- pie_top_logprobs' checks and launches for callers inside the library (top_logprobs.hip): the decode step's configured
// tail and the multi-sequence passes end in them.
#pragma once
#include "common.hpp"

// pie_top_logprobs' argument checks, reported under `who`; nothing is launched.  have_logprobs == false: the rows are not known yet (the
// setter of the multi-sequence passes, which are handed their logprobs per call) and `logprobs` is not looked at.
int top_logprobs_check(const char *who, int rows, int V, int n, bool have_logprobs, const void *logprobs, const void *tokens, const void *count,
                       const void *out_ids, const void *out_vals, const void *workspace);
// its two launches (arguments already checked)
int top_logprobs_launch(const float *logprobs, int rows, int V, int n, const int *tokens, const int *count, int *out_ids, float *out_vals, void *workspace,
                        hipStream_t st);
