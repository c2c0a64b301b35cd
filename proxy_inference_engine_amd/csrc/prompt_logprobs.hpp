// prompt_logprobs.hpp -- pie_prompt_logprobs' checks and launches for callers inside the library (prompt_logprobs.hip): the prompt passes
// score their rows block by block through them.
#pragma once
#include "common.hpp"

// pie_prompt_logprobs' argument checks, reported under `who`; nothing is launched.  have_logits == false: the rows are not known yet (the
// decoder's setter: the logits block lies in its workspace) and `logits` is not looked at.
int prompt_logprobs_check(const char *who, int rows, int V, int dtype, int n, bool have_logits, const void *logits, const void *targets, const void *count,
                          const void *out_ids, const void *out_vals, const void *workspace);
// its four launches (arguments already checked)
int prompt_logprobs_launch(const u16 *logits, int rows, int V, int dtype, int n, const int *targets, const int *count, int *out_ids, float *out_vals,
                           void *workspace, hipStream_t st);
