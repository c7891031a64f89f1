// wfst_decode.h -- the graph search of wfst_decode.hip for callers inside the
// library (infer_api.cpp): utterance n's log-likelihood row of frame t starts
// at ll + ll_off[n] + t * ll_stride[n] (floats), so that time-major batches and
// utterance-major row blocks go through the same kernels.  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "wfst_graph.h"

namespace kctc {
namespace wfst {

// bytes of workspace of a decode call, 0: invalid arguments
size_t decode_workspace_bytes(const Graph *g, const int *lens, int N, int max_active, long pool_tokens);

// kctc_wfst_decode_async with explicit row addressing; returns its codes
int decode_strided(Graph *g, const float *ll, const int *lens, const long long *ll_off, const long long *ll_stride,
                   int A, int N, float acoustic_scale, float beam, int max_active, long pool_tokens, int *words,
                   int *words_len, int *ali, double *scores, int *status, void *workspace, hipStream_t stream);

}  // namespace wfst
}  // namespace kctc
