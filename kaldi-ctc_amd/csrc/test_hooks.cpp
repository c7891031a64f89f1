// test_hooks.cpp -- C ABI of csrc/test_hooks.h (measurement / test entry
// points outside the drop-in headers).
#include "test_hooks.h"

#include <stdexcept>

#include "common.h"
#include "gemm.h"
#include "rnn.h"

extern "C" {

float kcm_bench_gemm_packed(struct ihipStream_t *stream, int M, int N, int K, int bf16, int iters, int split) {
  if (M <= 0 || N <= 0 || K <= 0 || iters <= 0) return -1.f;
  try {
    return kctc::x3p_bench(stream, M, N, K, bf16 != 0, iters, split);
  } catch (...) {
    return -1.f;
  }
}

int kcm_test_row_stream(struct ihipStream_t *stream, int M, int N, int K, int forward, int tail_rows,
                        const float *E, const float *Wt, const float *bias, float *C) {
  if (!E || !Wt || !C || M <= 0 || N <= 0 || K <= 0 || K % 32) return 1;
  try {
    kctc::x3p_row_stream_selftest(stream, M, N, K / 32, forward, tail_rows, E, Wt, bias, C);
    return hipGetLastError() == hipSuccess ? 0 : 3;
  } catch (const std::invalid_argument &) {
    return 1;
  } catch (...) {
    return 3;
  }
}

int kctc_test_rec6_select(int mode, int prec, int H, int dirs, int N, int fwd, int cfg[6], const void **kernel) {
  if (!cfg || !kernel) return 1;
  try {
    kctc::RnnDesc d;
    d.mode = mode; d.prec = prec; d.D = d.H = H; d.dirs = dirs;
    *kernel = kctc::rnn_rec6_select(d, N, fwd != 0, cfg);
    cfg[5] = kctc::rnn_usable_cus();
    return 0;
  } catch (...) {
    return 3;
  }
}

int kctc_test_rec_plan(int mode, int prec, int H, int dirs, int N, int fwd, long plan[8]) {
  if (!plan) return 1;
  try {
    kctc::RnnDesc d;
    d.mode = mode; d.prec = prec; d.D = d.H = H; d.dirs = dirs;
    kctc::rnn_rec_plan(d, N, fwd != 0, plan);
    return 0;
  } catch (...) {
    return 3;
  }
}

}  // extern "C"
