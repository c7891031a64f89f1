// test_hooks.cpp -- C ABI of csrc/test_hooks.h (measurement / test entry
// points outside the drop-in headers).
#include "test_hooks.h"

#include <stdexcept>

#include "common.h"
#include "gemm.h"
#include "gemm_x3p.h"
#include "rnn.h"

// runs f, waits for the stream and maps what happened to the hooks' status
template <typename F>
static int run_synced(struct ihipStream_t *stream, F &&f) {
  try {
    f();
    KCTC_HIP_CHECK(hipStreamSynchronize(stream));
    return hipGetLastError() == hipSuccess ? 0 : 3;
  } catch (const std::invalid_argument &) {
    return 1;
  } catch (...) {
    return 3;
  }
}

extern "C" {

float kcm_bench_gemm_packed(struct ihipStream_t *stream, int M, int N, int K, int bf16, int iters, int split) {
  if (M <= 0 || N <= 0 || K <= 0 || iters <= 0) return -1.f;
  try {
    return kctc::x3p_bench(stream, M, N, K, bf16 != 0, iters, split);
  } catch (...) {
    return -1.f;
  }
}

int kcm_test_gemm_packed(struct ihipStream_t *stream, int M, int N, int K, int bf16, int split, int dynamic,
                         int max_blocks, int M2, const float *A, const float *B, float *C, float *C2) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || split < 1 || M2 < 0 || M2 > M || (M2 > 0 && !C2)) return 1;
  char *buf = nullptr;
  int rc = 0;
  try {
    const int KB = bf16 ? (K + 63) / 64 : (K + 31) / 32;
    const size_t ap = (size_t)M * KB * 128, bp = (size_t)N * KB * 128, slab = sizeof(float) * (size_t)split * M * N;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    KCTC_HIP_CHECK(hipMalloc(&buf, up(ap) + up(bp) + 2 * up(slab) + up(sizeof(int) * (size_t)M) +
                                       up(sizeof(int) * (size_t)N) + up(sizeof(int))));
    char *o = buf;
    auto take = [&](size_t b) { char *r = o; o += up(b); return r; };
    _Float16 *Ap = reinterpret_cast<_Float16 *>(take(ap)), *Bp = reinterpret_cast<_Float16 *>(take(bp));
    float *ws = reinterpret_cast<float *>(take(slab)), *ws2 = reinterpret_cast<float *>(take(slab));
    int *eA = reinterpret_cast<int *>(take(sizeof(int) * (size_t)M)), *eB = reinterpret_cast<int *>(take(sizeof(int) * (size_t)N));
    int *counter = reinterpret_cast<int *>(take(sizeof(int)));
    if (bf16) {
      kctc::bf16_pack_rows(stream, A, K, M, K, reinterpret_cast<__bf16 *>(Ap));
      kctc::bf16_pack_rows(stream, B, K, N, K, reinterpret_cast<__bf16 *>(Bp));
    } else {
      kctc::x3p_pack_rows(stream, A, K, M, K, Ap, eA, 0.f);
      kctc::x3p_pack_rows(stream, B, K, N, K, Bp, eB, 0.f);
    }
    kctc::X3PArgs g;
    g.M = M; g.N = N; g.KB = KB; g.A = Ap; g.B = Bp; g.C = C; g.ldc = N; g.bf16 = bf16 != 0;
    if (!bf16) { g.eA = eA; g.eB = eB; }
    if (split > 1) { g.split_k = split; g.ws = ws; }
    g.max_blocks = max_blocks;
    if (dynamic || M2 > 0) g.tile_counter = counter;
    if (M2 > 0) {  // C2 = A[:M2] B^T: the packed rows of A are a prefix
      kctc::X3PArgs g2 = g;
      g2.M = M2; g2.C = C2; g2.ws = split > 1 ? ws2 : nullptr;
      kctc::gemm_x3p_pair(stream, g, g2);
    } else {
      kctc::gemm_x3p(stream, g);
    }
    KCTC_HIP_CHECK(hipStreamSynchronize(stream));
    rc = hipGetLastError() == hipSuccess ? 0 : 3;
  } catch (const std::invalid_argument &) {
    rc = 1;
  } catch (...) {
    rc = 3;
  }
  if (buf) (void)hipFree(buf);
  return rc;
}

int kcm_test_gemm_f32(struct ihipStream_t *stream, int transA, int transB, int M, int N, int K, float alpha,
                      float beta, const float *A, long lda, const float *B, long ldb, float *C, long ldc,
                      const float *bias, const float *bias2, int batch, long strideA, long strideB, long strideC,
                      long strideBias, int split_k, float *ws, int max_blocks, int *tile_counter, int *split_used) {
  if (!C || M <= 0 || N <= 0 || K < 0 || batch < 1 || (K > 0 && (!A || !B)) || split_k < -1 || split_k == 0 ||
      max_blocks < 0)
    return 1;
  if (split_k < 0) split_k = kctc::gemm_pick_split(M, N, K, batch);
  if (split_k > 1 && !ws) return 1;
  kctc::GemmArgs g;
  g.transA = transA != 0; g.transB = transB != 0;
  g.M = M; g.N = N; g.K = K; g.alpha = alpha; g.beta = beta;
  g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc;
  g.bias = bias; g.bias2 = bias2;
  g.batch = batch; g.strideA = strideA; g.strideB = strideB; g.strideC = strideC; g.strideBias = strideBias;
  g.split_k = split_k; g.ws = ws; g.max_blocks = max_blocks; g.tile_counter = tile_counter;
  if (split_used) *split_used = ws ? kctc::gemm_split_used(K, split_k) : 1;
  return run_synced(stream, [&] { kctc::gemm_f32(stream, g); });
}

int kcm_test_gemm_pick_split(int M, int N, int K, int batch) { return kctc::gemm_pick_split(M, N, K, batch); }
int kcm_test_gemm_split_used(int K, int split_k) { return kctc::gemm_split_used(K, split_k); }

int kcm_test_absmax(struct ihipStream_t *stream, const float *X, long ldx, int rows, int cols, unsigned *rmax,
                    unsigned *cmax, int batch, long strideX, long strideR, long strideC) {
  if (!X || rows <= 0 || cols <= 0 || batch < 1 || ldx < cols || (!rmax && !cmax)) return 1;
  return run_synced(stream, [&] {
    kctc::absmax_f32(stream, X, ldx, rows, cols, rmax, cmax, batch, strideX, strideR, strideC);
  });
}

int kcm_test_pack(struct ihipStream_t *stream, int kind, const float *X, long ldx, int R, int KC, int shift,
                  float bound, int batch, long sX, long sOut, long sE, void *out, int *eout, const unsigned *cmax,
                  const unsigned *avoid_word, int *counter) {
  if (kind < 0 || kind > 3 || !X || !out || R <= 0 || KC <= 0 || ldx < KC || batch < 1) return 1;
  const bool cols = kind == 1 || kind == 3, bf16 = kind >= 2;
  if (cols ? (batch != 1 || sX || sOut || sE) : shift != 0) return 1;
  if (bf16 && (bound != 0.f || eout || cmax)) return 1;
  if (kind == 1 ? (!(bound > 0.f) && !cmax) : cmax != nullptr) return 1;
  if ((avoid_word || counter) && (kind != 1 || !avoid_word || !counter)) return 1;
  return run_synced(stream, [&] {
    _Float16 *oh = static_cast<_Float16 *>(out);
    __bf16 *ob = static_cast<__bf16 *>(out);
    switch (kind) {
      case 0: kctc::x3p_pack_rows(stream, X, ldx, R, KC, oh, eout, bound, batch, sX, sOut, sE); break;
      case 1: {
        kctc::PackAvoid avoid;
        avoid.word = avoid_word; avoid.counter = counter;
        kctc::x3p_pack_cols(stream, X, ldx, R, KC, shift, oh, eout, cmax, bound, avoid);
        break;
      }
      case 2: kctc::bf16_pack_rows(stream, X, ldx, R, KC, ob, batch, sX, sOut); break;
      default: kctc::bf16_pack_cols(stream, X, ldx, R, KC, shift, ob); break;
    }
  });
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

long kctc_test_rnn_colmax_offset(int mode, int prec, int D, int H, int dirs, int T, int N) {
  try {
    kctc::RnnDesc d;
    d.mode = mode; d.D = D; d.H = H; d.dirs = dirs;
    kctc::rnn_set_precision(d, prec);
    return (long)kctc::rnn_ws_colmax_offset(d, T, N);
  } catch (...) {
    return -1;
  }
}

}  // extern "C"
