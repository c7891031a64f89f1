// lda_stats.hip -- LdaEstimate::Accumulate (src/transform/lda-estimate.cc:45-55)
// for a block of rows, in fp64 on gfx950's v_mfma_f64_16x16x4_f64.
//
// One product covers all three statistics.  With the R x D rows X, the weights
// w and the weighted one-hot matrix E[r][c] = w_r [class_r == c]:
//   second = (diag(w) X)^T X      first = E^T X      zero = E^T 1
// so the output is a (D + C) x (D + 1) matrix whose row operand is either a
// weighted feature column or a one-hot column generated on the fly, and whose
// column operand is a feature column or (column D, class rows only) ones.  It
// is cut into 64 x 64 tiles: the lower triangle of the D x D block and every
// tile of the class rows.  A workgroup (4 waves, 2 x 2, each 32 x 32 = 2 x 2
// MFMA tiles) owns one tile for one chunk of kChunkRows rows and writes its
// fp64 partial sums to the workspace; k_lda_reduce then adds the chunks of a
// pass to the accumulators in chunk order.  No atomics: the bytes depend only
// on the call sequence.
//
// Rows are staged 32 at a time in LDS as fp32 (both operands of a tile from
// that one row block) and widened on the way into the MFMA: fp32 -> fp64 is
// exact, w_r * x_ri is exact in fp64 (24 + 24 bits), and the MFMA rounds
// (w_r x_ri) * x_rj + acc in fp64.  Rows whose class id is outside [0, C) are
// selected out while staging (they may hold NaN), never multiplied by zero.
#include "lda.h"

#include <algorithm>
#include <stdexcept>

#include "common.h"

namespace kctc {
namespace lda {

using d4 = __attribute__((ext_vector_type(4))) double;

constexpr int kStageRows = 32;  // rows per LDS stage: 8 MFMA k-steps
constexpr int kLdsStride = 80;  // floats; the 4 rows of a k-step land in different banks
constexpr int kTileWords = kTile * kTile;
constexpr size_t kPassWords = (size_t)256 << 17;  // 256 MiB of fp64 partials per pass
constexpr double kGuardValue = -0x1.5a5a5a5a5a5a5p+77;

__global__ __launch_bounds__(256) void k_lda_partial(const float *__restrict__ X, const int *__restrict__ cls,
                                                     const float *__restrict__ w, long r0, long R, int D, int C,
                                                     const int4 *__restrict__ tiles, double *__restrict__ ws) {
  __shared__ float sA[kStageRows][kLdsStride], sB[kStageRows][kLdsStride];
  __shared__ float sW[kStageRows];
  __shared__ int sC[kStageRows];
  const int4 t = tiles[blockIdx.x];
  const int i0 = t.x, j0 = t.y;
  const bool cls_tile = t.z != 0;
  const long rb = r0 + (long)blockIdx.y * kChunkRows;
  const long re = min(R, rb + (long)kChunkRows);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wy = wave >> 1, wx = wave & 1;
  d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};

  for (long rs = rb; rs < re; rs += kStageRows) {
    // stage: wave `wave` takes rows wave, wave + 4, ...; a lane takes one column
    int hit = 0;
#pragma unroll
    for (int k = 0; k < kStageRows / 4; k++) {
      const int row = wave + 4 * k;
      const long r = rs + row;
      int c = -1;
      if (r < re) {
        c = cls[r];
        if ((unsigned)c >= (unsigned)C) c = -1;
      }
      float a = 0.f, b = 0.f;
      if (c >= 0) {
        const float *xr = X + (size_t)r * D;
        const int jb = j0 + lane;
        if (jb < D) b = xr[jb];
        else if (cls_tile && jb == D) b = 1.f;
        if (!cls_tile && i0 + lane < D) a = xr[i0 + lane];
        hit |= (c >= i0 && c < i0 + kTile);
      }
      sB[row][lane] = b;
      if (!cls_tile) sA[row][lane] = a;
      if (lane == 0) {
        sC[row] = c;
        sW[row] = c >= 0 ? (w ? w[r] : 1.f) : 0.f;
      }
    }
    // a class tile none of whose classes occurs in this row block adds nothing
    const int any = __syncthreads_or(cls_tile ? hit : 1);
    if (any) {
#pragma unroll
      for (int ks = 0; ks < kStageRows; ks += 4) {
        const int k = ks + (lane >> 4), m = lane & 15;
        const double wk = (double)sW[k];
        double a0, a1;
        if (cls_tile) {
          const int c = sC[k] - i0 - 32 * wy;
          a0 = c == m ? wk : 0.0;
          a1 = c == m + 16 ? wk : 0.0;
        } else {
          a0 = (double)sA[k][32 * wy + m] * wk;
          a1 = (double)sA[k][32 * wy + 16 + m] * wk;
        }
        const double b0 = (double)sB[k][32 * wx + m], b1 = (double)sB[k][32 * wx + 16 + m];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // f64 C/D map: column = lane & 15, row = (lane >> 4) + 4 * reg
  double *out = ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kTileWords;
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int row = 32 * wy + 16 * a + (lane >> 4) + 4 * reg;
        const int col = 32 * wx + 16 * b + (lane & 15);
        out[row * kTile + col] = acc[a][b][reg];
      }
}

// accumulator += the tile's partial sums of chunks 0, 1, ... in that order
__global__ __launch_bounds__(256) void k_lda_reduce(const double *__restrict__ ws, int nchunks, int D, int C,
                                                    const int4 *__restrict__ tiles, double *__restrict__ zero,
                                                    double *__restrict__ first, double *__restrict__ second) {
  const int4 t = tiles[blockIdx.x];
  const int e = blockIdx.y * 256 + threadIdx.x;
  const int i = t.x + (e >> 6), j = t.y + (e & 63);
  double *dst = nullptr;
  if (t.z) {
    if (i < C) {
      if (j < D) dst = first + (size_t)i * D + j;
      else if (j == D) dst = zero + i;
    }
  } else if (i < D && j <= i) {
    dst = second + (size_t)i * D + j;
  }
  if (!dst) return;
  double s = 0.0;
  for (int q = 0; q < nchunks; q++) s += ws[((size_t)q * gridDim.x + blockIdx.x) * kTileWords + e];
  *dst += s;
}

DeviceStats::DeviceStats(int dim, int num_classes, int device) : D_(dim), C_(num_classes), device_(device) {
  KCTC_REQUIRE(dim >= 1 && dim <= kMaxDim, "lda: dim outside [1, 2048]");
  KCTC_REQUIRE(num_classes >= 1 && num_classes <= kMaxClasses, "lda: num_classes outside [1, 16384]");
}

DeviceStats::~DeviceStats() {
  if (!acc_) return;
  (void)hipSetDevice(device_);
  (void)hipStreamSynchronize(last_);
  (void)hipFree(acc_);
  (void)hipFree(ws_);
  (void)hipFree(tiles_);
  if (ev_) (void)hipEventDestroy(ev_);
}

void DeviceStats::Allocate() {
  if (acc_) return;
  std::vector<int4> tiles;
  const int nfb = ceil_div(D_, kTile), ncb = ceil_div(C_, kTile), njb = ceil_div(D_ + 1, kTile);
  for (int bi = 0; bi < nfb; bi++)
    for (int bj = 0; bj <= bi; bj++) tiles.push_back(int4{bi * kTile, bj * kTile, 0, 0});
  for (int cb = 0; cb < ncb; cb++)
    for (int bj = 0; bj < njb; bj++) tiles.push_back(int4{cb * kTile, bj * kTile, 1, 0});
  ntiles_ = (int)tiles.size();
  pass_chunks_ = (int)std::min<size_t>(kMaxPassChunks, std::max<size_t>(1, kPassWords / kTileWords / ntiles_));
  KCTC_HIP_CHECK(hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
  KCTC_HIP_CHECK(hipMalloc(&tiles_, sizeof(int4) * tiles.size()));
  KCTC_HIP_CHECK(hipMemcpy(tiles_, tiles.data(), sizeof(int4) * tiles.size(), hipMemcpyHostToDevice));
  KCTC_HIP_CHECK(hipMalloc(&acc_, sizeof(double) * acc_words_()));
  KCTC_HIP_CHECK(hipMemset(acc_, 0, sizeof(double) * acc_words_()));
  const std::vector<double> g(kGuardWords, kGuardValue);
  for (double *p : {acc_, zero_() + C_, first_() + (size_t)C_ * D_, second_() + (size_t)D_ * D_})
    KCTC_HIP_CHECK(hipMemcpy(p, g.data(), sizeof(double) * kGuardWords, hipMemcpyHostToDevice));
  KCTC_HIP_CHECK(hipDeviceSynchronize());  // the fills above precede work on any stream
}

// work on a new stream starts after the work enqueued on the previous one
void DeviceStats::Order(hipStream_t stream) {
  if (used_ && stream != last_) {
    KCTC_HIP_CHECK(hipEventRecord(ev_, last_));
    KCTC_HIP_CHECK(hipStreamWaitEvent(stream, ev_, 0));
  }
  last_ = stream;
  used_ = true;
}

void DeviceStats::Accumulate(hipStream_t stream, const float *feats, const int *cls, const float *weight, long R) {
  KCTC_REQUIRE(R >= 0, "lda accumulate: negative row count");
  if (R == 0) return;
  KCTC_REQUIRE(feats && cls, "lda accumulate: null pointer");
  KCTC_HIP_CHECK(hipSetDevice(device_));
  Allocate();
  const long nchunks = (R + kChunkRows - 1) / kChunkRows;
  const size_t need = (size_t)std::min<long>(nchunks, pass_chunks_);
  if (need > ws_chunks_) {  // grow-only; the old one may still be read
    if (used_) KCTC_HIP_CHECK(hipStreamSynchronize(last_));
    if (ws_) KCTC_HIP_CHECK(hipFree(ws_));
    ws_ = nullptr;
    ws_chunks_ = 0;
    const size_t words = need * ntiles_ * kTileWords;
    KCTC_HIP_CHECK(hipMalloc(&ws_, sizeof(double) * (words + 2 * kGuardWords)));
    const std::vector<double> g(kGuardWords, kGuardValue);
    KCTC_HIP_CHECK(hipMemcpy(ws_, g.data(), sizeof(double) * kGuardWords, hipMemcpyHostToDevice));
    KCTC_HIP_CHECK(hipMemcpy(ws_ + kGuardWords + words, g.data(), sizeof(double) * kGuardWords,
                             hipMemcpyHostToDevice));
    KCTC_HIP_CHECK(hipDeviceSynchronize());
    ws_chunks_ = need;
  }
  Order(stream);
  double *ws = ws_ + kGuardWords;
  for (long q0 = 0; q0 < nchunks; q0 += pass_chunks_) {
    const int nq = (int)std::min<long>(pass_chunks_, nchunks - q0);
    hipLaunchKernelGGL(k_lda_partial, dim3(ntiles_, nq), dim3(256), 0, stream, feats, cls, weight,
                       q0 * kChunkRows, R, D_, C_, tiles_, ws);
    hipLaunchKernelGGL(k_lda_reduce, dim3(ntiles_, kTileWords / 256), dim3(256), 0, stream, ws, nq, D_, C_, tiles_,
                       zero_(), first_(), second_());
  }
  KCTC_HIP_CHECK(hipGetLastError());
}

void DeviceStats::AddTo(double *zero, double *first, double *second) {
  if (!acc_) return;
  KCTC_HIP_CHECK(hipSetDevice(device_));
  KCTC_HIP_CHECK(hipStreamSynchronize(last_));
  std::vector<double> h(acc_words_());
  KCTC_HIP_CHECK(hipMemcpy(h.data(), acc_, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  const double *z = h.data() + kGuardWords, *f = z + C_ + kGuardWords, *s = f + (size_t)C_ * D_ + kGuardWords;
  for (int c = 0; c < C_; c++) zero[c] += z[c];
  for (size_t i = 0; i < (size_t)C_ * D_; i++) first[i] += f[i];
  for (int i = 0; i < D_; i++)
    for (int j = 0; j <= i; j++) second[(size_t)i * D_ + j] += s[(size_t)i * D_ + j];
}

void DeviceStats::Zero() {
  if (!acc_) return;
  KCTC_HIP_CHECK(hipSetDevice(device_));
  KCTC_HIP_CHECK(hipStreamSynchronize(last_));
  KCTC_HIP_CHECK(hipMemset(zero_(), 0, sizeof(double) * C_));
  KCTC_HIP_CHECK(hipMemset(first_(), 0, sizeof(double) * C_ * D_));
  KCTC_HIP_CHECK(hipMemset(second_(), 0, sizeof(double) * D_ * D_));
  KCTC_HIP_CHECK(hipDeviceSynchronize());
}

bool DeviceStats::GuardsIntact() {
  if (!acc_) return true;
  KCTC_HIP_CHECK(hipSetDevice(device_));
  KCTC_HIP_CHECK(hipStreamSynchronize(last_));
  std::vector<const double *> at = {acc_, zero_() + C_, first_() + (size_t)C_ * D_, second_() + (size_t)D_ * D_};
  if (ws_) {
    at.push_back(ws_);
    at.push_back(ws_ + kGuardWords + ws_chunks_ * ntiles_ * kTileWords);
  }
  double g[kGuardWords];
  for (const double *p : at) {
    KCTC_HIP_CHECK(hipMemcpy(g, p, sizeof(g), hipMemcpyDeviceToHost));
    for (double v : g)
      if (v != kGuardValue) return false;
  }
  return true;
}

}  // namespace lda
}  // namespace kctc
