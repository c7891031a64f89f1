// dropout.hip -- DropoutComponent forward / backward for gfx950 (dropout.h).
//
// Memory-bound (one read and one write per element): each lane handles one
// Philox block = four consecutive elements = one 16-byte load and store per
// iteration, 256-thread blocks, at most 2048 of them with a grid-stride loop,
// no LDS.  The last n % 4 elements are done by the first lanes of block 0,
// each from its own block of the generator.  Pointers that are not 16-byte
// aligned (a caller's view into a larger buffer) take the element-wise kernel;
// the element -> word mapping is the same, so the mask is too.
#include "dropout.h"

#include <cmath>
#include <stdexcept>

#include "common.h"

namespace kctc {

namespace {

struct MaskArgs {
  uint32_t k0, k1, draw, stream, thr;
  float low, high;
};

__device__ __forceinline__ float mask_of(uint32_t word, const MaskArgs &a) { return word >= a.thr ? a.high : a.low; }

__device__ __forceinline__ void block_of(long v, const MaskArgs &a, uint32_t w[4]) {
  philox4x32_10((uint32_t)((unsigned long)v & 0xffffffffu), (uint32_t)((unsigned long)v >> 32), a.draw, a.stream,
                a.k0, a.k1, w);
}

__device__ __forceinline__ float one(const float *x, long i, const MaskArgs &a) {
  uint32_t w[4];
  block_of(i >> 2, a, w);
  const int j = (int)(i & 3);
  const uint32_t word = j == 0 ? w[0] : j == 1 ? w[1] : j == 2 ? w[2] : w[3];
  return x[i] * mask_of(word, a);
}

// x and y may be the same array (every element is read and written by one lane)
__global__ __launch_bounds__(256) void k_dropout_vec(const float *x, float *y, long n, MaskArgs a) {
  const long nvec = n >> 2;
  const float4 *x4 = reinterpret_cast<const float4 *>(x);
  float4 *y4 = reinterpret_cast<float4 *>(y);
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long)gridDim.x * 256) {
    float4 t = x4[v];
    uint32_t w[4];
    block_of(v, a, w);
    t.x *= mask_of(w[0], a);
    t.y *= mask_of(w[1], a);
    t.z *= mask_of(w[2], a);
    t.w *= mask_of(w[3], a);
    y4[v] = t;
  }
  const long i = (nvec << 2) + threadIdx.x;
  if (blockIdx.x == 0 && i < n) y[i] = one(x, i, a);
}

__global__ __launch_bounds__(256) void k_dropout_elem(const float *x, float *y, long n, MaskArgs a) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = one(x, i, a);
}

void launch(hipStream_t s, const float *x, float *y, long n, const DropoutMask &m) {
  if (n <= 0) return;
  if (!x || !y) throw std::invalid_argument("dropout: null array");
  MaskArgs a;
  a.k0 = (uint32_t)(m.seed & 0xffffffffu);
  a.k1 = (uint32_t)(m.seed >> 32);
  a.draw = m.draw;
  a.stream = m.stream;
  a.thr = dropout_threshold(m.proportion);
  a.low = m.scale;
  a.high = dropout_high_scale(m.proportion, m.scale);
  const bool aligned = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15u) == 0;
  const long work = aligned ? n >> 2 : n;
  const long blocks = (work + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks);
  if (aligned) hipLaunchKernelGGL(k_dropout_vec, dim3(grid), dim3(256), 0, s, x, y, n, a);
  else hipLaunchKernelGGL(k_dropout_elem, dim3(grid), dim3(256), 0, s, x, y, n, a);
  KCTC_HIP_CHECK(hipGetLastError());
}

}  // namespace

uint32_t dropout_threshold(float proportion) {
  if (!(proportion >= 0.f && proportion < 1.f)) throw std::invalid_argument("dropout proportion outside [0, 1)");
  return (uint32_t)std::floor((double)proportion * 4294967296.0);
}

float dropout_high_scale(float proportion, float scale) {
  return (float)((1.0 - (double)proportion * (double)scale) / (1.0 - (double)proportion));
}

void dropout_forward(hipStream_t s, const float *in, float *out, long n, const DropoutMask &m) {
  launch(s, in, out, n, m);
}

void dropout_backward(hipStream_t s, const float *out_deriv, float *in_deriv, long n, const DropoutMask &m) {
  launch(s, out_deriv, in_deriv, n, m);
}

}  // namespace kctc
