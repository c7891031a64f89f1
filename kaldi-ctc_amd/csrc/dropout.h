// dropout.h -- DropoutComponent's forward and backward (nnet-component.cc:3551-3612)
// with a mask that is never stored: both directions compute it from a
// counter-based generator, so the backward regenerates what the forward drew.
//
// Generator: Philox4x32-10 as Random123 defines it (multipliers 0xD2511F53 /
// 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds).  Element
// i = r * dim + c (64-bit) uses word i % 4 of the block with
//   counter (v & 0xffffffff, v >> 32, draw, stream), v = i / 4,
//   key     (seed & 0xffffffff, seed >> 32),
// and nothing else: not the grid, not the vector width, not the row count.
// Element i is kept iff word >= thr, thr = (uint32) floor(dp * 2^32) (computed
// in double on the host from the float dp; dp = 0 keeps everything).  The
// values are the reference's (nnet-component.cc:3573-3590):
//   low = dropout_scale, high = (1 - dp * low) / (1 - dp), m = kept ? high : low
// with high evaluated in double from the floats dp and low and rounded once to
// float (the reference's expression has double literals too).
//   forward   out[i]      = in[i] * m
//   backward  in_deriv[i] = out_deriv[i] * m      (in_deriv may alias out_deriv)
//
// Deliberate difference from the reference: its backward is
// out_deriv * out_value / in_value, with out_deriv passed through unscaled
// where in_value == 0 (cu-kernels.cu:587-599).  Regenerating m is the
// derivative of what the forward computed, reads one array instead of three,
// and differs from the reference only at exact zeros of the input.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kctc {

struct DropoutMask {
  uint64_t seed = 0;
  uint32_t stream = 0, draw = 0;
  float proportion = 0.5f, scale = 0.f;
};

// (uint32) floor(dp * 2^32), dp in [0, 1)
uint32_t dropout_threshold(float proportion);
// the kept elements' scale (above)
float dropout_high_scale(float proportion, float scale);

// one Philox4x32-10 block; 64-bit products, which compile to the mul_hi /
// mul_lo pair on the device
__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// stream-ordered on s; n = rows * dim elements
void dropout_forward(hipStream_t s, const float *in, float *out, long n, const DropoutMask &m);
void dropout_backward(hipStream_t s, const float *out_deriv, float *in_deriv, long n, const DropoutMask &m);

}  // namespace kctc
