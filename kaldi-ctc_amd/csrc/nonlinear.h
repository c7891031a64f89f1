// nonlinear.h -- RectifiedLinearComponent's kernels (nonlinear.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace kctc {

// out = in < 0 ? 0 : in  (CopyFromMat + ApplyFloor(0.0), nnet-component.cc:
// 798-805); in == out allowed.  16-byte accesses when both pointers are
// 16-byte aligned (scalar tail for n % 4), scalar otherwise.
void relu_forward(hipStream_t s, const float *in, float *out, long n);

// RectifiedLinearComponent::Backprop + NonlinearComponent::UpdateStats in one
// pass over out_value / out_deriv [rows][dim] (the reference: CopyFromMat,
// ApplyHeaviside, two AddRowSumMat, MulElements; nnet-component.cc:807-826,
// 337-363):
//   in_deriv = out_value > 0 ? out_deriv : 0     (in_deriv non-null; it may
//                                                 alias out_deriv)
//   stats (non-null; device fp64, [2 * dim + 1]):
//     stats[0 .. dim)        += column sums of out_value        (value_sum)
//     stats[dim .. 2 dim)    += column sums of (out_value > 0)  (deriv_sum)
//     stats[2 dim]           += rows                            (count)
// The column sums are formed as sum_rows forms them: row slab p (rows p*4+w,
// + 4*slabs, ...; w = the wave) leaves fp32 partials in ws, a second launch
// adds the slabs in slab order in fp64 (16 groups of consecutive slabs side by
// side, then the groups in group order).  No atomics: the result depends on
// (rows, dim) only, never on launch timing.  ws >= relu_stats_ws_floats floats
// (needed only with stats).  16-byte accesses when dim % 4 == 0 and every
// pointer is 16-byte aligned (then every row is), scalar otherwise.
size_t relu_stats_ws_floats(long rows, int dim);
void relu_backprop_stats(hipStream_t s, const float *out_value, const float *out_deriv, float *in_deriv, long rows,
                         int dim, double *stats, float *ws);

// NonlinearComponent statistics arithmetic on the device (fp64, n = 2*dim+1):
// a[i] = alpha * a[i] + beta * b[i]; b null: a[i] = alpha * a[i]
// (Scale: b null; Add(beta, other): alpha = 1)
void stats_axpby(hipStream_t s, double *a, const double *b, long n, double alpha, double beta);
// the fp32 image the gradient exchange's float all-reduce carries, and back
void stats_to_float(hipStream_t s, const double *a, float *f, long n);
void stats_from_float(hipStream_t s, const float *f, double *a, long n);
// a[i] += b[i]; b[i] *= m                   (Nnet::AddNnet(1.0, delta, m))
void stats_fold(hipStream_t s, double *a, double *b, long n, double m);

}  // namespace kctc
