// nonlinear.hip -- RectifiedLinearComponent on gfx950 (nonlinear.h): the
// forward floor and the one-pass backward that also forms the
// NonlinearComponent statistics.  Both are streaming passes: 16-byte accesses,
// at most 8 blocks per CU with a grid-stride loop, no atomics.
#include "common.h"
#include "nonlinear.h"
#include "prof.h"

#include <algorithm>

namespace kctc {
namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr long kGridCap = 2048;  // 8 blocks per CU (seq_align.hip's training passes)
constexpr int kUnroll = 4;       // rows (forward: vectors) in flight per thread

__device__ __forceinline__ float relu(float x) { return x < 0.f ? 0.f : x; }

__global__ __launch_bounds__(256) void k_relu_fwd_v4(const float *in, float *out, long n) {
  const long n4 = n / 4, step = (long)gridDim.x * 256;
  const floatx4 *in4 = reinterpret_cast<const floatx4 *>(in);
  floatx4 *out4 = reinterpret_cast<floatx4 *>(out);
  // in may be out: every element is read by the thread that writes it, and
  // the loads of a batch are issued before its stores
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += step * kUnroll) {
    floatx4 v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; u++)
      if (i + u * step < n4) v[u] = in4[i + u * step];
#pragma unroll
    for (int u = 0; u < kUnroll; u++)
      if (i + u * step < n4) {
        floatx4 o;
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = relu(v[u][j]);
        out4[i + u * step] = o;
      }
  }
  // scalar tail (n % 4 elements)
  if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) out[n4 * 4 + threadIdx.x] = relu(in[n4 * 4 + threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_relu_fwd(const float *in, float *out, long n) {
  const long step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) out[i] = relu(in[i]);
}

// Grid (column tiles of 256, row slabs).  Wave w of slab p takes rows
// p*4 + w, + 4*slabs, ...; lane l the columns (tile*64 + l)*4 .. +3 (VEC) or
// tile*256 + l + 64*j (scalar).  kUnroll rows are loaded before any is stored.
template <bool VEC, bool STATS>
__global__ __launch_bounds__(256) void k_relu_bwd(const float *out_value, const float *out_deriv, float *in_deriv,
                                                  long rows, int dim, float *ws) {
  __shared__ float part[2][4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * 256;
  int col[4];
#pragma unroll
  for (int j = 0; j < 4; j++) col[j] = VEC ? tile + lane * 4 + j : tile + lane + 64 * j;
  float vs[4] = {0.f, 0.f, 0.f, 0.f}, ds[4] = {0.f, 0.f, 0.f, 0.f};
  const long rstep = 4L * gridDim.y;
  for (long r0 = (long)blockIdx.y * 4 + wave; r0 < rows; r0 += rstep * kUnroll) {
    float y[kUnroll][4], d[kUnroll][4];
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const long r = r0 + u * rstep;
      if (r >= rows) continue;
      const long base = r * dim;
      if (VEC) {
        if (col[0] < dim) {
          const floatx4 a = *reinterpret_cast<const floatx4 *>(out_value + base + col[0]);
          floatx4 b = {0.f, 0.f, 0.f, 0.f};
          if (in_deriv) b = *reinterpret_cast<const floatx4 *>(out_deriv + base + col[0]);
#pragma unroll
          for (int j = 0; j < 4; j++) { y[u][j] = a[j]; d[u][j] = b[j]; }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (col[j] < dim) {
            y[u][j] = out_value[base + col[j]];
            d[u][j] = in_deriv ? out_deriv[base + col[j]] : 0.f;
          }
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; u++) {
      const long r = r0 + u * rstep;
      if (r >= rows) continue;
      const long base = r * dim;
      if (VEC) {
        if (col[0] < dim) {
          floatx4 o;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const bool pos = y[u][j] > 0.f;
            o[j] = pos ? d[u][j] : 0.f;
            if (STATS) { vs[j] += y[u][j]; ds[j] += pos ? 1.f : 0.f; }
          }
          if (in_deriv) *reinterpret_cast<floatx4 *>(in_deriv + base + col[0]) = o;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (col[j] < dim) {
            const bool pos = y[u][j] > 0.f;
            if (in_deriv) in_deriv[base + col[j]] = pos ? d[u][j] : 0.f;
            if (STATS) { vs[j] += y[u][j]; ds[j] += pos ? 1.f : 0.f; }
          }
      }
    }
  }
  if (!STATS) return;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    part[0][wave][col[j] - tile] = vs[j];
    part[1][wave][col[j] - tile] = ds[j];
  }
  __syncthreads();
  const int c = tile + threadIdx.x;
  if (c < dim) {  // the four waves in wave order; slab blockIdx.y's partials: ws[slab][value | deriv][dim]
    const int t = threadIdx.x;
    float *w = ws + (long)blockIdx.y * 2 * dim;
    w[c] = ((part[0][0][t] + part[0][1][t]) + part[0][2][t]) + part[0][3][t];
    w[dim + c] = ((part[1][0][t] + part[1][1][t]) + part[1][2][t]) + part[1][3][t];
  }
}

// stats += the slabs' partials; count += rows.  One block per 64 columns of
// the [value | deriv] row; wave g of its 16 adds the slabs of group g
// ([g * per, (g + 1) * per)) in slab order in fp64, then wave 0 adds the 16
// group sums in group order: a fixed order for a given (rows, dim).
constexpr int kAddWaves = 16;
__global__ __launch_bounds__(64 * kAddWaves) void k_relu_stats_add(const float *ws, int slabs, int dim, long rows,
                                                                   double *stats) {
  __shared__ double part[kAddWaves][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane, n = 2 * dim;
  const int per = (slabs + kAddWaves - 1) / kAddWaves;
  const int p0 = g * per, p1 = min(slabs, p0 + per);
  double s = 0.0;
  if (c < n) {
#pragma unroll 8
    for (int p = p0; p < p1; p++) s += (double)ws[(long)p * n + c];
  }
  part[g][lane] = s;
  __syncthreads();
  if (g == 0 && c < n) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kAddWaves; k++) t += part[k][lane];
    stats[c] += t;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) stats[n] += (double)rows;
}

// a = alpha * a + beta * b (b null: a = alpha * a)
__global__ void k_stats_axpby(double *a, const double *b, long n, double alpha, double beta) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    a[i] = b ? alpha * a[i] + beta * b[i] : alpha * a[i];
}
__global__ void k_stats_to_float(const double *a, float *f, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) f[i] = (float)a[i];
}
__global__ void k_stats_from_float(const float *f, double *a, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) a[i] = (double)f[i];
}
__global__ void k_stats_fold(double *a, double *b, long n, double m) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const double d = b[i];
    a[i] += d;
    b[i] = d * m;
  }
}

bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }

int relu_slabs(long rows, int dim) {
  const long tiles = (dim + 255) / 256;
  const long cap = std::max<long>(1, kGridCap / tiles);
  return (int)std::max<long>(1, std::min<long>(cap, (rows + 4 * kUnroll - 1) / (4 * kUnroll)));
}

}  // namespace

void relu_forward(hipStream_t s, const float *in, float *out, long n) {
  if (n <= 0) return;
  if (aligned16(in) && aligned16(out)) {
    const long n4 = std::max<long>(1, n / 4);
    const unsigned grid = (unsigned)std::min<long>((n4 + 256 * kUnroll - 1) / (256 * kUnroll), kGridCap);
    hipLaunchKernelGGL(k_relu_fwd_v4, dim3(grid), dim3(256), 0, s, in, out, n);
  } else {
    const unsigned grid = (unsigned)std::min<long>((n + 255) / 256, kGridCap);
    hipLaunchKernelGGL(k_relu_fwd, dim3(grid), dim3(256), 0, s, in, out, n);
  }
  KCTC_HIP_CHECK(hipGetLastError());
}

size_t relu_stats_ws_floats(long rows, int dim) { return (size_t)2 * relu_slabs(rows, dim) * (size_t)dim; }

void relu_backprop_stats(hipStream_t s, const float *out_value, const float *out_deriv, float *in_deriv, long rows,
                         int dim, double *stats, float *ws) {
  if (rows <= 0 || dim <= 0 || (!in_deriv && !stats)) return;
  if (stats && !ws) throw std::invalid_argument("relu_backprop_stats: statistics need a workspace");
  const int slabs = relu_slabs(rows, dim);
  const dim3 grid((dim + 255) / 256, slabs);
  const bool vec = dim % 4 == 0 && aligned16(out_value) && aligned16(out_deriv) && aligned16(in_deriv);
  if (vec && stats)
    hipLaunchKernelGGL((k_relu_bwd<true, true>), grid, dim3(256), 0, s, out_value, out_deriv, in_deriv, rows, dim, ws);
  else if (vec)
    hipLaunchKernelGGL((k_relu_bwd<true, false>), grid, dim3(256), 0, s, out_value, out_deriv, in_deriv, rows, dim, ws);
  else if (stats)
    hipLaunchKernelGGL((k_relu_bwd<false, true>), grid, dim3(256), 0, s, out_value, out_deriv, in_deriv, rows, dim, ws);
  else
    hipLaunchKernelGGL((k_relu_bwd<false, false>), grid, dim3(256), 0, s, out_value, out_deriv, in_deriv, rows, dim, ws);
  if (stats) {
    ProfSpan ps(s, "relu_stats_add");
    hipLaunchKernelGGL(k_relu_stats_add, dim3((2 * dim + 63) / 64), dim3(64 * kAddWaves), 0, s, ws, slabs, dim, rows,
                       stats);
  }
  KCTC_HIP_CHECK(hipGetLastError());
}

static unsigned stats_grid(long n) { return (unsigned)std::min<long>((n + 255) / 256, kGridCap); }

void stats_axpby(hipStream_t s, double *a, const double *b, long n, double alpha, double beta) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_stats_axpby, dim3(stats_grid(n)), dim3(256), 0, s, a, b, n, alpha, beta);
  KCTC_HIP_CHECK(hipGetLastError());
}

void stats_to_float(hipStream_t s, const double *a, float *f, long n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_stats_to_float, dim3(stats_grid(n)), dim3(256), 0, s, a, f, n);
  KCTC_HIP_CHECK(hipGetLastError());
}

void stats_from_float(hipStream_t s, const float *f, double *a, long n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_stats_from_float, dim3(stats_grid(n)), dim3(256), 0, s, f, a, n);
  KCTC_HIP_CHECK(hipGetLastError());
}

void stats_fold(hipStream_t s, double *a, double *b, long n, double m) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_stats_fold, dim3(stats_grid(n)), dim3(256), 0, s, a, b, n, m);
  KCTC_HIP_CHECK(hipGetLastError());
}

}  // namespace kctc
