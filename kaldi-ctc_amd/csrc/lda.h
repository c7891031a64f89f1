// lda.h -- what the LDA sources share: the device accumulators behind
// kctc_lda_accumulate (lda_stats.hip), the host estimator (lda_estimate.cpp)
// and the handle of include/kaldi_lda.h (lda_api.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace kctc {
namespace lda {

constexpr int kMaxDim = 2048, kMaxClasses = 16384;
constexpr int kTile = 64;          // a workgroup's output tile is kTile x kTile
constexpr int kChunkRows = 1024;   // rows of one workgroup's partial sum
constexpr int kMaxPassChunks = 64; // chunks reduced by one launch pair
constexpr int kGuardWords = 8;     // fp64 guard words around every device array

// Device accumulators of one (dim, num_classes) problem; see lda_stats.hip.
class DeviceStats {
 public:
  DeviceStats(int dim, int num_classes, int device);
  ~DeviceStats();
  DeviceStats(const DeviceStats &) = delete;
  DeviceStats &operator=(const DeviceStats &) = delete;
  // stream-ordered; throws std::invalid_argument before anything is enqueued
  void Accumulate(hipStream_t stream, const float *feats, const int *cls, const float *weight, long R);
  // waits for the enqueued work; adds the device sums to zero [C], first [C][D]
  // and the lower triangle of second [D][D]
  void AddTo(double *zero, double *first, double *second);
  void Zero();
  bool GuardsIntact();
  int device() const { return device_; }

 private:
  void Allocate();
  void Order(hipStream_t stream);
  int D_, C_, device_;
  int ntiles_ = 0, pass_chunks_ = 1;
  double *acc_ = nullptr;  // [guard][zero C][guard][first C*D][guard][second D*D][guard]
  double *ws_ = nullptr;   // [guard][chunks][tiles][kTile*kTile][guard]
  size_t ws_chunks_ = 0;
  int4 *tiles_ = nullptr;  // {first output row, first output column, 1: class rows, 0}
  hipStream_t last_ = nullptr;
  bool used_ = false;
  hipEvent_t ev_ = nullptr;
  double *zero_() const { return acc_ + kGuardWords; }
  double *first_() const { return zero_() + C_ + kGuardWords; }
  double *second_() const { return first_() + (size_t)C_ * D_ + kGuardWords; }
  size_t acc_words_() const { return (size_t)C_ + (size_t)C_ * D_ + (size_t)D_ * D_ + 4 * kGuardWords; }
};

struct EstimateOptions {
  int dim = -1;
  double within_class_factor = 0.001;
  bool remove_offset = true;
  double max_singular_value = 5.0;
};

// LdaEstimate::GetStats + FeatureTransformEstimate::EstimateInternal in fp64.
// second: full [D][D], read through its lower triangle.  M: out_dim x
// (D + remove_offset) floats; cholesky: nullable, D x D.
void Estimate(const double *zero, const double *first, const double *second, int D, int C,
              const EstimateOptions &opts, float *M, double *cholesky);

// eigen-decomposition of the symmetric a [n][n] (destroyed) by cyclic Jacobi:
// w descending, row k of vt the eigenvector of w[k]; throws if 100 sweeps do not converge
void SymEig(std::vector<double> &a, int n, std::vector<double> *w, std::vector<double> *vt);

}  // namespace lda
}  // namespace kctc
