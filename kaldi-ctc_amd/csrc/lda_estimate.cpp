// lda_estimate.cpp -- nnet-get-feature-transform on the host, in fp64:
// LdaEstimate::GetStats (src/transform/lda-estimate.cc:57-82) and
// FeatureTransformEstimate::EstimateInternal
// (src/nnet2/get-feature-transform.cc:40-127) restated from (zero, first,
// second).  No LAPACK: Cholesky, a triangular inverse and a cyclic Jacobi
// eigen-solver.  Jacobi costs O(D^3) per sweep and takes 6-10 sweeps: a blink
// at the recipe's D = 360, minutes at D = 2048, a one-off either way.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <stdexcept>
#include <string>

#include "lda.h"

namespace kctc {
namespace lda {

void SymEig(std::vector<double> &a, int n, std::vector<double> *w, std::vector<double> *vt) {
  std::vector<double> v((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) v[(size_t)i * n + i] = 1.0;
  long rotations = 1;
  for (int sweep = 0; sweep < 100 && rotations; sweep++) {
    rotations = 0;
    for (int p = 0; p < n - 1; p++) {
      double *ap = &a[(size_t)p * n];
      for (int q = p + 1; q < n; q++) {
        double *aq = &a[(size_t)q * n];
        const double apq = ap[q];
        if (apq == 0.0) continue;
        const double app = ap[p], aqq = aq[q];
        // an element that cannot change either diagonal entry any more
        if (std::fabs(apq) <= 1e-20 * (std::fabs(app) + std::fabs(aqq))) {
          ap[q] = aq[p] = 0.0;
          continue;
        }
        rotations++;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; k++) {
          const double x = ap[k], y = aq[k];
          ap[k] = c * x - s * y;
          aq[k] = s * x + c * y;
        }
        ap[p] = app - t * apq;
        aq[q] = aqq + t * apq;
        ap[q] = aq[p] = 0.0;
        for (int k = 0; k < n; k++) {  // keep it symmetric: columns p, q = rows p, q
          if (k == p || k == q) continue;
          a[(size_t)k * n + p] = ap[k];
          a[(size_t)k * n + q] = aq[k];
        }
        double *vp = &v[(size_t)p * n], *vq = &v[(size_t)q * n];
        for (int k = 0; k < n; k++) {
          const double x = vp[k], y = vq[k];
          vp[k] = c * x - s * y;
          vq[k] = s * x + c * y;
        }
      }
    }
  }
  if (rotations) throw std::runtime_error("lda estimate: the Jacobi eigen-solver did not converge in 100 sweeps");
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int x, int y) { return a[(size_t)x * n + x] > a[(size_t)y * n + y]; });
  w->resize(n);
  vt->resize((size_t)n * n);
  for (int k = 0; k < n; k++) {
    (*w)[k] = a[(size_t)order[k] * n + order[k]];
    std::copy(&v[(size_t)order[k] * n], &v[(size_t)order[k] * n] + n, &(*vt)[(size_t)k * n]);
  }
}

// lower-triangular l with a = l l^T; false when a pivot is not positive
static bool cholesky(const std::vector<double> &a, int n, std::vector<double> *l) {
  l->assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) {
    double *li = &(*l)[(size_t)i * n];
    for (int j = 0; j <= i; j++) {
      const double *lj = &(*l)[(size_t)j * n];
      double s = a[(size_t)i * n + j];
      for (int k = 0; k < j; k++) s -= li[k] * lj[k];
      if (j < i) {
        li[j] = s / lj[j];
      } else {
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        li[i] = std::sqrt(s);
      }
    }
  }
  return true;
}

// inverse of the lower-triangular l (lower-triangular)
static std::vector<double> tri_inverse(const std::vector<double> &l, int n) {
  std::vector<double> x((size_t)n * n, 0.0);
  for (int j = 0; j < n; j++) {
    x[(size_t)j * n + j] = 1.0 / l[(size_t)j * n + j];
    for (int i = j + 1; i < n; i++) {
      double s = 0.0;
      for (int k = j; k < i; k++) s -= l[(size_t)i * n + k] * x[(size_t)k * n + j];
      x[(size_t)i * n + j] = s / l[(size_t)i * n + i];
    }
  }
  return x;
}

// c [m][n] = a [m][k] b [k][n]
static std::vector<double> matmul(const double *a, const double *b, int m, int k, int n) {
  std::vector<double> c((size_t)m * n, 0.0);
  for (int i = 0; i < m; i++)
    for (int x = 0; x < k; x++) {
      const double aix = a[(size_t)i * k + x];
      if (aix == 0.0) continue;
      const double *bx = b + (size_t)x * n;
      double *ci = &c[(size_t)i * n];
      for (int j = 0; j < n; j++) ci[j] += aix * bx[j];
    }
  return c;
}

void Estimate(const double *zero, const double *first, const double *second, int D, int C,
              const EstimateOptions &opts, float *M, double *chol_out) {
  if (!zero || !first || !second || !M) throw std::invalid_argument("lda estimate: null pointer");
  if (D < 1 || D > kMaxDim || C < 1 || C > kMaxClasses) throw std::invalid_argument("lda estimate: bad dimensions");
  const int target = opts.dim <= 0 ? D : opts.dim;
  if (target > D) throw std::invalid_argument("lda estimate: output dimension above the feature dimension");
  const size_t DD = (size_t)D * D;
  double count = 0.0;
  bool finite = true;
  for (int c = 0; c < C; c++) {
    finite = finite && std::isfinite(zero[c]);
    count += zero[c];
  }
  for (size_t i = 0; i < (size_t)C * D; i++) finite = finite && std::isfinite(first[i]);
  for (int i = 0; i < D; i++)
    for (int j = 0; j <= i; j++) finite = finite && std::isfinite(second[(size_t)i * D + j]);
  if (!finite) throw std::invalid_argument("lda estimate: a statistic is not finite");
  if (!(count > 0.0)) throw std::invalid_argument("lda estimate: the total count is not positive");

  // GetStats
  std::vector<double> mean(D, 0.0), total(DD), between(DD, 0.0), cm(D);
  for (int c = 0; c < C; c++)
    for (int j = 0; j < D; j++) mean[j] += first[(size_t)c * D + j];
  for (int j = 0; j < D; j++) mean[j] *= 1.0 / count;
  for (int c = 0; c < C; c++) {
    if (zero[c] == 0.0) continue;
    const double inv = 1.0 / zero[c], wgt = zero[c] / count;
    for (int j = 0; j < D; j++) cm[j] = first[(size_t)c * D + j] * inv;
    for (int i = 0; i < D; i++)
      for (int j = 0; j <= i; j++) between[(size_t)i * D + j] += wgt * cm[i] * cm[j];
  }
  for (int i = 0; i < D; i++)
    for (int j = 0; j <= i; j++) {
      const double mm = mean[i] * mean[j];
      total[(size_t)i * D + j] = second[(size_t)i * D + j] * (1.0 / count) - mm;
      between[(size_t)i * D + j] -= mm;
      total[(size_t)j * D + i] = total[(size_t)i * D + j];
      between[(size_t)j * D + i] = between[(size_t)i * D + j];
    }

  // within-class covariance and its Cholesky factor, smoothed once if need be
  std::vector<double> wc(DD), L;
  for (size_t i = 0; i < DD; i++) wc[i] = total[i] - between[i];
  if (!cholesky(wc, D, &L)) {
    double trace = 0.0;
    for (int i = 0; i < D; i++) trace += wc[(size_t)i * D + i];
    const double smooth = (double)(float)(1.0e-03 * trace / D);  // a BaseFloat in the reference
    for (int i = 0; i < D; i++) wc[(size_t)i * D + i] += smooth;
    if (!cholesky(wc, D, &L))
      throw std::runtime_error("lda estimate: the within-class covariance is not positive definite");
  }
  if (chol_out) std::copy(L.begin(), L.end(), chol_out);
  const std::vector<double> Linv = tri_inverse(L, D);

  // eigen-decomposition of Linv B Linv^T (symmetric positive semi-definite)
  std::vector<double> LinvT(DD);
  for (int i = 0; i < D; i++)
    for (int j = 0; j < D; j++) LinvT[(size_t)j * D + i] = Linv[(size_t)i * D + j];
  std::vector<double> Y = matmul(Linv.data(), between.data(), D, D, D);
  std::vector<double> T = matmul(Y.data(), LinvT.data(), D, D, D);
  for (int i = 0; i < D; i++)
    for (int j = 0; j < i; j++) T[(size_t)j * D + i] = T[(size_t)i * D + j] = 0.5 * (T[(size_t)i * D + j] + T[(size_t)j * D + i]);
  std::vector<double> d, Ut;
  SymEig(T, D, &d, &Ut);

  // M = U^T Linv, the first `target` rows, scaled
  std::vector<double> Mat = matmul(Ut.data(), Linv.data(), target, D, D);
  if (opts.within_class_factor != 1.0)
    for (int i = 0; i < target; i++) {
      const double scale = std::sqrt((opts.within_class_factor + d[i]) / (1.0 + d[i]));
      for (int j = 0; j < D; j++) Mat[(size_t)i * D + j] *= scale;
    }

  // ceiling on M's singular values: M = U diag(s) V^T with M M^T = U diag(s^2) U^T,
  // so the floored-down M is U diag(min(s, ceiling) / s) U^T M
  if (opts.max_singular_value > 0.0) {
    std::vector<double> G((size_t)target * target);
    for (int i = 0; i < target; i++)
      for (int j = 0; j <= i; j++) {
        double s = 0.0;
        for (int k = 0; k < D; k++) s += Mat[(size_t)i * D + k] * Mat[(size_t)j * D + k];
        G[(size_t)i * target + j] = G[(size_t)j * target + i] = s;
      }
    std::vector<double> s2, Wt;
    SymEig(G, target, &s2, &Wt);
    bool bites = false;
    std::vector<double> ratio(target, 1.0);
    for (int k = 0; k < target; k++) {
      const double s = std::sqrt(std::max(s2[k], 0.0));
      if (s > opts.max_singular_value) {
        ratio[k] = opts.max_singular_value / s;
        bites = true;
      }
    }
    if (bites) {
      std::vector<double> P = matmul(Wt.data(), Mat.data(), target, target, D);  // U^T M
      for (int k = 0; k < target; k++)
        for (int j = 0; j < D; j++) P[(size_t)k * D + j] *= ratio[k];
      std::vector<double> W((size_t)target * target);
      for (int i = 0; i < target; i++)
        for (int k = 0; k < target; k++) W[(size_t)i * target + k] = Wt[(size_t)k * target + i];
      Mat = matmul(W.data(), P.data(), target, target, D);
    }
  }

  const int cols = D + (opts.remove_offset ? 1 : 0);
  for (int i = 0; i < target; i++) {
    double off = 0.0;
    for (int j = 0; j < D; j++) {
      M[(size_t)i * cols + j] = (float)Mat[(size_t)i * D + j];
      off -= Mat[(size_t)i * D + j] * mean[j];
    }
    if (opts.remove_offset) M[(size_t)i * cols + D] = (float)off;
  }
}

}  // namespace lda
}  // namespace kctc
