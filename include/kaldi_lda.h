/*
 * kaldi_lda.h -- estimating the LDA-like feature transform of the recipe's
 * --add-lda true front end (steps/nnet2/get_lda.sh: ali-to-post |
 * weight-silence-post | acc-lda, sum-lda-accs, nnet-get-feature-transform), as
 * a C ABI over gfx950 kernels (csrc/lda_stats.hip) and a host estimator
 * (csrc/lda_estimate.cpp).
 *
 *   kctc_lda_accumulate           <- LdaEstimate::Accumulate
 *                                    (src/transform/lda-estimate.cc:45-55), a block
 *                                    of rows per call, fp64 on the matrix cores
 *   kctc_lda_write / kctc_lda_read <- LdaEstimate::Write / Read (:180-260);
 *                                    read with add = 1 is sum-lda-accs
 *   kctc_lda_estimate(_from_stats) <- LdaEstimate::GetStats (:57-82) and
 *                                    FeatureTransformEstimate::EstimateInternal
 *                                    (src/nnet2/get-feature-transform.cc:40-127)
 *   kctc_lda_acc_egs              <- acc-lda over an egs archive and the
 *                                    Int32Vector table kctc_nnet_align_egs writes
 * Return 0 on success (kctc_last_error() describes a failure).
 *
 * Only kctc_lda_accumulate and kctc_lda_acc_egs touch the device; a handle that
 * never accumulated (set_stats / read / write / estimate) and
 * kctc_lda_estimate_from_stats work on a machine without one.
 */
#ifndef KALDI_CTC_AMD_KALDI_LDA_H_
#define KALDI_CTC_AMD_KALDI_LDA_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

struct ihipStream_t;
typedef struct kctcLda_ *kctcLda_t;

#define KCTC_LDA_MAX_DIM 2048
#define KCTC_LDA_MAX_CLASSES 16384

/* blank_policy of kctc_lda_acc_egs */
#define KCTC_LDA_BLANK_SKIP 0  /* blank frames are not counted (weight-silence-post 0.0) */
#define KCTC_LDA_BLANK_CLASS 1 /* blank is class 0 */
#define KCTC_LDA_BLANK_FILL 2  /* a blank frame takes the next non-blank label of its
                                  utterance, trailing blanks the last one */

/* Accumulators for `dim` (1..2048) dimensional rows in `num_classes`
 * (1..16384) classes, all zero.  Nothing is allocated on `device` before the
 * first kctc_lda_accumulate. */
int kctc_lda_create(kctcLda_t *out, int dim, int num_classes, int device);
int kctc_lda_destroy(kctcLda_t h);

/* Adds R >= 0 rows: feats_dev [R][dim] fp32 row-major contiguous, class_dev
 * [R] int32, weight_dev [R] fp32 or null (weight 1), all on the handle's device:
 *   zero[c] += w_r;  first[c][:] += w_r x_r;  second += w_r x_r x_r^T   (c = class_dev[r])
 * in fp64 (products exact or rounded once, fp64 sums).  Rows whose id is
 * outside [0, num_classes) are selected out and may hold anything (NaN, Inf):
 * id < 0 marks the padding rows of a time-major batch.  Stream-ordered on
 * `stream`: no host synchronisation, and no allocation once the workspace has
 * grown to the largest R seen (it depends on R only through min(R, 65536)).  No
 * floating-point atomics: the rows are split in fixed chunks whose fp64
 * partial sums are added in a fixed order, so two identical call sequences
 * give identical bytes.  A bad argument (null pointer, R < 0) returns an error
 * and enqueues nothing. */
int kctc_lda_accumulate(kctcLda_t h, struct ihipStream_t *stream, const float *feats_dev, const int *class_dev,
                        const float *weight_dev, long R);

/* The statistics (host, fp64): zero [C], first [C][dim], second [dim][dim] (the
 * full symmetric matrix; exactly symmetric).  Waits for the accumulate calls
 * enqueued so far.  set_stats replaces them (add = 0) or adds to them (add = 1);
 * `second` is read through its lower triangle.  (What LdaEstimate::Read does
 * with numbers that are already in memory; kctc_lda_read is built on it.) */
int kctc_lda_get_stats(kctcLda_t h, double *zero, double *first, double *second);
int kctc_lda_set_stats(kctcLda_t h, const double *zero, const double *first, const double *second, int add);

/* LdaEstimate::Write / Read: <LDAACCS> <VECSIZE> dim <NUMCLASSES> C <ZERO_ACCS>
 * Vector<float> <FIRST_ACCS> Matrix<float> <SECOND_ACCS> SpMatrix<float>
 * </LDAACCS>, text or binary; the second-order block is the packed lower
 * triangle of second - sum_c first_c first_c^T / zero_c, undone on reading.
 * The file is float and therefore lossy.  read: add = 0 replaces the handle's
 * statistics, add = 1 adds the file's (sum-lda-accs); dimensions must match. */
int kctc_lda_write(kctcLda_t h, const char *path, int binary);
int kctc_lda_read(kctcLda_t h, const char *path, int add);

/* acc-lda over an egs archive (binary "ark:", read in archive order) and a
 * table of Int32Vector alignments (binary "ark:", read whole, looked up by
 * key).  For every example with an alignment a of length L: the output frames
 * are the example's rows left_context .. left_context + L - 1 (an example whose
 * rows do not cover them is a mismatch and is skipped); spliced row t is the
 * concatenation of the rows t + context[k] (n_context sorted offsets, 1..32,
 * n_context * feature dim = dim), indices clamped to the example's first and
 * last row (splice-feats' edge rule); the class of a frame is its symbol id
 * (label = pdf + 1, below num_classes) under blank_policy; entries of -1 skip
 * the frame.  Every frame counts with weight 1 (no --rand-prune).  Speaker
 * vectors of the examples are not part of the rows.  Outputs (nullable):
 * examples used, examples without an alignment, mismatches, frames accumulated. */
int kctc_lda_acc_egs(kctcLda_t h, const char *egs_rspecifier, const char *ali_rspecifier, const int *context,
                     int n_context, int blank_policy, long *num_used, long *num_no_ali, long *num_mismatch,
                     long *num_frames);

/* nnet-get-feature-transform: out_dim <= 0 is the full dimension; M receives
 * out_dim x (dim + 1 if remove_offset else dim) floats, row-major; cholesky
 * (nullable) dim x dim doubles, the lower-triangular factor of the within-class
 * covariance that was inverted (the reference's --write-cholesky; after the
 * smoothing retry, the factor of the smoothed matrix).  max_singular_value <= 0:
 * no ceiling.  Errors: out_dim > dim, a total count that is not positive, a
 * non-finite statistic, a null pointer, a within-class covariance that is not
 * positive definite even after smoothing. */
int kctc_lda_estimate(kctcLda_t h, int out_dim, double within_class_factor, int remove_offset,
                      double max_singular_value, float *M, double *cholesky);
int kctc_lda_estimate_from_stats(const double *zero, const double *first, const double *second, int dim,
                                 int num_classes, int out_dim, double within_class_factor, int remove_offset,
                                 double max_singular_value, float *M, double *cholesky);

#ifdef __cplusplus
}
#endif
#endif /* KALDI_CTC_AMD_KALDI_LDA_H_ */
