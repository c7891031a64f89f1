/*
 * test_hooks.h -- measurement and test entry points of libkaldictc_amd.so
 * that have no reference counterpart and are not part of the drop-in ABI
 * (the headers under include/).  Used only by tests/, bench.py and scripts/.
 */
#ifndef KALDI_CTC_AMD_TEST_HOOKS_H_
#define KALDI_CTC_AMD_TEST_HOOKS_H_

#ifdef __cplusplus
extern "C" {
#endif

struct ihipStream_t;

/* Average ms of the packed gate GEMM (the kernel under kcm_add_mat_mat_x3
 * and the RNN GEMMs) on random packed operands, C[M][N] = A[M][K] B[N][K]^T, split-fp16 (bf16 = 0) or bf16
 * operands, split-K slices; -1 on failure. */
float kcm_bench_gemm_packed(struct ihipStream_t *stream, int M, int N, int K, int bf16, int iters, int split);
/* The packed GEMM on fp32 device operands A [M][K], B [N][K]: packs both
 * (split-fp16 rows with their exponents, or bf16 rows) and runs gemm_x3p into
 * C [M][N] = A B^T.  split > 1: split-K over a slab the hook allocates;
 * dynamic: tiles dealt from a counter; max_blocks: persistent grid; M2 > 0:
 * also C2 [M2][N] = A[:M2] B^T, both as one gemm_x3p_pair launch.  1 on
 * arguments the GEMM refuses, 3 on any other failure. */
int kcm_test_gemm_packed(struct ihipStream_t *stream, int M, int N, int K, int bf16, int split, int dynamic,
                         int max_blocks, int M2, const float *A, const float *B, float *C, float *C2);
/* The three hooks below run one library call on device memory that the caller
 * owns entirely (workspace and counters included, so that it can check guard
 * regions) and synchronise the stream.  0; 1 on arguments the hook or the
 * library (std::invalid_argument) refuses; 3 on any other failure.
 *
 * gemm_f32 with every field of GemmArgs (gemm.h).  split_k = -1: the split of
 * gemm_pick_split(M, N, K, batch); ws then needs that many slabs of
 * batch * M * N floats.  *split_used (may be null): the slabs the launch
 * runs, 1 without a split. */
int kcm_test_gemm_f32(struct ihipStream_t *stream, int transA, int transB, int M, int N, int K, float alpha,
                      float beta, const float *A, long lda, const float *B, long ldb, float *C, long ldc,
                      const float *bias, const float *bias2, int batch, long strideA, long strideB, long strideC,
                      long strideBias, int split_k, float *ws, int max_blocks, int *tile_counter, int *split_used);
/* gemm_pick_split(M, N, K, batch) and gemm_split_used(K, split_k); host code only. */
int kcm_test_gemm_pick_split(int M, int N, int K, int batch);
int kcm_test_gemm_split_used(int K, int split_k);
/* absmax_f32 (gemm.h): float bits of max |X| per row into rmax[b * strideR + r]
 * and per column into cmax[b * strideC + c]; either may be null. */
int kcm_test_absmax(struct ihipStream_t *stream, const float *X, long ldx, int rows, int cols, unsigned *rmax,
                    unsigned *cmax, int batch, long strideX, long strideR, long strideC);
/* One pack pass of gemm_x3p.h.  kind: 0 x3p_pack_rows, 1 x3p_pack_cols, 2
 * bf16_pack_rows, 3 bf16_pack_cols.  Rows: R rows of KC values (shift = 0),
 * batch matrices sX floats, sOut halves and sE ints apart.  Columns: the
 * transpose of X [R][KC], source row k - shift at k; one matrix (batch = 1,
 * strides 0).  Split-fp16 kinds: exponents into eout (may be null) from the
 * data (columns: cmax, float bits of each column's max |x|) or from bound
 * > 0; the bf16 kinds take neither (bound = 0, eout = cmax = null).
 * avoid_word / counter (x3p_pack_cols, both or neither): the PackAvoid launch
 * of 8 XCDs, a zeroed word and a zeroed int. */
int kcm_test_pack(struct ihipStream_t *stream, int kind, const float *X, long ldx, int R, int KC, int shift,
                  float bound, int batch, long sX, long sOut, long sE, void *out, int *eout, const unsigned *cmax,
                  const unsigned *avoid_word, int *counter);
/* The streamed direction-split GEMM of the RNN backward (dx) and chained forward (next projection) against a
 * producer that has already finished: C[M][N] = E[:, 0:K] Wt[0]^T +
 * E[:, K:2K] Wt[1]^T (+ bias[c]), E [M][2K], Wt [2][N][K], device pointers;
 * forward: the producer's direction order of a forward recurrence; tail_rows:
 * split-K tail slots per direction (-1: default).  1 on unsupported shapes. */
int kcm_test_row_stream(struct ihipStream_t *stream, int M, int N, int K, int forward, int tail_rows,
                        const float *E, const float *Wt, const float *bias, float *C);
/* A CuDNNRecurrentComponent handle (include/kaldi_nnet2_component.h) with
 * the trainer's side streams and forward-time prepacks on (on = 1): its
 * Propagate packs W^T and x^T / y^T beside the recurrence, its Backprop
 * streams dx and runs the weight GEMMs on the side stream, as in training. */
struct kctcComponentImpl;
int kctc_test_component_side_streams(struct kctcComponentImpl *h, int on);
/* Which v6 recurrence a layer of (mode, prec, H, dirs) runs at N sequences
 * (mode: 0 RELU, 1 TANH, 2 LSTM, 3 GRU; fwd: forward or backward-data): cfg =
 * {U, nth, rg, gs, variant (1 plain, 2 stacked, 3 IO-wave), usable CUs} --
 * zeros but the last when v6 does not apply -- and *kernel the address of the
 * kernel the lookup names for it (NULL then).  Nothing is launched. */
int kctc_test_rec6_select(int mode, int prec, int H, int dirs, int N, int fwd, int cfg[6], const void **kernel);
/* The whole plan of the recurrence that such a layer runs: plan = {version (6:
 * v6, 4: the generic kernels; 0: not supported, then all zeros), U, grid in
 * workgroups, threads per workgroup, dynamic LDS bytes, bit mask of the XCDs
 * a pinned v6 launch occupies, workgroups per (row group, direction), xpd
 * (generic: XCD slots per direction, 0 in plain block mapping; v6: 1 when
 * pinned)}.  Nothing is launched. */
int kctc_test_rec_plan(int mode, int prec, int H, int dirs, int N, int fwd, long plan[8]);
/* Byte offset, in the workspace of a one-layer RNN (mode, prec, D, H, dirs) at
 * (T, N), of the dGates column maxima its v6 backward recurrence leaves:
 * [2][dirs][nw H] floats as bits (DX, then the GRU's E; max over all frames of
 * |value|).  -1 on error.  Nothing is launched. */
long kctc_test_rnn_colmax_offset(int mode, int prec, int D, int H, int dirs, int T, int N);
/* LDA statistics (kaldi_lda.h).  lda is a kctcLda_t.  test_guards: *intact = 1
 * when the guard words around the device accumulators and the workspace are as
 * they were written (1 too before anything is allocated); waits for the
 * handle's work.  test_batch_rows: the spliced rows after which
 * kctc_lda_acc_egs hands a batch to accumulate (rows <= 0: the default, 8192);
 * returns the previous value. */
int kctc_lda_test_guards(void *lda, int *intact);
long kctc_lda_test_batch_rows(long rows);

#ifdef __cplusplus
}
#endif
#endif /* KALDI_CTC_AMD_TEST_HOOKS_H_ */
