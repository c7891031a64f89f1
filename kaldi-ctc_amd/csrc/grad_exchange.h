// grad_exchange.h -- constructors of the GradExchange implementations
// (grad_exchange.cpp) for the data-parallel entry points of train_api.cpp.
#pragma once
#include "kaldi_ctc_train.h"
#include "nnet.h"

// RCCL all-reduce of every gradient bucket on a comm stream of its own
kctc::nnet2::GradExchange *kctc_new_rccl_exchange(const void *uid128, int rank, int world, hipStream_t compute);
// the same buckets summed through the caller's host all-reduce
kctc::nnet2::GradExchange *kctc_new_host_exchange(kctc_host_allreduce_fn fn, void *user, int world,
                                                  hipStream_t compute);
// one rank whose "all-reduce" holds `blocks` CUs for `usec` (the CU-budget probe)
kctc::nnet2::GradExchange *kctc_new_cu_probe_exchange(int blocks, double usec, hipStream_t compute);
