// wfst_decode.hip -- Viterbi token passing over a decoding graph for MI355X
// (gfx950): the best path of every utterance of a batch through a weighted
// finite-state transducer (include/kaldi_ctc_decode.h).
//
// Two launches per call, stream-ordered:
//   K1 wfst_search     one workgroup of 4 waves per utterance, serial over the
//                      frames, no traffic between workgroups.  The token set
//                      Q_t is a list of states plus one 64-bit key per state,
//                      (order-preserving image of the fp32 cost) << 32 |
//                      (arc id + 1), so that one integer atomic min decides
//                      "(cost, arc id) lexicographically smaller".  A frame is
//                        select   count the tokens inside the beam; if more
//                                 than max_active, a radix search (8 bits a
//                                 pass, LDS histogram) finds the max_active-th
//                                 smallest (cost bits, state id);
//                        emit     tokens in chunks of 256: a workgroup scan
//                                 of their arc counts, then one lane per ARC
//                                 (binary search of the arc's token), cost +
//                                 weight - scale * loglike from the row staged
//                                 in LDS, atomic min on the destination's key;
//                                 the lane that finds the key empty appends
//                                 the state to the next token list;
//                        closure  at most eps_depth rounds over a work list of
//                                 the states whose key fell in the round
//                                 before (a stamp per state keeps a state once
//                                 on the list), expanded like emit;
//                        append   every token gets a record (previous record,
//                                 arc id) in the utterance's pool, its cost is
//                                 rebased on the frame's best, which goes to
//                                 the fp64 offset; the old keys are cleared
//                                 through the old list.
//   K2 wfst_backtrace  one workgroup per utterance walks the winner's records
//                      through LDS windows of whole frames and writes ali, and
//                      the words from the end of their row, then moves them to
//                      its front.
// Deterministic outputs: the keys are unique minima; the order of the lists
// (and with it the record ids) may differ from run to run, nothing else.
#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "common.h"
#include "ctc_shared.h"
#include "kaldi_ctc_decode.h"
#include "nnet_handle.h"
#include "prof.h"
#include "wfst_decode.h"
#include "wfst_graph.h"

namespace kctc {
namespace wfst {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowLdsMax = 16384;  // columns of a log-likelihood row staged in LDS (64 KB); wider rows are read in place
constexpr int kBtWin = 4096;       // records per backtrace window (32 KB)
constexpr u64 kEmpty = ~0ull;

// ---- device image of a graph -------------------------------------------------
struct DevGraph {
  int S, start, eps_depth;
  const float *fin;       // [S]
  const int *emit_off;    // [S + 1]
  const int4 *emit;       // (arc id, dst, column, weight bits)
  const int *eps_off;     // [S + 1]
  const int4 *eps;        // (arc id, dst, 0, weight bits)
  const int2 *arc;        // [arcs] (src, ilabel)
  const int *olabel;      // [arcs]
};
struct DevImage {
  DevGraph g;
  void *mem;
};

static void free_image(int device, void *image) {
  DevImage *im = static_cast<DevImage *>(image);
  int prev = 0;
  if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(device) == hipSuccess) {
    (void)hipFree(im->mem);
    (void)hipSetDevice(prev);
  }
  delete im;
}

// the image on the current device, made (one allocation, one copy, one
// synchronisation) at the first decode there
static const DevGraph &device_graph(Graph *g) {
  int device = 0;
  KCTC_HIP_CHECK(hipGetDevice(&device));
  std::lock_guard<std::mutex> lock(g->dev_mutex);
  auto it = g->dev.find(device);
  if (it != g->dev.end()) return static_cast<DevImage *>(it->second)->g;
  const size_t S = g->num_states, NA = g->arcs.size(), NE = g->emit_arc.size(), NP = g->eps_arc.size();
  size_t p = 0;
  auto take = [&](size_t bytes) { const size_t at = p; p = align_up(p + bytes, 256); return at; };
  const size_t o_fin = take(4 * S), o_eoff = take(4 * (S + 1)), o_emit = take(16 * std::max<size_t>(NE, 1)),
               o_poff = take(4 * (S + 1)), o_eps = take(16 * std::max<size_t>(NP, 1)),
               o_arc = take(8 * std::max<size_t>(NA, 1)), o_ol = take(4 * std::max<size_t>(NA, 1));
  std::vector<char> host(p, 0);
  memcpy(&host[o_fin], g->final_cost.data(), 4 * S);
  memcpy(&host[o_eoff], g->emit_off.data(), 4 * (S + 1));
  memcpy(&host[o_poff], g->eps_off.data(), 4 * (S + 1));
  int4 *emit = reinterpret_cast<int4 *>(&host[o_emit]), *eps = reinterpret_cast<int4 *>(&host[o_eps]);
  auto wbits = [](float w) { int b; memcpy(&b, &w, 4); return b; };
  for (size_t e = 0; e < NE; e++) {
    const Arc &a = g->arcs[g->emit_arc[e]];
    emit[e] = make_int4(g->emit_arc[e], a.dst, g->ilabel_to_col[a.ilabel], wbits(a.weight));
  }
  for (size_t e = 0; e < NP; e++) {
    const Arc &a = g->arcs[g->eps_arc[e]];
    eps[e] = make_int4(g->eps_arc[e], a.dst, 0, wbits(a.weight));
  }
  int2 *arc = reinterpret_cast<int2 *>(&host[o_arc]);
  int *ol = reinterpret_cast<int *>(&host[o_ol]);
  for (size_t k = 0; k < NA; k++) {
    arc[k] = make_int2(g->arcs[k].src, g->arcs[k].ilabel);
    ol[k] = g->arcs[k].olabel;
  }
  std::unique_ptr<DevImage> im(new DevImage);
  KCTC_HIP_CHECK(hipMalloc(&im->mem, p));
  if (hipMemcpy(im->mem, host.data(), p, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(im->mem);
    throw HipError("copying the decoding graph to the device failed");
  }
  char *d = static_cast<char *>(im->mem);
  im->g.S = g->num_states;
  im->g.start = g->start;
  im->g.eps_depth = g->eps_depth;
  im->g.fin = reinterpret_cast<const float *>(d + o_fin);
  im->g.emit_off = reinterpret_cast<const int *>(d + o_eoff);
  im->g.emit = reinterpret_cast<const int4 *>(d + o_emit);
  im->g.eps_off = reinterpret_cast<const int *>(d + o_poff);
  im->g.eps = reinterpret_cast<const int4 *>(d + o_eps);
  im->g.arc = reinterpret_cast<const int2 *>(d + o_arc);
  im->g.olabel = reinterpret_cast<const int *>(d + o_ol);
  g->dev_free = free_image;
  DevImage *raw = im.release();
  g->dev[device] = raw;
  return raw->g;
}

// ---- workspace -----------------------------------------------------------------
struct Utt {
  int T;
  long long ll_off, ll_stride;  // loglikes of frame t: ll + ll_off + t * ll_stride
};
struct Fin {
  int rec, T;                    // record of the winning token (-1: none)
  long long expanded, held;      // sum over the frames of |E_t|, sum over t = 0..T of |Q_t|
};
// per utterance, in bytes from its base: keys [2][S] u64, rec [2][S] int, stamp [S] u32,
// list [2][S] int, cost [2][S] float, work [2][S] int, frame base [maxT + 2] int, pool [P] int2
struct Layout {
  size_t utt, fin, per, keys, rec, stamp, list, cost, work, fbase, pool, base, total;
  int max_T;
};

// the descriptors come first in a workspace, then one Fin per utterance
static size_t fin_offset(int N) { return align_up(sizeof(Utt) * (size_t)N, 256); }

static bool make_layout(const Graph &g, const int *lens, int N, int max_active, long pool_tokens, Layout *l,
                        std::vector<Utt> *utts) {
  if (N < 1 || !lens || max_active < 1 || max_active > (1 << 20) || pool_tokens < 1 || pool_tokens > INT_MAX - 2)
    return false;
  int max_T = 0;
  for (int n = 0; n < N; n++) {
    if (lens[n] < 0) return false;
    max_T = std::max(max_T, lens[n]);
  }
  // closure stamps are frame * (eps_depth + 2) + round as unsigned ints
  if (((long long)max_T + 2) * ((long long)g.eps_depth + 2) > 0xFFFFFFF0ll) return false;
  if (utts) {
    utts->resize(N);
    for (int n = 0; n < N; n++) (*utts)[n] = Utt{lens[n], 0, 0};
  }
  const size_t S = g.num_states;
  size_t p = 0;
  auto take = [&](size_t bytes) { const size_t at = p; p = align_up(p + bytes, 256); return at; };
  l->keys = take(16 * S);
  l->rec = take(8 * S);
  l->stamp = take(4 * S);
  l->list = take(8 * S);
  l->cost = take(8 * S);
  l->work = take(8 * S);
  l->fbase = take(4 * ((size_t)max_T + 2));
  l->pool = take(8 * (size_t)pool_tokens);
  l->per = p;
  p = 0;
  l->utt = take(sizeof(Utt) * N);  // == 0, and the next is fin_offset(N)
  l->fin = take(sizeof(Fin) * N);
  l->base = p;
  l->total = p + l->per * N;
  l->max_T = max_T;
  return true;
}

// ---- device helpers --------------------------------------------------------------
// order-preserving image of a finite float; 0xFFFFFFFF is never produced
__device__ __forceinline__ u32 fkey(float x) {
  const u32 u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(u32 k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// the keys and the stamps are read and cleared past the CU's vector cache: the
// atomics that update them act in L2
__device__ __forceinline__ u64 key_load(const u64 *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void key_store(u64 *p, u64 v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int wave_incl_scan(int x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

struct SearchArgs {
  DevGraph g;
  const float *ll;
  int A, row_in_lds;
  float scale, beam;
  int max_active, state_bits;
  long long pool_tokens;
  char *ws;
  size_t o_utt, o_fin, o_base, per, o_keys, o_rec, o_stamp, o_list, o_cost, o_work, o_fbase, o_pool;
  int *words_len;
  double *scores;
  int *status;
};

struct Shared {
  int off[kThreads];    // exclusive scan of the chunk's arc counts
  int lo[kThreads];     // first CSR entry of the chunk's tokens
  float cost[kThreads]; // their costs
  int hist[256];
  int wtot[kWaves];
  int cnt;       // tokens of the set under construction
  int wcnt[2];   // closure work lists
  int nb;        // tokens inside the beam
  u32 best;      // image of the smallest cost
  int bin, krem;
  u64 win_final, win_any;
};

// Relaxes the arcs (EMIT: emitting, else epsilon) of the `n` states of `list`
// into the key array `K`, one lane per arc.  EMIT: token i has cost costs[i]
// and takes part if it is inside the beam and, when pruning, not behind tau;
// else the cost is read from the state's key.  New states go to `tlist`;
// with !EMIT a state whose key fell goes once (stamp) to `wnext`.
template <bool EMIT>
__device__ __forceinline__ void expand(const SearchArgs &a, Shared &sh, const int *__restrict__ list, int n,
                                       const float *__restrict__ costs, bool prune, u64 tau, const float *row,
                                       u64 *K, int *tlist, u32 *stamps, u32 stamp, int *wnext, int *wcnt) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int *off = EMIT ? a.g.emit_off : a.g.eps_off;
  const int4 *ent = EMIT ? a.g.emit : a.g.eps;
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + tid;
    int cnt = 0, lo = 0;
    float c = 0.f;
    if (i < n) {
      const int s = list[i];
      bool in = true;
      if (EMIT) {
        c = costs[i];
        in = c <= a.beam && (!prune || (((u64)__float_as_uint(c) << 32) | (u32)s) <= tau);
      } else {
        c = fkey_inv((u32)(key_load(K + s) >> 32));
      }
      if (in) {
        lo = off[s];
        cnt = off[s + 1] - lo;
      }
    }
    const int incl = wave_incl_scan(cnt, lane);
    if (lane == 63) sh.wtot[wid] = incl;
    sh.lo[tid] = lo;
    sh.cost[tid] = c;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
      woff += w < wid ? sh.wtot[w] : 0;
      total += sh.wtot[w];
    }
    sh.off[tid] = woff + incl - cnt;
    __syncthreads();
    for (int j = tid; j < total; j += kThreads) {
      // the last token whose first arc is not behind j
      int k = 0;
#pragma unroll
      for (int step = kThreads / 2; step >= 1; step >>= 1)
        if (sh.off[k + step] <= j) k += step;
      const int4 e = ent[sh.lo[k] + (j - sh.off[k])];
      float cn = sh.cost[k] + __int_as_float(e.w);
      if (EMIT) cn += -a.scale * row[e.z];
      if (!(fabsf(cn) < INFINITY)) continue;  // a NaN or infinite cost starts no token
      const u64 key = ((u64)fkey(cn) << 32) | (u32)(e.x + 1);
      const u64 old = atomicMin(K + e.y, key);
      if (old == kEmpty) tlist[atomicAdd(&sh.cnt, 1)] = e.y;
      if (!EMIT && key < old && a.g.eps_off[e.y + 1] > a.g.eps_off[e.y]) {
        if (atomicExch(stamps + e.y, stamp) != stamp) wnext[atomicAdd(wcnt, 1)] = e.y;
      }
    }
    __syncthreads();  // sh.off, sh.lo, sh.cost are rewritten by the next chunk
  }
}

__global__ __launch_bounds__(kThreads) void wfst_search(SearchArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lrow[];
  __shared__ Shared sh;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int S = a.g.S;
  const Utt u = reinterpret_cast<const Utt *>(a.ws + a.o_utt)[n];
  char *base = a.ws + a.o_base + a.per * n;
  u64 *keys = reinterpret_cast<u64 *>(base + a.o_keys);
  int *rec = reinterpret_cast<int *>(base + a.o_rec);
  u32 *stamps = reinterpret_cast<u32 *>(base + a.o_stamp);
  int *lists = reinterpret_cast<int *>(base + a.o_list);
  float *costs = reinterpret_cast<float *>(base + a.o_cost);
  int *works = reinterpret_cast<int *>(base + a.o_work);
  int *fbase = reinterpret_cast<int *>(base + a.o_fbase);
  int2 *pool = reinterpret_cast<int2 *>(base + a.o_pool);
  const int T = u.T;
  const u32 rounds = (u32)a.g.eps_depth + 2;

  for (int i = tid; i < 2 * S; i += kThreads) key_store(keys + i, kEmpty);
  for (int i = tid; i < S; i += kThreads) __hip_atomic_store(stamps + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) {
    sh.cnt = 1;
    sh.wcnt[0] = sh.wcnt[1] = 0;
    sh.nb = 0;
    sh.best = 0xFFFFFFFFu;
    sh.win_final = sh.win_any = kEmpty;
  }
  __syncthreads();
  // Q_0 before its closure: the start token, cost 0, arc id -1
  if (tid == 0) {
    key_store(keys + a.g.start, (u64)fkey(0.f) << 32);
    lists[0] = a.g.start;
  }
  __syncthreads();

  double off = 0.0;
  int ncur = 0, recs = 0, failed = 0;  // tokens of Q_t, records used, -1 / -2
  long long expanded = 0;
  // frame f builds Q_f in buffer f & 1: f = 0 from the start token, f >= 1 by emission from Q_{f-1}
  for (int f = 0; f <= T; f++) {
    const int nb = f & 1, cb = nb ^ 1;
    u64 *K = keys + (size_t)nb * S;
    int *tl = lists + (size_t)nb * S;
    if (f > 0) {
      const int t = f - 1;
      const float *grow = a.ll + u.ll_off + (long long)t * u.ll_stride;
      const float *row = grow;
      if (a.row_in_lds) {
        for (int c = tid; c < a.A; c += kThreads) lrow[c] = grow[c];
        row = lrow;
      }
      const float *cc = costs + (size_t)cb * S;
      const int *cl = lists + (size_t)cb * S;
      // ---- select: tokens inside the beam (the best token has cost 0)
      int mine = 0;
      for (int i = tid; i < ncur; i += kThreads) mine += cc[i] <= a.beam ? 1 : 0;
      mine = wave_incl_scan(mine, lane);
      if (lane == 63 && mine) atomicAdd(&sh.nb, mine);
      __syncthreads();
      const int inbeam = sh.nb;
      const bool prune = inbeam > a.max_active;
      expanded += min(inbeam, a.max_active);
      u64 tau = 0;
      if (prune) {  // workgroup-uniform
        // the max_active-th smallest (cost bits, state): costs are >= +0, their bits order them
        int krem = a.max_active;
        for (int shift = 56; shift >= 0; shift -= 8) {
          if (shift < 32 && shift >= (a.state_bits + 7) / 8 * 8) continue;  // tau's digit stays 0
          sh.hist[tid] = 0;
          __syncthreads();
          for (int i = tid; i < ncur; i += kThreads) {
            const float c = cc[i];
            if (c <= a.beam) {
              const u64 k = ((u64)__float_as_uint(c) << 32) | (u32)cl[i];
              if (shift == 56 || (k >> (shift + 8)) == (tau >> (shift + 8))) atomicAdd(&sh.hist[(k >> shift) & 255], 1);
            }
          }
          __syncthreads();
          if (tid < 64) {  // wave 0: the digit at which the running count reaches krem
            const int h0 = sh.hist[4 * lane], h1 = sh.hist[4 * lane + 1], h2 = sh.hist[4 * lane + 2],
                      h3 = sh.hist[4 * lane + 3];
            const int incl = wave_incl_scan(h0 + h1 + h2 + h3, lane);
            const int excl = incl - (h0 + h1 + h2 + h3);
            if (excl < krem && krem <= incl) {  // exactly one lane
              int r = krem - excl, b = 0;
              if (r > h0) { r -= h0; b = 1;
                if (r > h1) { r -= h1; b = 2;
                  if (r > h2) { r -= h2; b = 3; } } }
              sh.bin = 4 * lane + b;
              sh.krem = r;
            }
          }
          __syncthreads();
          tau |= (u64)sh.bin << shift;
          krem = sh.krem;
        }
      }
      // ---- emit
      expand<true>(a, sh, cl, ncur, cc, prune, tau, row, K, tl, nullptr, 0u, nullptr, nullptr);
    }
    // ---- closure: round r expands the states whose key fell in round r - 1 (round 0: every state)
    __syncthreads();
    {
      const int *wl = tl;
      int wn = sh.cnt;
      for (int r = 0; r < a.g.eps_depth && wn > 0; r++) {
        int *wnext = works + (size_t)(r & 1) * S;
        expand<false>(a, sh, wl, wn, nullptr, false, 0, nullptr, K, tl, stamps, (u32)f * rounds + (u32)r + 1u, wnext,
                      &sh.wcnt[r & 1]);
        wn = sh.wcnt[r & 1];  // expand ended on a barrier
        wl = wnext;
        __syncthreads();
        if (tid == 0) sh.wcnt[r & 1] = 0;  // read again two rounds on, behind two barriers
      }
    }
    __syncthreads();
    // ---- append: records, the frame's best, rebased costs
    const int nn = sh.cnt;
    if (nn == 0) { failed = -1; break; }
    if ((long long)recs + nn > a.pool_tokens) { failed = -2; break; }
    int *rn = rec + (size_t)nb * S;
    const int *rc = rec + (size_t)cb * S;
    u32 mb = 0xFFFFFFFFu;
    for (int i = tid; i < nn; i += kThreads) {
      const int s = tl[i];
      rn[s] = recs + i;
      mb = min(mb, (u32)(key_load(K + s) >> 32));
    }
    atomicMin(&sh.best, mb);
    __syncthreads();
    const float best = fkey_inv(sh.best);
    float *cn = costs + (size_t)nb * S;
    for (int i = tid; i < nn; i += kThreads) {
      const int s = tl[i];
      const u64 k = key_load(K + s);
      const int arc = (int)(u32)k - 1;
      cn[i] = fkey_inv((u32)(k >> 32)) - best;
      int prev = -1;
      if (arc >= 0) {
        const int2 ar = a.g.arc[arc];
        prev = ar.y == 0 ? rn[ar.x] : rc[ar.x];
      }
      pool[recs + i] = make_int2(prev, arc);
    }
    // Q_{f-1} is spent: its keys are the empty buffer of frame f + 1
    {
      u64 *Kc = keys + (size_t)cb * S;
      const int *cl = lists + (size_t)cb * S;
      for (int i = tid; i < ncur; i += kThreads) key_store(Kc + cl[i], kEmpty);
    }
    if (tid == 0) fbase[f] = recs;
    off += (double)best;
    recs += nn;
    ncur = nn;
    __syncthreads();
    if (tid == 0) {
      sh.cnt = 0;
      sh.nb = 0;
      sh.best = 0xFFFFFFFFu;
    }
    __syncthreads();
  }

  Fin *fin = reinterpret_cast<Fin *>(a.ws + a.o_fin);
  if (failed) {  // workgroup-uniform
    if (tid == 0) {
      fin[n] = Fin{-1, T, expanded, recs};
      a.status[n] = failed;
      a.scores[n] = INFINITY;
      a.words_len[n] = 0;
    }
    return;
  }
  if (tid == 0) fbase[T + 1] = recs;
  // ---- the winner among Q_T: (cost + final cost, state), else (cost, state)
  const int b = T & 1;
  const float *cc = costs + (size_t)b * S;
  const int *cl = lists + (size_t)b * S;
  for (int i = tid; i < ncur; i += kThreads) {
    const int s = cl[i];
    const float fc = a.g.fin[s];
    atomicMin(&sh.win_any, ((u64)fkey(cc[i]) << 32) | (u32)s);
    if (fc < INFINITY) atomicMin(&sh.win_final, ((u64)fkey(cc[i] + fc) << 32) | (u32)s);
  }
  __syncthreads();
  if (tid == 0) {
    const bool final_reached = sh.win_final != kEmpty;
    const u64 w = final_reached ? sh.win_final : sh.win_any;
    const int s = (int)(u32)w;
    fin[n] = Fin{rec[(size_t)b * S + s], T, expanded, recs};
    a.status[n] = final_reached ? 1 : 0;
    a.scores[n] = off + (double)fkey_inv((u32)(w >> 32));
  }
}

// ---------------------------------------------------------------------------
// K2.  Record v = (previous record, arc id); the records of frame f are
// [fbase[f], fbase[f + 1]).  An emitting arc's previous record lies in the
// frame before, an epsilon arc's in the same frame.  Windows of whole frames
// (as many as fit kBtWin records, from the walker's frame down) are staged by
// the workgroup; one lane chases the chain, reading a record outside the
// window (a frame with more than kBtWin tokens) in place.
// ---------------------------------------------------------------------------
struct BtArgs {
  DevGraph g;
  int N, max_T;
  long long row;  // ints per row of words: max_T + words_slack
  long long pool_tokens;
  char *ws;
  size_t o_fin, o_base, per, o_fbase, o_pool;
  int *words, *words_len, *ali;
};

__global__ __launch_bounds__(kThreads) void wfst_backtrace(BtArgs a) {
  __shared__ int2 win[kBtWin];
  __shared__ int s_v, s_f, s_pos;
  const int n = blockIdx.x, tid = threadIdx.x;
  const Fin fin = reinterpret_cast<const Fin *>(a.ws + a.o_fin)[n];
  const char *base = a.ws + a.o_base + a.per * n;
  const int *fbase = reinterpret_cast<const int *>(base + a.o_fbase);
  const int2 *pool = reinterpret_cast<const int2 *>(base + a.o_pool);
  int *out = a.words + a.row * n;
  const int T = fin.T;
  for (int t = tid; t < a.max_T; t += kThreads)
    if (t >= T || fin.rec < 0) a.ali[(size_t)t * a.N + n] = -1;
  int v = fin.rec, f = T;
  long long pos = a.row;       // words are written from the end of the row down (lane 0's copy counts)
  long long hops = a.row + 1;  // a path has at most `row` arcs (lane 0's copy counts)
  __syncthreads();
  while (v >= 0) {
    // frames [flo, f] in the window, flo the lowest with at most kBtWin records
    const int hi = fbase[f + 1];
    int flo = f;
    {
      int l = 0, r = f;  // the lowest frame whose base is >= hi - kBtWin
      while (l < r) {
        const int m = (l + r) >> 1;
        if (fbase[m] >= hi - kBtWin) r = m; else l = m + 1;
      }
      flo = l;
    }
    const int lo = max(fbase[flo], hi - kBtWin);  // frame f alone may be larger: its tail
    const int cnt = hi - lo;
    for (int i = tid; i < cnt; i += kThreads) win[i] = pool[lo + i];
    __syncthreads();
    if (tid == 0) {
      while (v >= 0 && f >= flo && hops > 0) {
        if (v >= a.pool_tokens) { v = -1; break; }  // never: records are below the pool's end
        const int2 r = (v >= lo && v < hi) ? win[v - lo] : pool[v];
        hops--;
        if (r.y >= 0) {
          const int il = a.g.arc[r.y].y, ol = a.g.olabel[r.y];
          if (ol != 0 && pos > 0) out[--pos] = ol;
          if (il != 0) {
            f--;
            if (f >= 0 && f < T) a.ali[(size_t)f * a.N + n] = il;
          }
        }
        v = r.x;
        if (f < 0) v = -1;
      }
      if (hops <= 0) v = -1;
      s_v = v; s_f = f; s_pos = (int)min(pos, (long long)INT_MAX);
    }
    __syncthreads();
    v = s_v;
    f = s_f;
    __syncthreads();  // win and s_* are rewritten by the next window
  }
  if (tid == 0) s_pos = (int)min(pos, (long long)INT_MAX);
  __syncthreads();
  pos = s_pos;
  const long long len = fin.rec < 0 ? 0 : a.row - pos;
  // move the words to the front: a chunk is read by every lane before any lane writes it
  if (pos > 0) {
    for (long long c = 0; c < len; c += kThreads) {
      const long long i = c + tid;
      const int x = i < len ? out[pos + i] : 0;
      __syncthreads();
      if (i < len) out[i] = x;
      __syncthreads();
    }
  }
  for (long long i = len + tid; i < a.row; i += kThreads) out[i] = -1;
  if (tid == 0) a.words_len[n] = (int)len;
}

// ---- launch ----------------------------------------------------------------------
int decode_launch(Graph *g, const float *ll, const std::vector<Utt> &utts_in, const Layout &lay, int A, int N,
                  float acoustic_scale, float beam, int max_active, long pool_tokens, int *words, int *words_len,
                  int *ali, double *scores, int *status, void *workspace, hipStream_t stream) {
  const DevGraph &dg = device_graph(g);
  char *stage = ctcimpl::staging_acquire(lay.fin);
  if (!stage) return 1;
  memcpy(stage + lay.utt, utts_in.data(), sizeof(Utt) * N);
  if (hipMemcpyAsync(workspace, stage, lay.fin, hipMemcpyHostToDevice, stream) != hipSuccess) return 1;
  ctcimpl::staging_release(stream);
  SearchArgs sa;
  sa.g = dg;
  sa.ll = ll;
  sa.A = A;
  sa.row_in_lds = A <= kRowLdsMax ? 1 : 0;
  sa.scale = acoustic_scale;
  sa.beam = beam;
  sa.max_active = max_active;
  sa.state_bits = 1;
  while (sa.state_bits < 32 && ((long long)1 << sa.state_bits) < g->num_states) sa.state_bits++;
  sa.pool_tokens = pool_tokens;
  sa.ws = static_cast<char *>(workspace);
  sa.o_utt = lay.utt; sa.o_fin = lay.fin; sa.o_base = lay.base; sa.per = lay.per;
  sa.o_keys = lay.keys; sa.o_rec = lay.rec; sa.o_stamp = lay.stamp; sa.o_list = lay.list;
  sa.o_cost = lay.cost; sa.o_work = lay.work; sa.o_fbase = lay.fbase; sa.o_pool = lay.pool;
  sa.words_len = words_len;
  sa.scores = scores;
  sa.status = status;
  const size_t shm = sa.row_in_lds ? sizeof(float) * (size_t)A : 0;
  {
    ProfSpan ps(stream, "wfst_search");
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(wfst_search), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)shm) != hipSuccess) {
      kctc_set_error("wfst_search: the device refuses the dynamic LDS of a log-likelihood row");
      return 3;
    }
    hipLaunchKernelGGL(wfst_search, dim3(N), dim3(kThreads), shm, stream, sa);
  }
  BtArgs ba;
  ba.g = dg;
  ba.N = N;
  ba.max_T = lay.max_T;
  ba.row = (long long)lay.max_T + words_slack(g->eps_depth, lay.max_T);
  ba.pool_tokens = pool_tokens;
  ba.ws = sa.ws;
  ba.o_fin = lay.fin; ba.o_base = lay.base; ba.per = lay.per;
  ba.o_fbase = lay.fbase; ba.o_pool = lay.pool;
  ba.words = words;
  ba.words_len = words_len;
  ba.ali = ali;
  {
    ProfSpan ps(stream, "wfst_backtrace");
    hipLaunchKernelGGL(wfst_backtrace, dim3(N), dim3(kThreads), 0, stream, ba);
  }
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

// Checks a decode call's arguments; 0 or CTC_STATUS_INVALID_VALUE's number (2).
static int check_decode(const Graph *g, const void *ll, const int *lens, int A, int N, float beam, int max_active,
                        long pool_tokens, Layout *lay, std::vector<Utt> *utts) {
  if (!g || !ll || A < 1 || !(beam > 0.f)) return 2;
  if (g->max_col >= A) return 2;
  if (!make_layout(*g, lens, N, max_active, pool_tokens, lay, utts)) return 2;
  if ((long long)lay->max_T + words_slack(g->eps_depth, lay->max_T) > INT_MAX - 2) return 2;
  return 0;
}

int decode_strided(Graph *g, const float *ll, const int *lens, const long long *ll_off, const long long *ll_stride,
                   int A, int N, float acoustic_scale, float beam, int max_active, long pool_tokens, int *words,
                   int *words_len, int *ali, double *scores, int *status, void *workspace, hipStream_t stream) {
  Layout lay;
  std::vector<Utt> utts;
  if (!words || !words_len || !ali || !scores || !status || !workspace || !std::isfinite(acoustic_scale)) return 2;
  const int st = check_decode(g, ll, lens, A, N, beam, max_active, pool_tokens, &lay, &utts);
  if (st) return st;
  for (int n = 0; n < N; n++) {
    utts[n].ll_off = ll_off[n];
    utts[n].ll_stride = ll_stride[n];
  }
  return decode_launch(g, ll, utts, lay, A, N, acoustic_scale, beam, max_active, pool_tokens, words, words_len, ali,
                       scores, status, workspace, stream);
}

size_t decode_workspace_bytes(const Graph *g, const int *lens, int N, int max_active, long pool_tokens) {
  Layout lay;
  if (!g || !make_layout(*g, lens, N, max_active, pool_tokens, &lay, nullptr)) return 0;
  return lay.total;
}

}  // namespace wfst
}  // namespace kctc

extern "C" {

int kctc_wfst_decode_workspace_size(kctcGraph_t graph, const int *input_lengths, int minibatch, int max_active,
                                    long pool_tokens, size_t *size_bytes) {
  if (!size_bytes || !graph) return 2;
  try {
    const size_t b = kctc::wfst::decode_workspace_bytes(graph, input_lengths, minibatch, max_active, pool_tokens);
    if (!b) return 2;
    *size_bytes = b;
    return 0;
  } catch (...) {
    return 4;
  }
}

int kctc_wfst_decode_counts(const void *workspace, int minibatch, struct ihipStream_t *stream, long *expanded,
                            long *held) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(workspace && minibatch >= 1 && expanded && held, "kctc_wfst_decode_counts: bad argument");
    using kctc::wfst::Fin;
    std::vector<Fin> fin((size_t)minibatch);
    const size_t at = kctc::wfst::fin_offset(minibatch);
    KCTC_HIP_CHECK(hipMemcpyAsync(fin.data(), static_cast<const char *>(workspace) + at, sizeof(Fin) * minibatch,
                                  hipMemcpyDeviceToHost, stream));
    KCTC_HIP_CHECK(hipStreamSynchronize(stream));
    for (int n = 0; n < minibatch; n++) {
      expanded[n] = fin[n].expanded;
      held[n] = fin[n].held;
    }
  });
}

int kctc_wfst_decode_async(kctcGraph_t graph, const float *loglikes, const int *input_lengths, int num_columns,
                           int minibatch, float acoustic_scale, float beam, int max_active, long pool_tokens,
                           int *words_dev, int *words_len_dev, int *ali_dev, double *scores_dev, int *status_dev,
                           void *workspace, struct ihipStream_t *stream) {
  try {
    if (minibatch < 1 || !input_lengths) return 2;
    std::vector<long long> off((size_t)minibatch), stride((size_t)minibatch, (long long)minibatch * num_columns);
    for (int n = 0; n < minibatch; n++) off[n] = (long long)n * num_columns;  // time-major rows
    return kctc::wfst::decode_strided(graph, loglikes, input_lengths, off.data(), stride.data(), num_columns,
                                      minibatch, acoustic_scale, beam, max_active, pool_tokens, words_dev,
                                      words_len_dev, ali_dev, scores_dev, status_dev, workspace, stream);
  } catch (const std::exception &e) {
    kctc_set_error(e.what());
    return 4;
  } catch (...) {
    return 4;
  }
}

}  // extern "C"
