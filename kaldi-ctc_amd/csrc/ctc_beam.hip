// ctc_beam.hip -- lexicon-free CTC prefix beam search for MI355X (gfx950): the
// most likely transcript of each utterance among the prefixes a beam keeps
// (include/ctc.h, extensions).
//
// Three launches per call, all stream-ordered:
//   K1 ctc_logz            ctc.hip's per-frame normaliser: lp = act - logsumexp(act).
//   K2 ctc_beam_search     one workgroup of 4 waves per utterance, serial over
//                          T.  lp rows come into LDS a chunk of 32 frames
//                          ahead by LDS-DMA; at the head of a chunk every wave
//                          ranks rows of it (the K best non-blank symbols of a
//                          frame and the rank of every symbol).  A frame is
//                            merge   thread q looks the hash of q's parent
//                                    prefix up among the beam's hashes: if the
//                                    parent p is in the beam, the extension
//                                    p + last(q) is q itself, so its mass goes
//                                    to q's stay candidate and the extension
//                                    candidate is struck out;
//                            score   candidate i (K+1) + j is beam entry i
//                                    staying (j = 0) or extended by the j-th
//                                    best symbol, R candidates per thread in
//                                    registers, fp32 relative to the running
//                                    fp64 offset;
//                            select  the beam-th largest total by a radix
//                                    search over the order-preserving integer
//                                    image of the fp32 totals, 2 bits a step,
//                                    counted with ballots (no atomics);
//                            write   survivors take their slots in (wave,
//                                    register, lane) order, ties at the
//                                    threshold in that order too; an extension
//                                    that survives gets node 1 + t beam + slot
//                                    of the utterance's node pool.
//   K3 ctc_beam_backtrace  one workgroup per utterance walks the winner's
//                          parent chain through LDS windows of 2048 pool nodes
//                          and writes the labels front to back, -1 behind them.
// Deterministic: no atomics, a fixed order everywhere.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "common.h"
#include "ctc.h"
#include "ctc_shared.h"
#include "prof.h"

namespace kctc {
namespace ctcimpl {

constexpr int kBeamThreads = 256;
constexpr int kBeamWaves = kBeamThreads / 64;
constexpr int kBeamMax = 128;   // beam entries
constexpr int kBeamSymMax = 64; // symbols a frame extends by: one wave's lanes
constexpr int kBeamF = 32;      // frames per emission chunk
constexpr int kBeamRMax = (kBeamMax * (kBeamSymMax + 1) + kBeamThreads - 1) / kBeamThreads;  // 33
constexpr int kBtWin = 2048;    // pool nodes per backtrace window
constexpr int kBtBeamThreads = 256;

typedef unsigned long long u64;
typedef unsigned int u32;

struct BeamLayout {
  size_t desc, fin, logz, lp, pool, total;
  int T_max;
};

// Checks the arguments the workspace depends on and lays it out; false: invalid.
static bool make_beam_layout(const int *input_lengths, int A, int N, int beam, BeamLayout *lay,
                             std::vector<UttDesc> *descs) {
  if (A < 2 || N <= 0 || !input_lengths || beam < 1 || beam > kBeamMax) return false;
  int T_max = 0;
  long long nodes = 0;
  if (descs) descs->resize(N);
  for (int n = 0; n < N; n++) {
    const int T = input_lengths[n];
    if (T < 0 || (long long)T * beam > INT_MAX - 2) return false;  // node ids are ints
    T_max = std::max(T_max, T);
    if (descs) {
      UttDesc &d = (*descs)[n];
      d.T = T; d.L = 0; d.S = 0; d.feasible = 1; d.lab_off = 0; d.pad = 0;
      d.ab_off = nodes;  // this utterance's first pool node
      d.off_off = 0;
    }
    nodes += (long long)T * beam;  // at most `beam` new prefixes a frame
  }
  BeamLayout &l = *lay;
  size_t p = 0;
  l.desc = p; p = align_up(p + sizeof(UttDesc) * N, 256);
  l.fin = p;  p = align_up(p + sizeof(int2) * N, 256);  // winner of each utterance: (node, length)
  l.logz = p; p = align_up(p + sizeof(float) * (size_t)T_max * N + 4, 256);
  l.lp = p;   p = align_up(p + sizeof(float) * (size_t)T_max * N * A + 4, 256);
  l.pool = p; p = align_up(p + sizeof(int4) * (size_t)(nodes > 0 ? nodes : 1), 256);
  l.total = p;
  l.T_max = T_max;
  return true;
}

// dynamic LDS of K2, in bytes from the base (every array 16-byte aligned)
struct BeamLds {
  int F, AP, B, K;
  size_t emit, sym, h, ph, fb, fnb, last, node, len, extra, red, rank, kill, total;
  void lay() {
    size_t p = 0;
    auto take = [&](size_t bytes) { const size_t at = p; p = align_up(p + bytes, 16); return at; };
    emit = take(sizeof(float) * 2 * F * AP);    // [2][F][AP] lp rows
    sym = take(sizeof(int) * F * kBeamSymMax);  // [F][64] the K best symbols of a frame, best first
    h = take(sizeof(u64) * 2 * B);              // beam, double-buffered: prefix hash
    ph = take(sizeof(u64) * 2 * B);             //   hash of the prefix without its last label
    fb = take(sizeof(float) * 2 * B);           //   log-prob ending in blank, relative to the offset
    fnb = take(sizeof(float) * 2 * B);          //   ... ending in a label
    last = take(sizeof(int) * 2 * B);           //   last label (-1: the empty prefix)
    node = take(sizeof(int) * 2 * B);           //   pool node (0: the empty prefix)
    len = take(sizeof(int) * 2 * B);            //   labels
    extra = take(sizeof(float) * B);            // mass merged into entry q's stay candidate
    red = take(sizeof(int) * 64);               // the waves' partial counts and maxima
    rank = take((size_t)F * AP);                // [F][AP] bytes: rank of a symbol in its frame (255: not among the K)
    kill = take((size_t)B * (K + 1));           // [B][K+1] bytes: candidate merged away this frame
    total = p;
  }
};

__device__ __forceinline__ float logadd(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return m;
  return m + __logf(1.0f + __expf(fminf(a, b) - m));
}

// h(p + c): one splitmix64 round over the parent's hash and the symbol
__device__ __forceinline__ u64 hash_mix(u64 h, int c) {
  u64 x = h + 0x9E3779B97F4A7C15ull * (u64)(c + 1);
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
constexpr u64 kRootHash = 0x243F6A8885A308D3ull;

// order-preserving image of a finite float or -inf in [1, 2^32); 0 is kept for "no candidate"
__device__ __forceinline__ u32 float_key(float x) {
  const u32 u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int popc64(u64 m) { return __builtin_popcountll(m); }
__device__ __forceinline__ int lanes_below(u64 m) {
  return (int)__builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
}

// ---------------------------------------------------------------------------
// K2.  R: candidates per thread, R * 256 >= beam * (K + 1).
// ---------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(kBeamThreads) void ctc_beam_search(
    const float *__restrict__ lp, int N, int A, int blank, const UttDesc *__restrict__ descs,
    int4 *__restrict__ pool, int2 *__restrict__ fin, int *__restrict__ hyp_len, double *__restrict__ scores,
    BeamLds L) {
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  char *base = reinterpret_cast<char *>(lds);
  const int F = L.F, AP = L.AP, B = L.B, K = L.K, K1 = K + 1;
  float *emit = lds;  // L.emit == 0
  int *sym = reinterpret_cast<int *>(base + L.sym);
  u64 *bh = reinterpret_cast<u64 *>(base + L.h);
  u64 *bph = reinterpret_cast<u64 *>(base + L.ph);
  float *bfb = reinterpret_cast<float *>(base + L.fb);
  float *bfnb = reinterpret_cast<float *>(base + L.fnb);
  int *blast = reinterpret_cast<int *>(base + L.last);
  int *bnode = reinterpret_cast<int *>(base + L.node);
  int *blen = reinterpret_cast<int *>(base + L.len);
  float *extra = reinterpret_cast<float *>(base + L.extra);
  int *red = reinterpret_cast<int *>(base + L.red);
  // red: [0, 24) the radix search's counts [2][kBeamWaves][3]; [24, 28) wave maxima; [28, 32) live
  // counts; [32, 40) the waves' (above, at) the threshold
  float *wmax = reinterpret_cast<float *>(red + 24);
  int *wlive = red + 28, *wtot = red + 32;
  unsigned char *rk = reinterpret_cast<unsigned char *>(base + L.rank);
  unsigned char *kill = reinterpret_cast<unsigned char *>(base + L.kill);

  const UttDesc d = descs[n];
  const int T = d.T;
  int4 *poolu = pool + d.ab_off;  // node id v lives at poolu[v - 1]

  // candidate e = r * 256 + tid is beam entry e / (K+1), slot e % (K+1)
  int ci[R], cj[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int e = r * kBeamThreads + tid;
    ci[r] = e / K1;
    cj[r] = e - ci[r] * K1;
  }

  for (int i = tid; i < B * K1; i += kBeamThreads) kill[i] = 0;
  if (tid == 0) {
    bh[0] = kRootHash; bph[0] = 0;
    bfb[0] = 0.f; bfnb[0] = -INFINITY;
    blast[0] = -1; bnode[0] = 0; blen[0] = 0;
  }

  const long tstride = (long)N * A;
  const float *lrow = lp + (long)n * A;  // + t * N * A
  const int nblk = AP >> 6;
  auto issue = [&](int c, int b) {
    float *dst = emit + (size_t)b * F * AP;
    const int fend = min(F, T - c * F);
    for (int p = wid; p < fend * nblk; p += kBeamWaves) {
      const int f = p / nblk, sb = p - f * nblk;
      const float *src = lrow + (long)(c * F + f) * tstride;
      __builtin_amdgcn_global_load_lds(src + min(sb * 64 + lane, A - 1), dst + (size_t)f * AP + sb * 64, 4, 0, 0);
    }
  };

  const int nchunk = (T + F - 1) / F;
  if (nchunk > 0) issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();
  double off = 0.0;
  int cur = 0, nbeam = 1;
  for (int c = 0; c < nchunk; c++) {
    if (c + 1 < nchunk) issue(c + 1, (c + 1) & 1);
    const float *em = emit + (size_t)(c & 1) * F * AP;
    const int fend = min(F, T - c * F);

    // the chunk's symbol sets: wave w ranks rows w, w + 4, ...; lane owns symbols lane + 64 k.
    // rank = how many non-blank symbols beat it (larger lp, or equal lp and lower id)
    for (int f = wid; f < fend; f += kBeamWaves) {
      const float *row = em + (size_t)f * AP;
      for (int s0 = 0; s0 < A; s0 += 64) {
        const int s = s0 + lane;
        const float v = row[min(s, A - 1)];
        int rank = 0;
        for (int a = 0; a < A; a++) {
          const float u = row[a];
          rank += (a != blank && (u > v || (u == v && a < s))) ? 1 : 0;
        }
        if (s < A) {
          const bool in = s != blank && rank < K;
          rk[(size_t)f * AP + s] = in ? (unsigned char)rank : (unsigned char)255;
          if (in) sym[f * kBeamSymMax + rank] = s;
        }
      }
    }
    lds_barrier();

    for (int f = 0; f < fend; f++) {
      const int t = c * F + f;
      const float *row = em + (size_t)f * AP;
      const u64 *h = bh + cur * B;
      const float *fb = bfb + cur * B, *fnb = bfnb + cur * B;
      const int *last = blast + cur * B, *len = blen + cur * B, *node = bnode + cur * B;

      // ---- merge: is the parent of q in the beam?  then q is also parent + last(q)
      if (tid < nbeam) {
        const int q = tid;
        float ex = -INFINITY;
        if (len[q] > 0) {
          const u64 want = bph[cur * B + q];
          int par = -1;
          for (int i = 0; i < nbeam; i++) par = (par < 0 && h[i] == want) ? i : par;
          if (par >= 0) {
            const int cq = last[q];
            const int r = rk[(size_t)f * AP + cq];
            if (r != 255) {
              kill[par * K1 + 1 + r] = 1;
              ex = row[cq] + (cq == last[par] ? fb[par] : logadd(fb[par], fnb[par]));
            }
          }
        }
        extra[q] = ex;
      }
      lds_barrier();

      // ---- score
      const float lpb = row[blank];
      u32 key[R];
      float cb[R], cnb[R];
      float lmax = -INFINITY;
      int nlive_w = 0;
#pragma unroll
      for (int r = 0; r < R; r++) {
        key[r] = 0;
        cb[r] = -INFINITY;
        cnb[r] = -INFINITY;
        if (r * kBeamThreads < nbeam * K1) {  // workgroup-uniform
          const int i = ci[r];
          if (i < nbeam) {
            const float b = fb[i], nbv = fnb[i], tot = logadd(b, nbv);
            const int e = last[i];
            if (cj[r] == 0) {
              cb[r] = lpb + tot;
              cnb[r] = logadd(e >= 0 ? row[e] + nbv : -INFINITY, extra[i]);
            } else {
              const int s = sym[f * kBeamSymMax + cj[r] - 1];
              const int at = i * K1 + cj[r];
              if (kill[at]) kill[at] = 0;  // merged into the entry it equals; the flag is this thread's to clear
              else cnb[r] = row[s] + (s == e ? b : tot);
            }
            const float tt = logadd(cb[r], cnb[r]);
            if (tt > -INFINITY) key[r] = float_key(tt);
            lmax = fmaxf(lmax, tt);
          }
          nlive_w += popc64(__builtin_amdgcn_ballot_w64(key[r] != 0));
        }
      }
      lmax = wave_max_l63(lmax);
      if (lane == 63) wmax[wid] = lmax;
      if (lane == 0) wlive[wid] = nlive_w;
      lds_barrier();
      float M = wmax[0];
      int nlive = wlive[0];
#pragma unroll
      for (int w = 1; w < kBeamWaves; w++) {
        M = fmaxf(M, wmax[w]);
        nlive += wlive[w];
      }

      // ---- select: tau = the B-th largest key (0: every live candidate stays)
      u32 tau = 0;
      if (nlive > B) {  // workgroup-uniform
        int par = 0;
        for (int sh = 30; sh >= 0; sh -= 2) {
          const u32 t1 = tau | (1u << sh), t2 = tau | (2u << sh), t3 = tau | (3u << sh);
          int c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
          for (int r = 0; r < R; r++) {
            if (r * kBeamThreads < nbeam * K1) {
              c1 += popc64(__builtin_amdgcn_ballot_w64(key[r] >= t1));
              c2 += popc64(__builtin_amdgcn_ballot_w64(key[r] >= t2));
              c3 += popc64(__builtin_amdgcn_ballot_w64(key[r] >= t3));
            }
          }
          int *wc = red + par * 3 * kBeamWaves;
          if (lane == 0) {
            wc[wid * 3 + 0] = c1;
            wc[wid * 3 + 1] = c2;
            wc[wid * 3 + 2] = c3;
          }
          lds_barrier();
          c1 = c2 = c3 = 0;
#pragma unroll
          for (int w = 0; w < kBeamWaves; w++) {
            c1 += wc[w * 3 + 0];
            c2 += wc[w * 3 + 1];
            c3 += wc[w * 3 + 2];
          }
          tau = c3 >= B ? t3 : c2 >= B ? t2 : c1 >= B ? t1 : tau;
          par ^= 1;  // the next step writes the other half: one barrier a step is enough
        }
      }

      // ---- write: slots in (wave, register, lane) order; above the threshold first, then ties
      int gw = 0, ew = 0;
#pragma unroll
      for (int r = 0; r < R; r++) {
        if (r * kBeamThreads < nbeam * K1) {
          gw += popc64(__builtin_amdgcn_ballot_w64(key[r] > tau));
          ew += popc64(__builtin_amdgcn_ballot_w64(tau != 0 && key[r] == tau));
        }
      }
      if (lane == 0) {
        wtot[wid * 2] = gw;
        wtot[wid * 2 + 1] = ew;
      }
      lds_barrier();
      int gpos = 0, epos = 0, G = 0;
#pragma unroll
      for (int w = 0; w < kBeamWaves; w++) {
        const int g = wtot[w * 2], e = wtot[w * 2 + 1];
        gpos += w < wid ? g : 0;
        epos += w < wid ? e : 0;
        G += g;
      }
      const int need = B - G;  // ties that still fit (only read when tau != 0)
      const int nx = cur ^ 1;
#pragma unroll
      for (int r = 0; r < R; r++) {
        if (r * kBeamThreads < nbeam * K1) {
          const bool gt = key[r] > tau, eq = tau != 0 && key[r] == tau;
          const u64 mg = __builtin_amdgcn_ballot_w64(gt), me = __builtin_amdgcn_ballot_w64(eq);
          int slot = -1;
          if (gt) slot = gpos + lanes_below(mg);
          else if (eq && epos + lanes_below(me) < need) slot = G + epos + lanes_below(me);
          gpos += popc64(mg);
          epos += popc64(me);
          if (slot >= 0 && slot < B) {
            const int i = ci[r], o = nx * B + slot;
            bfb[o] = cb[r] - M;
            bfnb[o] = cnb[r] - M;
            if (cj[r] == 0) {
              bh[o] = h[i];
              bph[o] = bph[cur * B + i];
              blast[o] = last[i];
              bnode[o] = node[i];
              blen[o] = len[i];
            } else {
              const int s = sym[f * kBeamSymMax + cj[r] - 1];
              const int v = 1 + t * B + slot;  // a new prefix: the node of this frame and slot
              bh[o] = hash_mix(h[i], s);
              bph[o] = h[i];
              blast[o] = s;
              bnode[o] = v;
              blen[o] = len[i] + 1;
              poolu[v - 1] = make_int4(node[i], s, len[i] + 1, 0);
            }
          }
        }
      }
      off += (double)M;
      nbeam = min(B, nlive);
      cur = nx;
      lds_barrier();
    }
    // the next chunk's rows have landed; every wave is done with this chunk's buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
  }
  if (tid == 0) {
    // the most likely prefix; the earlier slot on a tie
    int best = 0;
    float bt = -INFINITY;
    for (int i = 0; i < nbeam; i++) {
      const float tt = logadd(bfb[cur * B + i], bfnb[cur * B + i]);
      if (tt > bt) { bt = tt; best = i; }
    }
    // nbeam == 0: a frame without a finite log-prob (NaN or inf activations) left nothing alive
    fin[n] = nbeam ? make_int2(bnode[cur * B + best], blen[cur * B + best]) : make_int2(0, 0);
    hyp_len[n] = nbeam ? blen[cur * B + best] : 0;
    scores[n] = nbeam ? off + (double)bt : -INFINITY;
  }
}

// ---------------------------------------------------------------------------
// K3: node v = (parent, symbol, length) sits at pool[v - 1] and was made in
// frame (v - 1) / B; a parent is older than its child.  Windows of kBtWin
// nodes, from the winner's frame down, are staged by the workgroup; one lane
// chases the chain inside the window and writes label `length - 1`.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBtBeamThreads) void ctc_beam_backtrace(
    const UttDesc *__restrict__ descs, const int4 *__restrict__ pool, const int2 *__restrict__ fin, int maxT, int B,
    int *__restrict__ hyp) {
  __shared__ int4 win[kBtWin];
  __shared__ int s_node;
  const int n = blockIdx.x, tid = threadIdx.x;
  const UttDesc d = descs[n];
  const int4 *poolu = pool + d.ab_off;
  int node = fin[n].x;
  if (node > d.T * B) node = 0;  // never: the pool has T * B nodes
  const int len = min(fin[n].y, maxT);
  int *out = hyp + (long)n * maxT;
  for (int p = len + tid; p < maxT; p += kBtBeamThreads) out[p] = -1;
  const int W = kBtWin / B;  // frames per window (>= 16)
  while (node > 0) {
    const int fhi = (node - 1) / B, flo = max(fhi - W + 1, 0);
    const int lo = flo * B, cnt = (fhi + 1) * B - lo;  // pool entries [lo, lo + cnt), cnt <= kBtWin
    for (int it = tid; it < cnt; it += kBtBeamThreads) win[it] = poolu[lo + it];
    __syncthreads();
    if (tid == 0) {
      int v = node;
      while (v > lo) {
        const int4 nd = win[v - 1 - lo];
        const int pos = nd.z - 1;
        if (pos >= 0 && pos < len) out[pos] = nd.y;
        v = (nd.x >= 0 && nd.x < v) ? nd.x : 0;  // a parent is older than its child
      }
      s_node = v;
    }
    __syncthreads();
    node = s_node;
    __syncthreads();  // win and s_node are rewritten by the next window
  }
}

template <int R>
static void launch_search(int N, size_t shm, hipStream_t stream, const float *lp, int A, int blank,
                          const UttDesc *descs, int4 *pool, int2 *fin, int *hyp_len, double *scores,
                          const BeamLds &L) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ctc_beam_search<R>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  hipLaunchKernelGGL(ctc_beam_search<R>, dim3(N), dim3(kBeamThreads), shm, stream, lp, N, A, blank, descs, pool, fin,
                     hyp_len, scores, L);
}

static ctcStatus_t launch_beam(const BeamLayout &lay, const std::vector<UttDesc> &descs, const float *acts, int A,
                               int N, int beam, int symbols, int *hyp_dev, int *hyp_len_dev, double *scores_dev,
                               void *workspace, hipStream_t stream, int blank) {
  if (blank < 0 || blank >= A || symbols < 1 || symbols > kBeamSymMax || !acts || !workspace || !hyp_dev ||
      !hyp_len_dev || !scores_dev)
    return CTC_STATUS_INVALID_VALUE;
  BeamLds L;
  L.B = beam;
  L.K = std::min(symbols, A - 1);
  L.AP = (A + 63) / 64 * 64;
  // chunk depth: as many frames as fit 64 KB of double-buffered rows (1..32)
  L.F = (int)std::min<size_t>(kBeamF, std::max<size_t>(1, (size_t)64 * 1024 / (2 * sizeof(float) * L.AP)));
  L.lay();
  if (L.total > 160 * 1024) return CTC_STATUS_INVALID_VALUE;
  char *ws = static_cast<char *>(workspace);
  char *stage = staging_acquire(lay.fin);
  if (!stage) return CTC_STATUS_MEMOPS_FAILED;
  memcpy(stage + lay.desc, descs.data(), sizeof(UttDesc) * N);
  if (hipMemcpyAsync(ws, stage, lay.fin, hipMemcpyHostToDevice, stream) != hipSuccess)
    return CTC_STATUS_MEMOPS_FAILED;
  staging_release(stream);
  const UttDesc *d_desc = reinterpret_cast<const UttDesc *>(ws + lay.desc);
  int2 *d_fin = reinterpret_cast<int2 *>(ws + lay.fin);
  float *d_lp = reinterpret_cast<float *>(ws + lay.lp);
  int4 *d_pool = reinterpret_cast<int4 *>(ws + lay.pool);
  const long rows = (long)lay.T_max * N;
  if (rows > 0) launch_logz(acts, A, rows, reinterpret_cast<float *>(ws + lay.logz), d_lp, stream);
  {
    ProfSpan ps(stream, "ctc_beam_search");
    const int cands = beam * (L.K + 1);
    if (cands <= 3 * kBeamThreads)
      launch_search<3>(N, L.total, stream, d_lp, A, blank, d_desc, d_pool, d_fin, hyp_len_dev, scores_dev, L);
    else if (cands <= 11 * kBeamThreads)
      launch_search<11>(N, L.total, stream, d_lp, A, blank, d_desc, d_pool, d_fin, hyp_len_dev, scores_dev, L);
    else
      launch_search<kBeamRMax>(N, L.total, stream, d_lp, A, blank, d_desc, d_pool, d_fin, hyp_len_dev, scores_dev, L);
  }
  {
    ProfSpan ps(stream, "ctc_beam_backtrace");
    hipLaunchKernelGGL(ctc_beam_backtrace, dim3(N), dim3(kBtBeamThreads), 0, stream, d_desc, d_pool, d_fin,
                       lay.T_max, beam, hyp_dev);
  }
  if (hipGetLastError() != hipSuccess) return CTC_STATUS_EXECUTION_FAILED;
  return CTC_STATUS_SUCCESS;
}

}  // namespace ctcimpl
}  // namespace kctc

using namespace kctc::ctcimpl;

extern "C" {

ctcStatus_t mictc_get_beam_workspace_size(const int *input_lengths, int alphabet_size, int minibatch, int beam,
                                          size_t *size_bytes) {
  if (!size_bytes) return CTC_STATUS_INVALID_VALUE;
  BeamLayout lay;
  if (!make_beam_layout(input_lengths, alphabet_size, minibatch, beam, &lay, nullptr))
    return CTC_STATUS_INVALID_VALUE;
  *size_bytes = lay.total;
  return CTC_STATUS_SUCCESS;
}

ctcStatus_t mictc_ctc_beam_search_async(const float *activations, const int *input_lengths, int alphabet_size,
                                        int minibatch, int beam, int symbols, int *hyp_dev, int *hyp_len_dev,
                                        double *scores_dev, void *workspace, ctcStream_t stream, int blank_label) {
  try {
    BeamLayout lay;
    std::vector<UttDesc> descs;
    if (!make_beam_layout(input_lengths, alphabet_size, minibatch, beam, &lay, &descs))
      return CTC_STATUS_INVALID_VALUE;
    return launch_beam(lay, descs, activations, alphabet_size, minibatch, beam, symbols, hyp_dev, hyp_len_dev,
                       scores_dev, workspace, reinterpret_cast<hipStream_t>(stream), blank_label);
  } catch (...) {
    return CTC_STATUS_UNKNOWN_ERROR;
  }
}

}  // extern "C"
