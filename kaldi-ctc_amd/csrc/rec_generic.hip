// rec_generic.hip -- the generic recurrences (rnn_fwd_rec / rnn_bwd_rec: fp32
// MFMA, all-gather of h or dGates per step), for the shapes v6 does not
// compile.  Host: rnn.hip.
#include "rec_common.h"

namespace kctc {
namespace {

// ---------------------------------------------------------------------------
// generic recurrences: all-gather hand-off, fp32 MFMA
// ---------------------------------------------------------------------------
// Block mapping (block_of): with p.xpd > 0 the grid is 8 * ceil(nwg / xpd) and
// block b works in XCD slot b & 7 -- direction slot / xpd, workgroup
// (b >> 3) * xpd + slot % xpd -- so that under round-robin dispatch the
// workgroups of one direction share xpd XCDs and their L2; blocks past dirs or
// nwg exit at once.  p.xpd == 0 (no U gives a direction whole slots): grid
// dirs * nwg, block b -> (b / nwg, b % nwg).  The slots are a placement hint
// only: the hand-off is the placement-independent form throughout (sc1
// write-through payload and flag stores after every storing wave's vmcnt(0)
// and a barrier, sc1 loads: MI355X_MICROARCH.md "Valid forms", row 1).  A
// step is
//   wait for the direction's nwg epoch flags (one sc1 poll per lane, wave 0)
//   -> sc1 16-B loads of the previous step straight into MFMA A registers
//   -> v_mfma_f32_16x16x4_f32 over the LDS-resident R slice (K split over
//      the 4 waves, reduced through LDS)
//   -> pointwise cell math, one (n, unit) element per thread
//   -> payload stores -> vmcnt(0) -> barrier -> lane 0 epoch flag.
// Step k publishes epoch k + 2.
__device__ __forceinline__ bool block_of(const RecParams &p, int &d, int &g) {
  if (p.xpd > 0) {
    const int slot = blockIdx.x & 7;
    d = slot / p.xpd;
    g = (blockIdx.x >> 3) * p.xpd + slot % p.xpd;
  } else {
    d = blockIdx.x / p.nwg;
    g = blockIdx.x % p.nwg;
  }
  return d < p.dirs && g < p.nwg;
}

// Exchange image of one step, fragment-major: [dirs][KG][Npad][16] floats
// (KG = 16-wide k-groups).  One MFMA A fragment (16 rows x 16 k) is 1 KB of
// contiguous memory, so every hand-off load instruction moves whole 128-B
// lines; producers write 16 consecutive units of a row as 64 contiguous bytes.
// The row-major copies the rest of the layer needs (y, E) are written with
// plain stores off the critical path.
__device__ __forceinline__ long xoff(int d, int kg, int n, int j, int KG, int Npad) {
  return (((long)d * KG + kg) * Npad + n) * 16 + j;
}

// Hand-off loads + MFMA body of one step with compile-time trip counts: all
// loads first, then the MFMAs consume them in issue order, so the in-order
// vmcnt lets the first k-groups compute while the rest are in flight.
// Forward: acc[RT][CT] += h_{t-1}[rows][k] * R_slice^T[k][cols], K split over
// the 4 waves (wave w: k-groups w, w+4, ...).
template <int RT, int CT, int KGW>
__device__ __forceinline__ void fwd_step_mfma(floatx4 (&acc)[RT][kMaxCT], __amdgpu_buffer_rsrc_t rs, long dbase,
                                              int Npad, const float *Rs, int LDR, int w, int fr, int fq) {
  u32x4 af[KGW][RT];
#pragma unroll
  for (int i = 0; i < KGW; i++)
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
      af[i][rt] = ld_sc1(rs, (unsigned)((dbase + ((long)(w + 4 * i) * Npad + rt * 16 + fr) * 16 + fq * 4) * 4));
#pragma unroll
  for (int i = 0; i < KGW; i++) {
    const int kg = w + 4 * i;
    floatx4 b[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ct++) b[ct] = ld4(Rs + (ct * 16 + fr) * LDR + kg * 16 + fq * 4);
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
      for (int ct = 0; ct < CT; ct++)
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[i][rt][s]), b[ct][s], acc[rt][ct],
                                                             0, 0, 0);
  }
}

// Backward: acc[RT] = dG_{t+1}[rows][kk] * R^T_slice[kk][units] over all nW*H
// kk (wave w: k-groups w, w+4, ...); NA accumulator sets interleaved so no
// MFMA waits on its predecessor, summed in a fixed order.  RT_s holds U rows:
// a lane's B fragment comes from row br = fr, or row 0 for a lane past them
// (fr >= U).  Output column fr of the MFMA depends on B column fr alone, and
// the cell reads the columns below U only, so what such a lane multiplies
// never reaches a result; it only has to lie inside the image.  (Zeroing it,
// by a branch or a select per load, measured 3 to 11 % slower on LSTM-384.)
template <int RT, int KGW>
__device__ __forceinline__ void bwd_step_mfma(floatx4 (&acc)[RT], __amdgpu_buffer_rsrc_t rs, long dbase, int Npad,
                                              const float *RT_s, int LDK, int br, int w, int fr, int fq) {
  constexpr int NA = (KGW % 4 == 0) ? 4 : (KGW % 2 == 0 ? 2 : 1);
  u32x4 af[KGW][RT];
#pragma unroll
  for (int i = 0; i < KGW; i++)
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
      af[i][rt] = ld_sc1(rs, (unsigned)((dbase + ((long)(w + 4 * i) * Npad + rt * 16 + fr) * 16 + fq * 4) * 4));
  floatx4 part[NA][RT];
#pragma unroll
  for (int a = 0; a < NA; a++)
#pragma unroll
    for (int rt = 0; rt < RT; rt++) part[a][rt] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float *brow = RT_s + br * LDK + fq * 4;
#pragma unroll
  for (int i0 = 0; i0 < KGW; i0 += NA) {
    floatx4 b[NA];
#pragma unroll
    for (int a = 0; a < NA; a++) b[a] = ld4(brow + (w + 4 * (i0 + a)) * 16);
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
      for (int a = 0; a < NA; a++)
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
          part[a][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[i0 + a][rt][s]), b[a][s],
                                                             part[a][rt], 0, 0, 0);
  }
#pragma unroll
  for (int rt = 0; rt < RT; rt++) {
    floatx4 t = part[0][rt];
#pragma unroll
    for (int a = 1; a < NA; a++) t += part[a][rt];
    acc[rt] = t;
  }
}

// runtime trip count versions of the same bodies
template <int RT>
__device__ __forceinline__ void fwd_step_generic(floatx4 (&acc)[RT][kMaxCT], __amdgpu_buffer_rsrc_t rs, long dbase,
                                                 int Npad, int KG, int CT, const float *Rs, int LDR, int w, int fr,
                                                 int fq) {
  for (int kg = w; kg < KG; kg += 4) {
    u32x4 af[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
      af[rt] = ld_sc1(rs, (unsigned)((dbase + ((long)kg * Npad + rt * 16 + fr) * 16 + fq * 4) * 4));
#pragma unroll
    for (int ct = 0; ct < kMaxCT; ct++) {
      if (ct < CT) {
        const floatx4 b = ld4(Rs + (ct * 16 + fr) * LDR + kg * 16 + fq * 4);
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
          for (int rt = 0; rt < RT; rt++)
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[rt][s]), b[s], acc[rt][ct], 0, 0, 0);
      }
    }
  }
}
template <int RT>
__device__ __forceinline__ void bwd_step_generic(floatx4 (&acc)[RT], __amdgpu_buffer_rsrc_t rs, long dbase, int Npad,
                                                 int KG, const float *RT_s, int LDK, int br, int w, int fr, int fq) {
  for (int kg = w; kg < KG; kg += 4) {
    u32x4 af[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
      af[rt] = ld_sc1(rs, (unsigned)((dbase + ((long)kg * Npad + rt * 16 + fr) * 16 + fq * 4) * 4));
    const floatx4 b = ld4(RT_s + br * LDK + kg * 16 + fq * 4);
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
      for (int rt = 0; rt < RT; rt++)
        acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[rt][s]), b[s], acc[rt], 0, 0, 0);
  }
}

// Everything else a step reads from or writes to HBM (next step's input
// projection / dy / saved activations, the row-major y / E copies) is issued
// right AFTER the step's hand-off loads have been consumed, never in front of
// them: a wave's vector memory operations complete in issue order.
template <int MODE, int RT>
__global__ __launch_bounds__(NT, 1) void rnn_fwd_rec(RecParams p) {
  REC_TRACE_INIT;
  constexpr int NW = MODE == kLstm ? 4 : MODE == kGru ? 3 : 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int bad_lds;
  int d, g;
  if (!block_of(p, d, g)) return;
  const int H = p.H, U = p.U, N = p.N, T = p.T, ncol = p.ncol, Npad = p.Npad;
  const int LDR = H + 4;
  const int u0 = g * U;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int CT = ncol / 16;
  const long ldy = (long)p.dirs * H, ldg = (long)p.dirs * NW * H;
  const int KG = H / 16;
  const long xstep = (long)p.dirs * KG * Npad * 16;  // floats of one step's exchange image
  float *Rs = smem;                      // [ncol][LDR]
  float *red = Rs + (long)ncol * LDR;    // [4][Npad][ncol]
  const float *Wd = p.w + d * p.pl_stride;
  const float *R = Wd + p.r_off;
  if (tid == 0) bad_lds = 0;
  for (int idx = tid; idx < ncol * H; idx += NT) {
    const int c = idx / H, k = idx - c * H;
    float v = 0.f;
    if (c < NW * U) {
      const int gt = c / U, u = c - gt * U;
      v = R[(long)(gt * H + u0 + u) * H + k];
    }
    Rs[c * LDR + k] = v;
  }
  const int items = N * U;
  float cst[kMaxEPT], hpv[kMaxEPT], gin[kMaxEPT][NW], gnx[kMaxEPT][NW], bR[kMaxEPT][NW];
  float act[kMaxEPT][NW], cnew[kMaxEPT], hval[kMaxEPT];
  auto gin_load = [&](int t, float (&dst)[kMaxEPT][NW]) {
#pragma unroll
    for (int j = 0; j < kMaxEPT; j++) {
      const int e = tid + j * NT, n = e / U, u = e - n * U;
      if (e < items) {
#pragma unroll
        for (int q = 0; q < NW; q++) dst[j][q] = p.G[((long)t * N + n) * ldg + (long)d * NW * H + q * H + u0 + u];
      }
    }
  };
  // row-major outputs of step t: y, and for the backward pass G (activations,
  // overwritten in place) and aux
  auto out_store = [&](int t) {
#pragma unroll
    for (int j = 0; j < kMaxEPT; j++) {
      const int e = tid + j * NT, n = e / U, u = e - n * U;
      if (e < items) {
        p.y[((long)t * N + n) * ldy + (long)d * H + u0 + u] = hval[j];
        if (MODE == kLstm || MODE == kGru) {
          const long grow = ((long)t * N + n) * ldg + (long)d * NW * H + u0 + u;
#pragma unroll
          for (int q = 0; q < NW; q++) p.G[grow + q * H] = act[j][q];
          p.aux[((long)t * N + n) * ldy + (long)d * H + u0 + u] = cnew[j];
        }
      }
    }
  };
#pragma unroll
  for (int j = 0; j < kMaxEPT; j++) {
    cst[j] = hpv[j] = cnew[j] = hval[j] = 0.f;
    const int e = tid + j * NT, u = e % U;
#pragma unroll
    for (int q = 0; q < NW; q++) {
      bR[j][q] = (MODE == kGru && e < items) ? Wd[p.bR_off + q * H + u0 + u] : 0.f;
      gin[j][q] = gnx[j][q] = act[j][q] = 0.f;
    }
  }
  gin_load(d == 0 ? 0 : T - 1, gin);
  __syncthreads();  // the R slice and bad_lds are in place
  int bad = 0;
  unsigned *myflag = p.flags + d * p.nwg + g;
  const int KGW = KG / 4;
  const int fast = (KG % 4 == 0 && KGW * RT <= 32 && (KGW == 8 || KGW == 4)) ? CT * 100 + KGW / 2 : 0;
  const long dbase = (long)d * KG * Npad * 16;
  int t_prev = -1;
  for (int k = 0; k < T && !bad; k++) {
    const int t = d == 0 ? k : T - 1 - k, tp = d == 0 ? t - 1 : t + 1;
    floatx4 acc[RT][kMaxCT];
#pragma unroll
    for (int a = 0; a < RT; a++)
#pragma unroll
      for (int b = 0; b < kMaxCT; b++) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
    REC_TRACE(k, 0);
    if (k > 0) {
      wait_flags(p.flags + d * p.nwg, p.nwg, (unsigned)(k + 1), p.err, bad, &bad_lds);
      REC_TRACE(k, 1);
      const auto rs = rsrc(p.xch + (long)tp * xstep, (unsigned)(xstep * 4));
      switch (fast) {
        case 104: fwd_step_mfma<RT, 1, 8>(acc, rs, dbase, Npad, Rs, LDR, w, fr, fq); break;
        case 204: fwd_step_mfma<RT, 2, 8>(acc, rs, dbase, Npad, Rs, LDR, w, fr, fq); break;
        case 304: fwd_step_mfma<RT, 3, 8>(acc, rs, dbase, Npad, Rs, LDR, w, fr, fq); break;
        case 404: fwd_step_mfma<RT, 4, 8>(acc, rs, dbase, Npad, Rs, LDR, w, fr, fq); break;
        case 102: fwd_step_mfma<RT, 1, 4>(acc, rs, dbase, Npad, Rs, LDR, w, fr, fq); break;
        case 202: fwd_step_mfma<RT, 2, 4>(acc, rs, dbase, Npad, Rs, LDR, w, fr, fq); break;
        case 302: fwd_step_mfma<RT, 3, 4>(acc, rs, dbase, Npad, Rs, LDR, w, fr, fq); break;
        case 402: fwd_step_mfma<RT, 4, 4>(acc, rs, dbase, Npad, Rs, LDR, w, fr, fq); break;
        default: fwd_step_generic<RT>(acc, rs, dbase, Npad, KG, CT, Rs, LDR, w, fr, fq); break;
      }
    }
    asm volatile("" ::: "memory");
    // behind the hand-off loads: last step's row-major outputs, next step's
    // input projection
    if (t_prev >= 0) out_store(t_prev);
    if (k + 1 < T) gin_load(d == 0 ? t + 1 : t - 1, gnx);
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
      for (int ct = 0; ct < kMaxCT; ct++)
        if (ct < CT)
#pragma unroll
          for (int r = 0; r < 4; r++)
            red[((long)w * Npad + rt * 16 + fq * 4 + r) * ncol + ct * 16 + fr] = acc[rt][ct][r];
    if (p.trace) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      REC_TRACE_W(k, 10);
    }
    __syncthreads();
    REC_TRACE(k, 3);
    float *xt = p.xch + (long)t * xstep;
#pragma unroll
    for (int j = 0; j < kMaxEPT; j++) {
      const int e = tid + j * NT;
      if (e >= items) continue;
      const int n = e / U, u = e - n * U;
      float rh[NW];
#pragma unroll
      for (int q = 0; q < NW; q++) {
        const int c = q * U + u;
        rh[q] = ((red[((long)0 * Npad + n) * ncol + c] + red[((long)1 * Npad + n) * ncol + c]) +
                 red[((long)2 * Npad + n) * ncol + c]) + red[((long)3 * Npad + n) * ncol + c];
      }
      float h;
      if (MODE == kLstm) {
        act[j][0] = fsigm(gin[j][0] + rh[0]);
        act[j][1] = fsigm(gin[j][1] + rh[1]);
        act[j][2] = ftanh(gin[j][2] + rh[2]);
        act[j][3] = fsigm(gin[j][3] + rh[3]);
        cst[j] = act[j][1] * cst[j] + act[j][0] * act[j][2];
        cnew[j] = cst[j];
        h = act[j][3] * ftanh(cst[j]);
      } else if (MODE == kGru) {
        act[j][0] = fsigm(gin[j][0] + rh[0] + bR[j][0]);
        act[j][1] = fsigm(gin[j][1] + rh[1] + bR[j][1]);
        cnew[j] = rh[2] + bR[j][2];
        act[j][2] = ftanh(gin[j][2] + act[j][0] * cnew[j]);
        h = (1.f - act[j][1]) * act[j][2] + act[j][1] * hpv[j];
        hpv[j] = h;
      } else {
        const float pre = gin[j][0] + rh[0];
        h = MODE == kRelu ? fmaxf(pre, 0.f) : ftanh(pre);
      }
      hval[j] = h;
      const int uu = u0 + u;
      put(xt + xoff(d, uu >> 4, n, uu & 15, KG, Npad), h, 0);
    }
    signal_epoch(myflag, (unsigned)(k + 2), 0);
    REC_TRACE(k, 4);
#pragma unroll
    for (int j = 0; j < kMaxEPT; j++)
#pragma unroll
      for (int q = 0; q < NW; q++) gin[j][q] = gnx[j][q];
    t_prev = t;
    __syncthreads();  // red[] is rewritten by the next step
    REC_TRACE(k, 5);
  }
  if (t_prev >= 0 && !bad) out_store(t_prev);
  if (bad && tid == 0) atomicOr(p.err, 1u);
}

template <int MODE, int RT>
__global__ __launch_bounds__(NT, 1) void rnn_bwd_rec(RecParams p) {
  REC_TRACE_INIT;
  constexpr int NW = MODE == kLstm ? 4 : MODE == kGru ? 3 : 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int bad_lds;
  int d, g;
  if (!block_of(p, d, g)) return;
  const int H = p.H, U = p.U, N = p.N, T = p.T, Npad = p.Npad;
  const int K = NW * H, LDK = K + 4;
  const int KG = K / 16;
  const long xstep = (long)p.dirs * KG * Npad * 16;
  const int u0 = g * U;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const long ldy = (long)p.dirs * H, ldg = (long)p.dirs * NW * H;
  const int br = fr < U ? fr : 0;           // the row of RT_s this lane's B fragments come from (bwd_step_mfma)
  float *RT_s = smem;                       // [U][LDK]: RT_s[u][kk] = R[kk][u0+u]
  float *red = RT_s + (long)U * LDK;        // [4][Npad][16]
  const float *Wd = p.w + d * p.pl_stride;
  const float *R = Wd + p.r_off;
  if (tid == 0) bad_lds = 0;
  for (int idx = tid; idx < U * K; idx += NT) {
    const int kk = idx / U, u = idx - kk * U;
    RT_s[u * LDK + kk] = R[(long)kk * H + u0 + u];
  }
  const int items = N * U;
  // per element: current step's operands (c*), the next step's (n*), and the
  // row-major dGates of the previous step waiting to be stored (e*, dxk)
  float carry[kMaxEPT], bsx[kMaxEPT][NW], bsh[kMaxEPT][NW], dxk[kMaxEPT][NW], eg[kMaxEPT][NW];
  float cg[kMaxEPT][NW], cdy[kMaxEPT], ca[kMaxEPT], cap[kMaxEPT];
  float ng[kMaxEPT][NW], ndy[kMaxEPT], na[kMaxEPT], nap[kMaxEPT];
#pragma unroll
  for (int j = 0; j < kMaxEPT; j++) {
    carry[j] = cdy[j] = ca[j] = cap[j] = ndy[j] = na[j] = nap[j] = 0.f;
#pragma unroll
    for (int q = 0; q < NW; q++) bsx[j][q] = bsh[j][q] = cg[j][q] = ng[j][q] = dxk[j][q] = eg[j][q] = 0.f;
  }
  auto prefetch = [&](int k) {  // operands of forward-order step k into n*
    const int t = d == 0 ? k : T - 1 - k, tp = d == 0 ? t - 1 : t + 1;
#pragma unroll
    for (int j = 0; j < kMaxEPT; j++) {
      const int e = tid + j * NT;
      if (e >= items) continue;
      const int n = e / U, u = e - n * U;
      const long yrow = ((long)t * N + n) * ldy + (long)d * H + u0 + u;
      const long grow = ((long)t * N + n) * ldg + (long)d * NW * H + u0 + u;
      const long prow = ((long)tp * N + n) * ldy + (long)d * H + u0 + u;
      ndy[j] = p.dy[yrow];
      if (MODE == kLstm || MODE == kGru) {
#pragma unroll
        for (int q = 0; q < NW; q++) ng[j][q] = p.G[grow + q * H];
        na[j] = p.aux[yrow];
      }
      if (MODE == kLstm) nap[j] = k > 0 ? p.aux[prow] : 0.f;
      else if (MODE == kGru) nap[j] = k > 0 ? p.y[prow] : 0.f;
      else nap[j] = p.y[yrow];
    }
  };
  auto rotate = [&]() {
#pragma unroll
    for (int j = 0; j < kMaxEPT; j++) {
      cdy[j] = ndy[j]; ca[j] = na[j]; cap[j] = nap[j];
#pragma unroll
      for (int q = 0; q < NW; q++) cg[j][q] = ng[j][q];
    }
  };
  auto e_store = [&](int t) {  // row-major dGates of step t (E; GRU also DX)
#pragma unroll
    for (int j = 0; j < kMaxEPT; j++) {
      const int e = tid + j * NT;
      if (e >= items) continue;
      const int n = e / U, u = e - n * U;
      const long grow = ((long)t * N + n) * ldg + (long)d * NW * H + u0 + u;
#pragma unroll
      for (int q = 0; q < NW; q++) p.E[grow + q * H] = eg[j][q];
      if (MODE == kGru) {
#pragma unroll
        for (int q = 0; q < NW; q++) p.DX[grow + q * H] = dxk[j][q];
      }
    }
  };
  prefetch(T - 1);
  rotate();
  __syncthreads();  // the R^T slice and bad_lds are in place
  int bad = 0;
  unsigned *myflag = p.flags + d * p.nwg + g;
  const int KGW = KG / 4;
  const int fast = (KG % 4 == 0 && KGW * RT <= 32 &&
                    (KGW == 32 || KGW == 24 || KGW == 16 || KGW == 12 || KGW == 8 || KGW == 4)) ? KGW : 0;
  const long dbase = (long)d * KG * Npad * 16;
  int t_prev = -1;
  for (int k = T - 1; k >= 0 && !bad; k--) {
    const int t = d == 0 ? k : T - 1 - k;
    const int tn = d == 0 ? t + 1 : t - 1;
    const int ks = T - 1 - k;             // steps done before this one
    floatx4 acc[RT];
#pragma unroll
    for (int a = 0; a < RT; a++) acc[a] = floatx4{0.f, 0.f, 0.f, 0.f};
    REC_TRACE(ks, 0);
    if (ks > 0) {
      wait_flags(p.flags + d * p.nwg, p.nwg, (unsigned)(ks + 1), p.err, bad, &bad_lds);
      REC_TRACE(ks, 1);
      const auto rs = rsrc(p.xch + (long)tn * xstep, (unsigned)(xstep * 4));
      switch (fast) {
        case 32: bwd_step_mfma<RT, 32>(acc, rs, dbase, Npad, RT_s, LDK, br, w, fr, fq); break;
        case 24: bwd_step_mfma<RT, 24>(acc, rs, dbase, Npad, RT_s, LDK, br, w, fr, fq); break;
        case 16: bwd_step_mfma<RT, 16>(acc, rs, dbase, Npad, RT_s, LDK, br, w, fr, fq); break;
        case 12: bwd_step_mfma<RT, 12>(acc, rs, dbase, Npad, RT_s, LDK, br, w, fr, fq); break;
        case 8: bwd_step_mfma<RT, 8>(acc, rs, dbase, Npad, RT_s, LDK, br, w, fr, fq); break;
        case 4: bwd_step_mfma<RT, 4>(acc, rs, dbase, Npad, RT_s, LDK, br, w, fr, fq); break;
        default: bwd_step_generic<RT>(acc, rs, dbase, Npad, KG, RT_s, LDK, br, w, fr, fq); break;
      }
    }
    asm volatile("" ::: "memory");
    // behind the hand-off loads: next step's operands, last step's row-major dGates
    if (k > 0) prefetch(k - 1);
    if (t_prev >= 0) e_store(t_prev);
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
      for (int r = 0; r < 4; r++) red[((long)w * Npad + rt * 16 + fq * 4 + r) * 16 + fr] = acc[rt][r];
    if (p.trace) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      REC_TRACE_W(ks, 10);
    }
    __syncthreads();
    REC_TRACE(ks, 3);
    float *xt = p.xch + (long)t * xstep;
#pragma unroll
    for (int j = 0; j < kMaxEPT; j++) {
      const int e = tid + j * NT;
      if (e >= items) continue;
      const int n = e / U, u = e - n * U;
      const float dhr = ((red[((long)0 * Npad + n) * 16 + u] + red[((long)1 * Npad + n) * 16 + u]) +
                         red[((long)2 * Npad + n) * 16 + u]) + red[((long)3 * Npad + n) * 16 + u];
      float dh = cdy[j] + dhr;
      const int uu = u0 + u;
      if (MODE == kLstm) {
        const float ig = cg[j][0], fg = cg[j][1], gg = cg[j][2], og = cg[j][3];
        const float tc = ftanh(ca[j]);
        const float dO = dh * tc;
        const float dc = dh * og * (1.f - tc * tc) + carry[j];
        eg[j][0] = dc * gg * ig * (1.f - ig);
        eg[j][1] = dc * cap[j] * fg * (1.f - fg);
        eg[j][2] = dc * ig * (1.f - gg * gg);
        eg[j][3] = dO * og * (1.f - og);
        carry[j] = dc * fg;
      } else if (MODE == kGru) {
        dh += carry[j];
        const float r = cg[j][0], z = cg[j][1], nn = cg[j][2];
        const float dn = dh * (1.f - z), dz = dh * (cap[j] - nn);
        const float dpn = dn * (1.f - nn * nn);
        const float dpr = dpn * ca[j] * r * (1.f - r);
        const float dpz = dz * z * (1.f - z);
        carry[j] = dh * z;
        dxk[j][0] = dpr; dxk[j][1] = dpz; dxk[j][2] = dpn;
        eg[j][0] = dpr; eg[j][1] = dpz; eg[j][2] = dpn * r;
        bsh[j][0] += dpr; bsh[j][1] += dpz; bsh[j][2] += dpn * r;
      } else {
        const float der = MODE == kRelu ? (cap[j] > 0.f ? 1.f : 0.f) : (1.f - cap[j] * cap[j]);
        eg[j][0] = dh * der;
      }
#pragma unroll
      for (int q = 0; q < NW; q++) {
        const int kk = q * H + uu;
        put(xt + xoff(d, kk >> 4, n, kk & 15, KG, Npad), eg[j][q], 0);
        bsx[j][q] += (MODE == kGru) ? dxk[j][q] : eg[j][q];
      }
    }
    signal_epoch(myflag, (unsigned)(ks + 2), 0);
    REC_TRACE(ks, 4);
    rotate();
    t_prev = t;
    __syncthreads();
    REC_TRACE(ks, 5);
  }
  if (t_prev >= 0 && !bad) e_store(t_prev);
  // bias partial sums: reduce over n in a fixed order through LDS
  float *bs = red;  // reuse: [2][N][U][NW] floats (fits: see lds sizing)
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kMaxEPT; j++) {
    const int e = tid + j * NT;
    if (e >= items) continue;
    const int n = e / U, u = e - n * U;
#pragma unroll
    for (int q = 0; q < NW; q++) {
      const long base = ((long)n * U + u) * NW + q;
      bs[base] = bsx[j][q];
      bs[(long)N * U * NW + base] = (MODE == kGru) ? bsh[j][q] : bsx[j][q];
    }
  }
  __syncthreads();
  for (int q = tid; q < 2 * NW * U; q += NT) {
    const int part = q / (NW * U), rem = q - part * NW * U, gt = rem / U, u = rem - gt * U;
    float s = 0.f;
    for (int n = 0; n < N; n++) s += bs[(long)part * N * U * NW + ((long)n * U + u) * NW + gt];
    p.bias[((long)d * 2 + part) * NW * H + gt * H + u0 + u] = s;
  }
  if (bad && tid == 0) atomicOr(p.err, 1u);
}

template <int MODE>
const void *generic_of_mode(bool fwd, int rt) {
  switch (rt) {
    case 1: return reinterpret_cast<const void *>(fwd ? rnn_fwd_rec<MODE, 1> : rnn_bwd_rec<MODE, 1>);
    case 2: return reinterpret_cast<const void *>(fwd ? rnn_fwd_rec<MODE, 2> : rnn_bwd_rec<MODE, 2>);
    case 3: return reinterpret_cast<const void *>(fwd ? rnn_fwd_rec<MODE, 3> : rnn_bwd_rec<MODE, 3>);
    default: return reinterpret_cast<const void *>(fwd ? rnn_fwd_rec<MODE, 4> : rnn_bwd_rec<MODE, 4>);
  }
}

}  // namespace

const void *rec_generic_kernel(bool fwd, int mode, int rt) {
  switch (mode) {
    case kLstm: return generic_of_mode<kLstm>(fwd, rt);
    case kGru: return generic_of_mode<kGru>(fwd, rt);
    case kRelu: return generic_of_mode<kRelu>(fwd, rt);
    default: return generic_of_mode<kTanh>(fwd, rt);
  }
}

}  // namespace kctc
