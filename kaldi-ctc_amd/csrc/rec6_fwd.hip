// rec6_fwd.hip -- rnn_fwd_rec6, the v6 forward recurrence, and its half of the
// kernel lookup.  Host side and protocol: rnn.hip.
#include "rec_common.h"

namespace kctc {
namespace {
// First definition of the unit on purpose: it puts threadIdx's accessor ahead of the kernels in the
// module, as it was in rnn.hip's unit.  Without it the compiler's constant propagation loses the sign
// of rrow's argument in the U = 8 bf16 kernels and their code differs (same results); nothing calls it.
__device__ __attribute__((used)) unsigned rec6_fwd_tid() { return threadIdx.x; }

// ---------------------------------------------------------------------------
// v6 forward: split-fp16 MFMA over an fp16 hi/lo all-gather of h
// ---------------------------------------------------------------------------
// WG (dir, g) owns units u0..u0+U-1; per step it multiplies h_{t-1} [16 x H]
// by its R slice (the nW*U gate rows of its units) on
// v_mfma_f32_16x16x32_f16 with the split-fp16 products of the v6 backward
// (R scaled per WG, h scaled by 2^14: |h| <= 1 for LSTM / GRU), K split over
// the 4 waves and reduced through LDS in a fixed order, then does the cell
// update of its (n, unit) elements and publishes h_t as the fp16 hi/lo pair
// of its units.  The exchange image of a step is A-fragment-major:
// [dir][kb = k/32][hi|lo][16 rows][32 k] halves (1 KB per fragment), the same
// 64 KB per step as the fp32 image of rec_generic.hip; a consumer lane loads 16 B of hi
// and 16 B of lo per 32-k block.  The R slice lives in registers (B
// fragments) for the whole launch.  Hand-off as there (sc1 stores, vmcnt(0),
// barrier, sc1 epoch flag; sc1 loads).
// Generalised like rnn_bwd_rec6: row groups of 16 sequences (block b ->
// direction b % dirs, workgroup (b / dirs) % NWG, group b / (dirs NWG); each
// group has its own flag lines and step images), NTH = 256 or 512 threads (K
// split over NTH / 64 waves), U up to 32; P = kPrecBf16 exchanges h as bf16
// and multiplies by a bf16 R slice (one MFMA per block, no scaling).
template <int MODE, int U, int H, int NTH, int P>
__global__ __launch_bounds__(NTH, 1) void rnn_fwd_rec6(RecParams p) {
  REC_TRACE_INIT;
  constexpr int NW = MODE == kLstm ? 4 : 3;
  constexpr int NWV = NTH / 64;
  // P & 4: IO waves.  The upper half of the waves neither waits for the
  // hand-off nor multiplies: they load the input projection rows (G) of the
  // coming steps and pass them through LDS.  A wave's vmcnt counts its loads
  // and stores in order, so a G load (HBM latency) issued by a hand-off wave
  // held up that wave's next flag poll / hand-off loads / publish drain
  // (measured: forward 2.38 -> 1.89 us/step with the G loads left out)
  constexpr bool IOW = (P & 4) != 0;
  // the row-major outputs through the IO waves too: measured slower (forward
  // 2.46 -> 2.52 us/step; the IO waves' waits then delay the post-cell barrier)
  constexpr bool IO_OUT = false;
  constexpr int PR = P & 3;
  constexpr int CW = IOW ? NWV / 2 : NWV;  // hand-off (compute) waves
  constexpr int NC = NW * U, CT = (NC + 15) / 16, RP = CT * 16 + 1;  // red row pitch (floats)
  constexpr int KB = H / 32, KBW = (KB + CW - 1) / CW, NWG = H / U;
  constexpr int CH = U / 8;  // 16-B chunks of a published row part
  constexpr bool BF = PR == kPrecBf16;
  constexpr bool STK = PR == kPrecX3S;  // hi / lo stacked in one 16-row A operand (groups of <= 8 rows)
  constexpr int NP = BF ? 1 : 2;  // parts of an exchanged h: hi (+ lo)
  // element rows: a stacked group has at most 8, and the folded K partials of
  // a wave are 8 rows (no thread, no LDS row for the rows that cannot be live)
  constexpr int ER = STK ? 8 : 16;
  static_assert(16 * U <= NTH, "one (row, unit) element per thread");
  static_assert(!IOW || (16 * U == CW * 64 && NW <= 4 && NP * 16 * U / 8 <= 64),
                "IO waves: the elements fill the compute waves, one publishing wave");
  using AT = typename std::conditional<BF, __bf16, _Float16>::type;
  using AV = typename std::conditional<BF, bf16x8, halfx8>::type;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int bad_lds, loc_lds;
  __shared__ float wmax[NWV];
  const int dirs = p.dirs;
  // xpd = 1: XCD-slot mapping as rnn_bwd_rec6 (block b -> (row group, direction)
  // slot b & 7, workgroup b >> 3: one XCD per slot under round-robin dispatch)
  const int d = p.xpd ? (blockIdx.x & 7) % dirs : blockIdx.x % dirs;
  const int g = p.xpd ? (blockIdx.x >> 3) : (blockIdx.x / dirs) % NWG;
  const int grp = p.xpd ? (blockIdx.x & 7) / dirs : blockIdx.x / (dirs * NWG);
  if (g >= NWG || grp >= p.rg) return;
  const int N = p.N, T = p.T, n0 = grp * p.gs, nend = min(N, n0 + p.gs);
  const int u0 = g * U;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const long ldy = (long)dirs * H, ldg = (long)dirs * NW * H;
  constexpr long XG = 2L * KB * NP * 16 * 32;  // halves per row group's image of a step (dirs <= 2)
  const long XS = XG * p.rg;                    // halves per step image
  float *red = smem;                                                       // [NWV][16][RP]
  // [NP][16][U], 16-B aligned.  Offset arithmetic on smem only: a pointer
  // rounded through an integer loses the LDS address space, and the staging
  // reads and writes became FLAT instructions (counted in vmcnt, so the
  // publish waited for every store of the step still in flight)
  constexpr int RPR = (U % 16 == 0 && NW <= 4 && 4 * U > RP) ? 4 * U : RP;  // red floats per (wave, row)
  constexpr int kStgOff = (NWV * 16 * RPR + 3 + 3) / 4 * 4;
  // (stacked: [CW][8][U] float4, the first half of these floats)
  static_assert(!STK || (U % 16 == 0 && NW <= 4), "stacked: float4 K partials");
  AT *stg = reinterpret_cast<AT *>(smem + kStgOff);
  // IO waves: the G rows of step k in slot k & 7, [8][NW][16 U] floats,
  // filled by LDS-DMA p.gla (3 or 7) steps ahead
  float *ginl = smem + kStgOff + (NP * 16 * U + 7) / 8 * 4;  // 16-B aligned
  float *outl = ginl + 8 * NW * 16 * U;  // (IO_OUT) [2][NW + 2][16 U]
  const float *Wd = p.w + d * p.pl_stride;
  const float *R = Wd + p.r_off;
  AT *xch = reinterpret_cast<AT *>(p.xch);
  if (tid == 0) bad_lds = 0;
  // ---- R slice -> B fragments: B[k][c] = R[q*H + u0 + u][k], c = q*U + u ----
  auto rrow = [&](int c) -> const float * {
    const int q = c / U, u = c - q * U;
    return R + (long)(q * H + u0 + u) * H;
  };
  int sB = 0, sOut = 0;
  if constexpr (!BF) {
    float mx = 0.f;
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
      const int c = ct * 16 + fr;
      if (c < NC) {
        const float *rr = rrow(c);
#pragma unroll
        for (int i = 0; i < KBW; i++) {
          const int kb = (!IOW || w < CW) ? w + CW * i : KB;
          if (kb < KB) {
#pragma unroll
            for (int j = 0; j < 8; j++) mx = fmaxf(mx, fabsf(rr[kb * 32 + fq * 8 + j]));
          }
        }
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) wmax[w] = mx;
    __syncthreads();
    float m4 = wmax[0];
#pragma unroll
    for (int i = 1; i < NWV; i++) m4 = fmaxf(m4, wmax[i]);
    sB = split_exp(m4);
    sOut = -(sB + 14);
  }
  AV bhi[CT][KBW], blo[BF ? 1 : CT][BF ? 1 : KBW];
#pragma unroll
  for (int ct = 0; ct < CT; ct++) {
    const int c = ct * 16 + fr;
#pragma unroll
    for (int i = 0; i < KBW; i++) {
      const int kb = (!IOW || w < CW) ? w + CW * i : KB;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float v = (c < NC && kb < KB) ? rrow(c)[kb * 32 + fq * 8 + j] : 0.f;
        if constexpr (BF) {
          bhi[ct][i][j] = (__bf16)v;
        } else {
          _Float16 h, l;
          split16(ldexpf(v, sB), h, l);
          bhi[ct][i][j] = h;
          blo[ct][i][j] = l;
        }
      }
    }
  }
  // ---- per-element state: thread tid <-> (row n0 + en, unit u0 + eu) ----
  const bool has_e = tid < ER * U;
  const int en = tid / U, eu = tid - en * U;
  const int n = n0 + en;
  const bool live = has_e && n < nend;
  float cst = 0.f, hpv = 0.f, cnew = 0.f, hval = 0.f;
  float gin[NW], gnx[NW], bR[NW], act[NW];
#pragma unroll
  for (int q = 0; q < NW; q++) {
    gin[q] = gnx[q] = act[q] = 0.f;
    bR[q] = (MODE == kGru && has_e) ? Wd[p.bR_off + q * H + u0 + eu] : 0.f;
  }
  // Row-major addressing of the step loop: the element's byte offsets in a
  // step's y / aux and G rows stay in two VGPRs (opaque to the compiler, or it
  // works them out again every step), and the step's rows are wave-uniform
  // bases (yrow, grow, arow below) moved by one step image a step with scalar
  // adds -- no per-lane 64-bit index arithmetic between the last MFMA and the
  // K-partial writes the workgroup's barrier waits for
  typedef const float __attribute__((address_space(1))) *gcfp;
  typedef float __attribute__((address_space(1))) *gfp;
  unsigned yob = (unsigned)(((long)n * ldy + (long)d * H + u0 + eu) * sizeof(float));
  unsigned gob = (unsigned)(((long)n * ldg + (long)d * NW * H + u0 + eu) * sizeof(float));
  asm volatile("" : "+v"(yob), "+v"(gob));
  auto at = [](const float *base, unsigned ob) {  // element at byte offset ob of a step's rows
    return (gfp) reinterpret_cast<float *>(reinterpret_cast<uintptr_t>(base) + ob);
  };
  auto gin_load = [&](const float *gr, float (&dst)[NW]) {  // gr: the step's G rows
    if (!live) return;
    const gcfp s = at(gr, gob);
#pragma unroll
    for (int q = 0; q < NW; q++) dst[q] = s[q * H];
  };
  // bf16_io: the step's h (stg, bf16 [16][U]) as packed rows and columns
  auto y_pk_store = [&](int tt) {
    if constexpr (BF) {
      constexpr int RCH = U / 8;
      const long f0 = (long)tt * N + n0;
      const int i = tid;
      if (i < 16 * RCH) {
        const int rn = i / RCH, ch = i - rn * RCH;
        if (n0 + rn < nend)
          *reinterpret_cast<u32x4 *>(p.yr + (f0 + rn) * ldy + (long)d * H + u0 + ch * 8) =
              *reinterpret_cast<const u32x4 *>(stg + rn * U + ch * 8);
      } else if (i < 16 * RCH + 2 * U) {
        const int col = (i - 16 * RCH) >> 1, half = (i - 16 * RCH) & 1, r0 = half * 8;
        __bf16 *dst = p.yc + ((long)d * H + u0 + col) * p.kbt64 + f0 + r0;
        if ((N % 8 == 0) && (n0 % 8 == 0) && n0 + r0 + 8 <= nend) {
          bf16x8 v;
#pragma unroll
          for (int j = 0; j < 8; j++) v[j] = stg[(r0 + j) * U + col];
          *reinterpret_cast<bf16x8 *>(dst) = v;
        } else {
          for (int j = 0; j < 8; j++)
            if (n0 + r0 + j < nend) dst[j] = stg[(r0 + j) * U + col];
        }
      }
    }
  };
  // row-major y, activations (in place of G), aux of a step, given its rows
  auto out_store = [&](const float *yr, const float *gr, const float *ar) {
    if (!live) return;
    if (p.ysc1) __hip_atomic_store(at(yr, yob), hval, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);  // read by other XCDs during this kernel
    else *at(yr, yob) = hval;
    const gfp gd = at(gr, gob);
#pragma unroll
    for (int q = 0; q < NW; q++) gd[q * H] = act[q];
    *at(ar, yob) = cnew;
  };
  // IO waves: thread tid - 64 CW <-> element (ion, iou); G of step k into
  // ginl[k & 1] before step k's K-reduction barrier
  const int iot = tid - 64 * CW, ion = iot / U, iou = iot - ion * U;
  const bool io_live = IOW && w >= CW && n0 + ion < nend;
  // G row of forward-order step kk of this lane's element into slot kk & 7
  // by LDS-DMA (lane l of IO wave v writes element 64 v + l); NW DMAs per
  // call whatever kk, so that the waits can count them (rows past N and
  // steps past T read a valid row and are never used)
  auto io_dma = [&](int kk) {
    const int tt = d == 0 ? min(kk, T - 1) : max(T - 1 - kk, 0);
    const long gr = ((long)tt * N + n0 + (io_live ? ion : 0)) * ldg + (long)d * NW * H + u0 + iou;
#pragma unroll
    for (int q = 0; q < NW; q++) {
      const unsigned dst = __builtin_amdgcn_readfirstlane(
          (unsigned)reinterpret_cast<uintptr_t>(ginl + ((kk & 7) * NW + q) * 16 * U + (w - CW) * 64));
      dma_lds_dword(p.G + gr + q * H, dst);
    }
  };
  auto io_out = [&](int kk) {  // row-major outputs of step kk from outl[kk & 1]
    if (!io_live) return;
    const int tt = d == 0 ? kk : T - 1 - kk;
    const float *o = outl + (long)(kk & 1) * (NW + 2) * 16 * U + iot;
    const long yrow = ((long)tt * N + n0 + ion) * ldy + (long)d * H + u0 + iou;
    const long grow = ((long)tt * N + n0 + ion) * ldg + (long)d * NW * H + u0 + iou;
    p.y[yrow] = o[0];
#pragma unroll
    for (int q = 0; q < NW; q++) p.G[grow + q * H] = o[(1 + q) * 16 * U];
    p.aux[yrow] = o[(NW + 1) * 16 * U];
  };
  // the IO waves' wait for step k + 1's G: at most (gla - 1) * NW DMAs (the
  // steps after it) still in flight
  const bool gla7 = p.gla == 7;
  auto io_wait = [&]() {
    if (gla7) {
      if constexpr (NW == 4) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
    } else {
      if constexpr (NW == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    }
  };
  if constexpr (IOW) {
    if (w >= CW) {  // steps 0 .. gla - 1; step 0's in place before the loop's first barrier
      for (int kk = 0; kk < (gla7 ? 7 : 3); kk++) io_dma(kk);
      io_wait();
    }
    __syncthreads();
  }
  // the rows of the loop's current step (time t): wave-uniform, one step
  // image (tstep frames) on at the end of every step
  const long ysl = (d == 0 ? 1 : -1) * (long)N * ldy, gsl = (d == 0 ? 1 : -1) * (long)N * ldg;
  const float *yrow = p.y + (long)(d == 0 ? 0 : T - 1) * N * ldy;
  const float *arow = p.aux + (long)(d == 0 ? 0 : T - 1) * N * ldy;
  const float *grow = p.G + (long)(d == 0 ? 0 : T - 1) * N * ldg;
  if constexpr (!IOW) gin_load(grow, gin);
  int bad = 0;
  unsigned *myflag = flag6(p, grp, d, g, NWG);
  // XCD-pinned (p.xpd): the hand-off goes through a ring of p.ring step images
  // after the T per-step images, kept in the XCD's L2 (plain stores, workgroup-
  // scope flags) when probe6 finds the direction's workgroups on one XCD; a
  // streamed projection on the other XCDs reads the per-step images, written
  // through (sc1) behind the next step's hand-off loads, and follows sc1
  // copies of the epochs 256 lines on: gflag = k in step k's load phase
  // (step k - 1's signal drained step k - 2's copy), T + 1 at exit -- "epoch
  // - 2 = last step out" as the unpinned flags
  // (aggregated over the direction's workgroups by workgroup 0, as in
  // rnn_bwd_rec6: agg_flag6 = k after the K-reduction barrier of step k, by
  // which every producer's signal of step k - 1 drained its copy of step k - 2)
  // (compiled into the IO-wave variant only, the one chain_ok lets stream
  // off a pinned producer: the dead code of it in the other variants changed
  // their schedules -- U = 32 forward 3.19 -> 4.0 us/step at configs[2])
  const bool fcopy = IOW && p.xpd && p.fcopy;
  // y rows streamed (p.ysc1): step m's y goes out in step m + 1, behind that
  // step's hand-off loads, so it has landed once the workgroup publishes step
  // m + 2; workgroup 0 has every producer's step k - 1 image in step k, so
  // gflag = k there means rows of steps <= k - 3 are out ("epoch s + 3" as
  // the backward's rows), T + 2 at exit
  unsigned *gflag = ((fcopy || p.ysc1) && g == 0) ? agg_flag6(p, grp, d) : nullptr;
  if (tid == 0) {  // (the side launches' residency gate: beside_recurrence)
    if (p.xpd) atomicOr(p.flags + kXcdWord, 1u << xcc_id());
    atomicAdd(p.flags + kResWord, 1u);
  }
  if (tid == 0) loc_lds = 0;
  const int local = (p.xpd && p.allow_local) ? probe6(p, grp, d, g, NWG, bad, &bad_lds, &loc_lds) : 0;
  if (trc_ && tid == 0) trc_[9] = (unsigned long long)(local + 1);  // step 0, slot 9
  const long rbase = (long)T * XS;  // ring slots (p.ring > 0)
  // Self-tagged hand-off (as rnn_bwd_rec6): every fp16 half of step k's h
  // image carries ((k >> 1) & 1) in its LSB (hi's change is taken up by lo,
  // lo's own LSB costs 2^-21 of |h| at most); the consumers poll the image
  // words themselves: no drain, no flag.  Split-fp16 without IO waves, no
  // write-through copy for a streamed projection, ring of two L2 images set
  // to tag 1 before the launch.
  const bool dtag = !BF && !IOW && !fcopy && p.dtag && local && p.ring == 2;
  // the published 16 B of h: live across the whole loop (used after it), so
  // that no other value of the step is allocated to the data registers of the
  // write-through copy still in flight (gfx9 waits for a store's completion
  // before its data VGPRs are overwritten)
  u32x4 pv = u32x4{0u, 0u, 0u, 0u};
  // the per-step images as one loop-invariant buffer (chain_ok: T XS halves < 2 GB)
  const auto crs = rsrc(xch, fcopy ? (unsigned)(T * XS * sizeof(AT)) : 0u);
  // publish geometry: store thread s < NP * 16 * CH: part = s / (16 CH), row, chunk
  const int sp = tid / (16 * CH), sn = (tid / CH) % 16, sch = tid % CH;
  const int kb0 = u0 >> 5, koff = (u0 & 31) + sch * 8;
  // rows past N (a group of fewer than 16 sequences) are neither loaded nor stored
  // (STK: lanes fr >= 8 load the lo part of row fr - 8)
  const bool arow_live = n0 + (STK ? (fr & 7) : fr) < nend;
  // per-wave wait: the producers of the k blocks this wave loads (32 / U per block)
  int wprod = -1;
  {
    constexpr int PPK = 32 / U;
    const int i = lane / PPK, kb = (!IOW || w < CW) ? w + CW * i : KB;
    if (i < KBW && kb < KB) wprod = kb * PPK + lane % PPK;
  }
  const long gimg = (long)grp * XG;
  const bool pub = tid < NP * 16 * CH && n0 + sn < nend;  // a publishing thread: 16 B of h
  const long po = gimg + ((((long)d * KB + kb0) * NP + sp) * 16 + sn) * 32 + koff;
  // stacked fold: the two rows of a tile this lane keeps (row, row + 1)
  const int frow = (fq & 1) * 4 + (fq >> 1) * 2;
  int t_prev = -1;
  for (int k = 0; k < T && !bad; k++) {
    const int t = d == 0 ? k : T - 1 - k, tp = d == 0 ? t - 1 : t + 1;
    floatx4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ct++) acc[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
    REC_TRACE(k, 0);
    if (k > 0 && (!IOW || w < CW)) {
      if (dtag) {
        // self-tagged: the poll below is the wait
      } else {
        if (!wave_wait_prod(flag6(p, grp, d, 0, NWG), wprod, (unsigned)(k + 1), p.err, &bad_lds, p.poll_sleep)) bad = 1;
      }
      REC_TRACE(k, 1);
      const auto rs = rsrc(xch + (p.ring ? rbase + (long)((k - 1) & 1) * XS : (long)tp * XS),
                           (unsigned)(XS * sizeof(AT)));
      u32x4 ah[KBW], al[KBW];
      unsigned aoff[KBW];
      // unconditional loads (rows past N and k blocks past KB at an offset
      // past the buffer: the hardware returns zeros), so that the compiler
      // counts them exactly and the first MFMAs wait for their own loads only
#pragma unroll
      for (int i = 0; i < KBW; i++) {
        const int kb = w + CW * i;
        const long o = STK ? gimg + ((((long)d * KB + kb) * NP + (fr >> 3)) * 16 + (fr & 7)) * 32 + fq * 8
                           : gimg + ((((long)d * KB + kb) * NP) * 16 + fr) * 32 + fq * 8;
        const unsigned off = (kb < KB && arow_live) ? (unsigned)(o * sizeof(AT)) : 0x7fff0000u;
        aoff[i] = off;
        ah[i] = ld_sc1(rs, off);
        if constexpr (!BF && !STK) al[i] = ld_sc1(rs, off + 16 * 32 * sizeof(AT));
      }
      if constexpr (!BF) {
        if (dtag) {
          // every half of step k - 1 carries ((k - 1) >> 1) & 1 in its LSB
          // (bits 0 and 16 of a word; 4-B words are single-copy atomic); a
          // chunk still holding step k - 3's halves is loaded again
          const unsigned want = ((unsigned)((k - 1) >> 1) & 1u) * 0x00010001u;
          // (rows past N and k blocks past KB: zeros from past the buffer, no tag)
          const bool any_live = arow_live && w < KB;
          auto ready = [&]() {
            unsigned bad4 = 0u;
#pragma unroll
            for (int i = 0; i < KBW; i++) {
              if (w + CW * i < KB) {
                bad4 |= (ah[i][0] ^ want) | (ah[i][1] ^ want) | (ah[i][2] ^ want) | (ah[i][3] ^ want);
                if constexpr (!STK) bad4 |= (al[i][0] ^ want) | (al[i][1] ^ want) | (al[i][2] ^ want) | (al[i][3] ^ want);
              }
            }
            return !any_live || (bad4 & 0x00010001u) == 0u;
          };
          int spins = 0;
          while (!__all(ready())) {  // (not all there yet: the wave loads all its chunks again)
            if (++spins > kSpinLimit ||
                ((spins & 255) == 0 &&
                 __builtin_amdgcn_readfirstlane(__hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))) {
              bad = 1;
              if (lane == 0) bad_lds = 1;
              break;
            }
            if (p.poll_sleep) __builtin_amdgcn_s_sleep(1);
            asm volatile("" ::: "memory");
#pragma unroll
            for (int i = 0; i < KBW; i++) {
              ah[i] = ld_sc1(rs, aoff[i]);
              if constexpr (!BF && !STK) al[i] = ld_sc1(rs, aoff[i] + 16 * 32 * sizeof(AT));
            }
          }
        }
      }
      // all hand-off loads in flight before the first MFMA waits: without
      // this the scheduler (U = 32) issued the second k block's loads only
      // after the first block's MFMAs, one more L2 round trip per step
      __builtin_amdgcn_sched_barrier(0);
      // the streamed projection's write-through copy of the previous step's
      // image (pv still holds it), issued behind this step's hand-off loads:
      // gfx9 counts stores and loads in one vmcnt, so a write-through store
      // in flight at the next flag poll would hold up that poll; here the
      // waits for the loads ahead of it do not cover it, and this step's
      // signal drains it (the next step publishes its epoch)
      // (every lane of every wave issues it -- non-publishing lanes at an
      // offset past the buffer, which the hardware drops -- so that no
      // branch makes the compiler's wait counts conservative)
      // (unconditional: without a consumer crs covers 0 bytes and the store is dropped)
      __builtin_amdgcn_raw_buffer_store_b128(pv, crs, pub ? (int)(po * sizeof(AT)) : 0x7ffffff0,
                                             fcopy ? (int)(tp * XS * sizeof(AT)) : 0, 16);

#pragma unroll
      for (int i = 0; i < KBW; i++) {
        if (w + CW * i < KB) {
          const AV a0 = __builtin_bit_cast(AV, ah[i]);
          if constexpr (BF) {
#pragma unroll
            for (int ct = 0; ct < CT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bhi[ct][i], acc[ct], 0, 0, 0);
          } else if constexpr (STK) {
#pragma unroll
            for (int ct = 0; ct < CT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bhi[ct][i], acc[ct], 0, 0, 0);
#pragma unroll
            for (int ct = 0; ct < CT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, blo[ct][i], acc[ct], 0, 0, 0);
          } else {
            const AV a1 = __builtin_bit_cast(AV, al[i]);
#pragma unroll
            for (int ct = 0; ct < CT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bhi[ct][i], acc[ct], 0, 0, 0);
#pragma unroll
            for (int ct = 0; ct < CT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, blo[ct][i], acc[ct], 0, 0, 0);
#pragma unroll
            for (int ct = 0; ct < CT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bhi[ct][i], acc[ct], 0, 0, 0);
          }
        }
      }
      if constexpr (!IOW) {
        // this step's input projection row (loaded behind the last step's
        // hand-off loads) moves in here: the first MFMA's wait for the
        // hand-off loads has retired those older loads too (one in-order
        // vmcnt), so the cell below does not wait for memory.  Rotated in
        // the cell instead, the wait for them -- HBM misses -- and for the
        // row stores issued with them stood between the cell's exp and rcp
#pragma unroll
        for (int q = 0; q < NW; q++) gin[q] = gnx[q];
      }
    }
    asm volatile("" ::: "memory");
    // behind the hand-off loads: last step's row-major outputs, next step's input projection
    if (!IO_OUT && t_prev >= 0) out_store(yrow - ysl, grow - gsl, arow - ysl);
    // (stg still holds step t_prev's h: the cell phase below rewrites it)
    if (BF && p.yr && t_prev >= 0) y_pk_store(t_prev);
    if (!IOW && k + 1 < T) gin_load(grow + gsl, gnx);
    // K partials through LDS.  U % 16 == 0: column ct * 16 + fr of the
    // tile is gate ct / (U / 16) of unit (ct % (U / 16)) * 16 + fr, so a lane
    // holds every gate of its (row, unit) elements: one float4 per (wave,
    // row, unit) [NWV][16][U][4], and a cell thread sums NWV float4 reads
    // (4x fewer LDS instructions than one float per gate)
    constexpr bool RED4 = U % 16 == 0 && NW <= 4;
    if constexpr (STK) {
      // Rows 8..15 of a tile (lanes 32..63) hold the lo parts' products of rows
      // 0..7: row r + row r + 8, hi first.  v_permlane32_swap of register i
      // against register i + 2 (not against itself): one swap serves two rows,
      // every lane ends with two live sums: lanes 0..31 rows fq * 4 + {0, 1},
      // lanes 32..63 rows (fq - 2) * 4 + {2, 3}  (= frow, frow + 1).  Half the
      // swaps, no garbage lanes, and a wave's partials are 8 rows of float4
      constexpr int SU = U / 16;
      float sm2[CT][2];
#pragma unroll
      for (int ct = 0; ct < CT; ct++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[ct][j]), __float_as_uint(acc[ct][j + 2]),
                                                          false, false);
          sm2[ct][j] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        }
#pragma unroll
      for (int su = 0; su < SU; su++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
          floatx4 v4 = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int q = 0; q < NW; q++) v4[q] = sm2[q * SU + su][j];
          st4(red + (((long)(w * ER + frow + j) * U + su * 16 + fr) << 2), v4);
        }
    } else if constexpr (RED4) {
      constexpr int SU = U / 16;
      if (!IOW || w < CW) {
#pragma unroll
        for (int su = 0; su < SU; su++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            floatx4 v4 = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < NW; q++) v4[q] = acc[q * SU + su][i];
            st4(red + (((long)(w * 16 + fq * 4 + i) * U + su * 16 + fr) << 2), v4);
          }
      }
    } else {
#pragma unroll
      for (int ct = 0; ct < CT; ct++)
#pragma unroll
        for (int i = 0; i < 4; i++) red[(w * 16 + fq * 4 + i) * RP + ct * 16 + fr] = acc[ct][i];
    }
    lds_barrier<IOW>();
    if (bad_lds) bad = 1;
    // the aggregated epoch (before the signal: a write-through flag store
    // left in flight there would hold up the next step's first flag poll)
    if (gflag && k > 0 && tid == 0) __hip_atomic_store(gflag, (unsigned)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    REC_TRACE(k, 3);
    if (has_e) {
      float rh[NW];
      if constexpr (RED4) {
        floatx4 sm = *reinterpret_cast<const floatx4 *>(red + (((long)en * U + eu) << 2));  // fixed order
#pragma unroll
        for (int v = 1; v < CW; v++) sm += *reinterpret_cast<const floatx4 *>(red + (((long)(v * ER + en) * U + eu) << 2));
        if constexpr (IOW) {  // this step's G row, put there by the IO waves
#pragma unroll
          for (int q = 0; q < NW; q++) gin[q] = ginl[((k & 7) * NW + q) * 16 * U + tid];
        }
#pragma unroll
        for (int q = 0; q < NW; q++) rh[q] = BF ? sm[q] : ldexpf(sm[q], sOut);
      } else {
#pragma unroll
        for (int q = 0; q < NW; q++) {
          const int c = q * U + eu;
          float sm = red[(0 * 16 + en) * RP + c];  // the waves' K partials in a fixed order
#pragma unroll
          for (int v = 1; v < NWV; v++) sm += red[(v * 16 + en) * RP + c];
          rh[q] = BF ? sm : ldexpf(sm, sOut);
        }
      }
      float h;
      if (MODE == kLstm) {
        act[0] = fsigm(gin[0] + rh[0]);
        act[1] = fsigm(gin[1] + rh[1]);
        act[2] = ftanh(gin[2] + rh[2]);
        act[3] = fsigm(gin[3] + rh[3]);
        cst = act[1] * cst + act[0] * act[2];
        cnew = cst;
        h = act[3] * ftanh(cst);
      } else {
        act[0] = fsigm(gin[0] + rh[0] + bR[0]);
        act[1] = fsigm(gin[1] + rh[1] + bR[1]);
        cnew = rh[2] + bR[2];
        act[2] = ftanh(gin[2] + act[0] * cnew);
        h = (1.f - act[1]) * act[2] + act[1] * hpv;
        hpv = h;
      }
      if (!live) h = 0.f;
      hval = h;
      if constexpr (IO_OUT) {  // outputs for the IO waves (stored during the next step)
        float *o = outl + (long)(k & 1) * (NW + 2) * 16 * U + tid;
        o[0] = h;
#pragma unroll
        for (int q = 0; q < NW; q++) o[(1 + q) * 16 * U] = act[q];
        o[(NW + 1) * 16 * U] = cnew;
      }

      if constexpr (BF) {
        stg[en * U + eu] = (__bf16)h;
      } else {
        _Float16 hh, hl;
        if (!IOW) {  // hi's LSB := tag, lo takes up the change, then lo's LSB := tag
          // (in every mode a self-tagged launch may take: pinned and unpinned
          // runs stay bit-identical)
          const unsigned short tgh = (unsigned short)((k >> 1) & 1);
          const float x = h * 16384.f;
          hh = __builtin_bit_cast(_Float16, (unsigned short)((__builtin_bit_cast(unsigned short, (_Float16)x) & 0xFFFEu) | tgh));
          hl = __builtin_bit_cast(_Float16, (unsigned short)((__builtin_bit_cast(unsigned short, (_Float16)(x - (float)hh)) & 0xFFFEu) | tgh));
        } else {
          split16(h * 16384.f, hh, hl);
        }
        stg[en * U + eu] = hh;
        stg[(16 + en) * U + eu] = hl;
      }
    }
    if (IOW && w >= CW) {
      // IO waves, while the cell threads work: step k + 1's G (loaded during
      // step k - 1) into its slot -- read by the cell threads after the next
      // K-reduction barrier; the slot's step k - 1 readers passed the
      // barrier below last step -- then step k + 2's loads, then the
      // row-major outputs of step k - 1 (written before the last barrier;
      // their slot is rewritten after the next K-reduction barrier)
      {
        // step k + gla's G into slot (k + gla) & 7 (gla <= 7: last read by the
        // cell threads of step k - 1 at the latest, before the last barrier),
        // then wait for step k + 1's: in place before the barrier below,
        // gla - 1 steps after it was asked for
        io_dma(k + (gla7 ? 7 : 3));
        io_wait();
      }
      if (IO_OUT && k > 0) io_out(k - 1);
    }
    lds_barrier<IOW>();
    if (pub) {
      pv = *reinterpret_cast<const u32x4 *>(stg + (sp * 16 + sn) * U + sch * 8);
      const auto ro = rsrc(xch + (p.ring ? rbase + (long)(k & 1) * XS : (long)t * XS), (unsigned)(XS * sizeof(AT)));
      // local: plain stores stay in the XCD's L2 for the consumers' sc1 loads
      if (local) __builtin_amdgcn_raw_buffer_store_b128(pv, ro, (int)(po * sizeof(AT)), 0, 0);
      else __builtin_amdgcn_raw_buffer_store_b128(pv, ro, (int)(po * sizeof(AT)), 0, 16);
    }
    REC_TRACE(k, 7);
    if constexpr (NP * 16 * CH <= 64) {
      // one publishing wave (wave 0 stores the whole h part): it drains its
      // own stores and raises the flag, no workgroup barrier.  The other
      // waves go on to the next step's wait: their reads of red and stg this
      // step all came before the barrier above, and the next writes of either
      // follow the next K-reduction barrier, which wave 0 reaches only after
      // its stg read
      if (w == 0 && !dtag) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
          if (local) __hip_atomic_store(myflag, (unsigned)(k + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          else __hip_atomic_store(myflag, (unsigned)(k + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    } else if (!dtag) {
      signal_epoch(myflag, (unsigned)(k + 2), local);
    }
    REC_TRACE(k, 4);
    t_prev = t;
    yrow += ysl; arow += ysl; grow += gsl;
    REC_TRACE(k, 5);
  }
  if (IOW && w >= CW) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the IO waves' DMAs (ahead of T) land
  if (t_prev >= 0 && !bad) {
    if (BF && p.yr) y_pk_store(t_prev);
    if constexpr (IO_OUT) {
      if (w >= CW) io_out(T - 1);  // outl of the last step: written before the loop's last barrier
    } else {
      out_store(yrow - ysl, grow - gsl, arow - ysl);
    }
  }
  if ((fcopy || p.ysc1) && !bad) {  // the last step's copy / rows, then (workgroup 0) every producer's, then the epoch
    if (fcopy && pub)
      __builtin_amdgcn_raw_buffer_store_b128(pv, rsrc(xch + (long)t_prev * XS, (unsigned)(XS * sizeof(AT))),
                                             (int)(po * sizeof(AT)), 0, 16);
    signal_epoch(myflag, (unsigned)(T + 2), local);
    if (gflag) {
      wait_flags6(flag6(p, grp, d, 0, NWG), NWG, (unsigned)(T + 2), p.err, bad, &bad_lds, p.poll_sleep);
      if (!bad && tid == 0)
        __hip_atomic_store(gflag, (unsigned)(fcopy ? T + 1 : T + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  asm volatile("" ::"v"(pv));
  if (bad && tid == 0) atomicOr(p.err, 1u);
}

struct Fwd6 {
  template <int MODE, int U, int H, int NTH, int P>
  static const void *get() { return reinterpret_cast<const void *>(rnn_fwd_rec6<MODE, U, H, NTH, P>); }
};

}  // namespace

const void *rec6_fwd_kernel(int mode, int prec, int H, const V6Cfg &c) { return rec6_of<Fwd6>(mode, prec, H, c); }

}  // namespace kctc
