// sc_window.hip -- window previews of the re-scoring short lists on the matrix cores (gfx950 / CDNA4).
//
// Where it sits.  The lower-bound filter (sc_spec.hip / sc_filter.hip) gives every (query, entry) pair the minimum of
// the column-cosine distance over ALL 60 shifts; sc_select_kernel turns a query's row of bounds into a short list in
// ascending-bound order; the re-scoring needs, for every short-list entry it looks at,
//     k*  = the sector-key alignment of the pair (fastAlignUsingVkey, SC.cpp:93-113) and
//     pv ~= dist(query, entry) = min over the 7 shifts k* - 3 .. k* + 3 of d_k (SC.cpp:116-148)
// to decide which few entries deserve the exact fp64 evaluation.  Rounds 1-2 computed both on the VALU, one entry per
// wavefront (phase_a in sc_kernels.hip: ~650 issue slots per entry, 137 entries per query: 73 % of the re-scoring
// kernel).  Both are circular correlations of the query with the entry -- GEMMs whose A operand is a circulant of the
// query -- so for the head of every short list (two passes, see the kernel) they are computed here, 32 entries per wavefront:
//   * alignment: KC[k] = sum_j vkey_q[(j + k) % 60] * vkey_e[j], K = 64, keys scaled by a power of two and split into
//     fp16 hi + lo (hi*hi + hi*lo + lo*hi: 24 v_mfma_f32_32x32x16_f16 for 2 x 32 shifts x 32 entries).  argmin_k of
//     ||vkey_q - shift_k(vkey_e)|| = argmax_k KC[k] (the two squared norms do not depend on k).  The maximum is taken
//     as k* only when it is UNIQUE within the error bound of KC (below); otherwise k* = -1 and the preview is taken
//     over the union of the windows of every shift that could be the reference's choice -- still a valid LOWER bound of
//     the pair distance, so such an entry is usually pruned as well, and only if it survives does the re-scoring kernel
//     run the exact fp64 alignment with the reference's tie rule.
//   * preview: S[k][e] = sum_i q2[i + 20 k] * e[i], K = 1200, exactly the direct filter's GEMM (same fp16 images, same
//     circulant addressing of the query image in LDS, same epilogue arithmetic) -- 150 MFMAs per 32 entries -- but the
//     epilogue takes the minimum of d_k = 1 - S_k / n_eff(k) over the window of k* only.  |pv - dist| <= WINDOW_MARGIN
//     (= the direct filter's error budget, sc_filter.hip: 2u + u^2 from the fp16 operands + 1200 * 2^-23 from the fp32
//     accumulation + epilogue < 1.13e-3; shifts without an effective column are ignored on both sides).
// Hand-over: the kernel ends by taking tau_ub_w, the k-th smallest pv + margin over all its records of the query, and writing the
// positions that can still reach it as a dense survivor list behind a header (WindowSurvivor / WindowListHeader, sc_kernels.h),
// which is all sc_rescore_wave_kernel reads of the head of the list.
// Cost: 8192 queries x ~146 entries = 1.2 M pairs at 174 MFMAs per 32 = 0.21 Tflop: ~0.1 ms of matrix-core time against
// the ~1.2 ms of VALU time it replaces.  The entries are gathered (2400 + 256 B each, whole rows of the entry-major
// image hnR): 3.1 GB per batch out of a 27 MB database image, i.e. from L2 / MALL -- which is what bounds the kernel
// (0.36 ms).
// What its time follows (round 10, the region timers below; DESIGN.md "Where round 10 points"): the work the four resident
// workgroups of a CU put through its gather and VALU pipes, NOT the length of one workgroup's dependent chain -- a
// cooperative pass 2 cut the chain by 16 % and the kernel by 1 %, and a split that gathered every B fragment twice made it
// slower.  So the kernel does nothing twice: the list's records are loaded once, with the query (they reach do_group, the
// pass-2 selection and the tail through LDS), the head's ranking is shared by the four waves instead of repeated by each,
// the epilogue and the alignment use the lean forms of sc_window_dev.h (identical values), and the key copies are laid
// out without index divisions.
//
// Error bound of KC (scaled keys x, max |x| in [2^9, 2^10); E = sum x^2):
//   representation  x = hi + lo + r, |r| <= 2^-22 |x| (+ 2^-25 absolute where lo is subnormal)
//   dropped lo*lo   <= 2^-22 |x||y| per term
//   fp32 accumulation of 3 x 64 products in 12 chained MFMAs: <= 192 * 2^-23 relative to sum |terms| <= sqrt(E_q E_e)
//   total < (2.29e-5 + 4 * 2.4e-7) sqrt(E_q E_e);  kWinAlignEps = 3e-5 with sqrt(E) rounded up.
// Two quirks of the reference's search bound where this applies (split_key / `balanced` below): it starts from a best
// distance of 1e7 (keys with norms >= 4e6 are declined), and it works in fp64 on UNSCALED keys (pairs whose key norms
// differ by more than 1e6 are declined).
// A shift other than the true argmax can only reach KC_max - 2 eps sqrt(E_q E_e) when the true values are that close,
// so a unique candidate above that line IS the reference's argmin (whose fp64 arithmetic is off by < 1e-13 relative).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "rsx_common.h"
#include "sc_kernels.h"
#include "sc_entry_dev.h"
#include "sc_window_dev.h"

namespace rsx {
namespace sc {

namespace {

using win::half8;
using win::floatx16;
using win::u64;
using win::kNonFinite;
using win::W_STEPS;
using win::W_TILE1;
using win::QK_COPY;
using win::QK_LO;
using win::QK_NORM;
using win::W_LDS;

// the prologue's staging area inside the per-position arrays (s_rec): the normalised columns, the doubled key, the column mask
constexpr int W_ST2_OFF = DS * 2, W_QM_OFF = W_ST2_OFF + 2 * 128 * 2;
static_assert(W_ST2_OFF % 16 == 0 && W_QM_OFF % 8 == 0 && W_QM_OFF + 8 <= 5 * WINDOW_P * 4, "staging fits the arrays it aliases");

#ifndef WIN_OCC
#define WIN_OCC 4  // waves per SIMD the register budget is set for
#endif
#ifndef WIN_RING
#define WIN_RING 15  // B fragments of the image GEMM in flight per wave
#endif
// Region timers of the kernel's dependent chain: -DRSX_WINDOW_PROF=1 (tools/build_window_prof.sh; neither the product nor the
// experiments build has them).  Every wave sums s_memtime differences per region -- each lap drains the wave's own memory and
// LDS queues first, so a region owns the latency it started -- and adds them to block (query % WIN_PROF_COPIES) of a buffer
// that launch_window prints after every launch (it synchronises the stream: a profiling build).
#ifdef RSX_WINDOW_PROF
constexpr bool kWinProf = true;
#else
constexpr bool kWinProf = false;
#endif
enum WinProfRegion {
  WP_PROLOGUE = 0,  // start .. the images stand in LDS (the loads of the query and of the list records included)
  WP_GROUP1,        // the wave's pass-1 group
  WP_RANK,          // tau_ub of the head by counting
  WP_SELECT,        // which positions behind the head get a record (wave 0)
  WP_GROUP2,        // the pass-2 groups
  WP_TAIL,          // write_list
  WP_BARRIER,       // waiting at the workgroup's barriers
  WP_TOTAL,
  WP_COUNT,         // waves that reported (one per workgroup and wave index)
  WP_GROUPS2,       // pass-2 groups the wave took part in
  WIN_PROF_WORDS
};
constexpr int WIN_PROF_COPIES = 64;
// ------------------------------------------------------------------------------------------
// database side: [slot][hi 0..63 | lo 0..63] fp16 (elements 60..63 zero: the K padding) + the key's scaled norm
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sc_win_db_keys_kernel(const double *__restrict__ vkey, int64_t first, int64_t count,
                                                             _Float16 *__restrict__ vk16, float *__restrict__ vk_n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t it = (int64_t)blockIdx.x * 4 + wave;
  if (it >= count) return;
  dev::win_db_keys_entry(vkey, first + it, vk16, vk_n, lane);
}

// ------------------------------------------------------------------------------------------
// the window kernel: one workgroup per query, wave w takes short-list positions 32 w .. 32 w + 31 (then + 128, ...)
// ------------------------------------------------------------------------------------------
struct WindowArgs {
  const char *hnR;
  const char *vk16;
  const float *vk_n;
  const u64 *cmask;
  const float *qdesc;   // [nq][DS]: the queries; their two images are built in LDS by the kernel's prologue
  const double *qnorm;  // [nq][NS]
  const double *qvkey;  // [nq][NS]
  const RescoreEntry *slist;
  const int32_t *sl_cnt;
  WindowPreview *out;
  WindowSurvivor *surv;  // [nq][WINDOW_LIST_STRIDE]: header + survivor list of every query
  double eps;  // the filter's error budget, as the re-scoring kernel applies it to a bound
  int32_t k;
  unsigned long long *prof;  // RSX_WINDOW_PROF builds: [WIN_PROF_COPIES][4 waves][WIN_PROF_WORDS], else nullptr
};

__global__ __launch_bounds__(256, WIN_OCC) void sc_window_kernel(WindowArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float s_ub[WINDOW_HEAD];
  __shared__ int s_pos[WINDOW_P];
  __shared__ int s_n2;
  __shared__ float s_tau;  // the head's k-th smallest upper bound: from the lane that ranks it to the selection and the tail
  // what the workgroup knows of list position p once its group is done (filter bound, slot, preview, k* | shift mask); the
  // positions no group takes are never read: they are not survivors
  // (one block, because the prologue stages the query in it before the first group touches any of the five)
  __shared__ __attribute__((aligned(16))) char s_rec[5 * WINDOW_P * 4];
  float *const s_lb = reinterpret_cast<float *>(s_rec), *const s_pv = s_lb + WINDOW_P, *const s_cand = s_pv + WINDOW_P;
  int *const s_slot = reinterpret_cast<int *>(s_cand + WINDOW_P), *const s_ks = s_slot + WINDOW_P;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: group counters in SGPRs)
  const int qi = blockIdx.x;
  // region timers (kWinProf): wave-uniform, so they live in SGPRs; nothing of them is compiled into the product
  long long t_mark = 0, t_begin = 0, tacc[WP_TOTAL] = {0, 0, 0, 0, 0, 0, 0};
  int prof_groups2 = 0;
  if constexpr (kWinProf) t_begin = t_mark = clock64();
  auto lap = [&](int region) {
    if constexpr (kWinProf) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      const long long t = clock64();
      tacc[region] += t - t_mark;
      t_mark = t;
    }
  };
  auto barrier = [&](int region) {  // the region up to the barrier, then the wait
    lap(region);
    __syncthreads();
    lap(WP_BARRIER);
  };
  auto prof_flush = [&]() {
    if constexpr (kWinProf) {
      if (a.prof && lane == 0) {
        unsigned long long *o = a.prof + ((size_t)(qi % WIN_PROF_COPIES) * 4 + wave) * WIN_PROF_WORDS;
#pragma unroll
        for (int r = 0; r < WP_TOTAL; r++) atomicAdd(o + r, (unsigned long long)tacc[r]);
        atomicAdd(o + WP_TOTAL, (unsigned long long)(t_mark - t_begin));
        atomicAdd(o + WP_COUNT, 1ull);
        atomicAdd(o + WP_GROUPS2, (unsigned long long)prof_groups2);
      }
    }
  };
  // the query's descriptor column / norm (wave 0) and sector key (wave 1) are requested together with sl_cnt: nothing of the
  // prologue waits for the list length before its own round trip is on the way
  float4 qcol[5] = {};
  double qn = 0.0, qv = 0.0;
  if (wave == 0) {
    if (lane < NS) {
      const float4 *p = reinterpret_cast<const float4 *>(a.qdesc + (int64_t)qi * DS + lane * NR);
#pragma unroll
      for (int i = 0; i < 5; i++) qcol[i] = p[i];
      qn = a.qnorm[(int64_t)qi * NS + lane];
    }
  } else if (wave == 1) {
    if (lane < NS) qv = a.qvkey[(int64_t)qi * NS + lane];
  }
  // ... and so are the list records {lb, slot} of every position the kernel may look at, one or two per thread (one 8-byte
  // load each), whatever the list's length: the record array has RESCORE_SHORTLIST_CAP >= WINDOW_P slots per query, and what
  // lies behind min(sl_cnt, WINDOW_P) is dropped below.  They stay in registers across the prologue: do_group, the pass-2
  // selection and the tail read slots and bounds from LDS, so none of them starts with a round trip to the list.
  static_assert(WINDOW_P <= 2 * 256 && WINDOW_P <= RESCORE_SHORTLIST_CAP, "two positions per thread, inside the query's records");
  uint2 rec0, rec1 = {0u, 0u};
  {
    const uint2 *sl2 = reinterpret_cast<const uint2 *>(a.slist + (int64_t)qi * RESCORE_SHORTLIST_CAP);
    rec0 = sl2[threadIdx.x];
    if (threadIdx.x + 256 < WINDOW_P) rec1 = sl2[threadIdx.x + 256];
  }
  const int sl_cnt = a.sl_cnt[qi];
  WindowSurvivor *list = a.surv + (int64_t)qi * WINDOW_LIST_STRIDE;
  if (sl_cnt <= 0) {  // uniform; the re-scoring kernel still reads the header
    if (threadIdx.x == 0) {
      WindowListHeader h;
      h.count = 0;
      h.tau_ub = INFINITY;
      h.n_cand = 0;
      h.n_prev = 0;
      *reinterpret_cast<WindowListHeader *>(list) = h;
    }
    return;
  }
  // the list records: s_slot lies behind the staging area and is filled before the prologue's second barrier; s_lb aliases the
  // staging area and is filled behind that barrier (its first reader sits behind the barrier of pass 1)
  static_assert(3 * WINDOW_P * 4 >= W_QM_OFF + 8, "s_slot clear of the staging area");
  const int lim = sl_cnt < WINDOW_P ? sl_cnt : WINDOW_P;
  // ---- the query's two images, built here from its descriptor, column norms and sector key (what sc_img_query_kernel and a
  // key-image kernel used to write to global memory for this kernel to copy back): wave 0 the normalised columns and the
  // column mask, wave 1 the doubled hi / lo key, into the staging area; then every thread a share of the two displaced image
  // copies and the 16 displaced key copies.  Element for element the arithmetic of dev::normalise_column / split_key ----
  {
    _Float16 *st = reinterpret_cast<_Float16 *>(s_rec);                                        // DS halves
    _Float16(*st2)[128] = reinterpret_cast<_Float16(*)[128]>(s_rec + W_ST2_OFF);               // 2 x 128 halves
    u64 *s_qm = reinterpret_cast<u64 *>(s_rec + W_QM_OFF);
    dev::KeySplit ksplit{};
    if (wave == 0) {
      bool nonzero = false, bad = false;
      if (lane < NS) dev::normalise_column_regs(qcol, qn, &st[lane * NR], nonzero, bad);
      u64 m = __ballot(nonzero && lane < NS);
      if (__ballot(bad && lane < NS)) m |= kNonFinite;
      if (lane == 0) *s_qm = m;
    } else if (wave == 1) {
      ksplit = win::query_keys_stage(lane < NS ? qv : 0.0, st2, lane);
    }
    barrier(WP_PROLOGUE);
    dev::img_query_image(st, *s_qm, reinterpret_cast<uint4 *>(smem), threadIdx.x, 256);
    win::query_keys_copies_256(st2, smem + FILTER_QIMG_BYTES, threadIdx.x);
    if (wave == 1) win::query_keys_norms(ksplit, smem + FILTER_QIMG_BYTES, lane);
  }
  if ((int)threadIdx.x < lim) s_slot[threadIdx.x] = (int)rec0.y;
  if ((int)threadIdx.x + 256 < lim) s_slot[threadIdx.x + 256] = (int)rec1.y;
  barrier(WP_PROLOGUE);
  if ((int)threadIdx.x < lim) s_lb[threadIdx.x] = __uint_as_float(rec0.x);
  if ((int)threadIdx.x + 256 < lim) s_lb[threadIdx.x + 256] = __uint_as_float(rec1.x);
  const int n = lane & 31, hh = lane >> 5;
  const u64 qm = *reinterpret_cast<const u64 *>(smem + FILTER_QIMG_MASK_OFF);
  const float nq_key = *reinterpret_cast<const float *>(smem + FILTER_QIMG_BYTES + QK_NORM);
  const float uq_key = *reinterpret_cast<const float *>(smem + FILTER_QIMG_BYTES + QK_NORM + 4);
  // A-fragment addresses of this lane's row (shift n of tile 0; tile 1 = the same address + 40 K-steps, sc_filter.hip)
  const char *ap = smem + ((n & 1) ? (FILTER_QIMG_ODD + 40 * n - 8) : (40 * n)) + 16 * hh;
  const char *kp = smem + FILTER_QIMG_BYTES + (n & 7) * QK_COPY + ((n & ~7) + 8 * hh) * 2;  // tile 1: + 64 B

  // the lane index as a value the compiler cannot follow: what is derived from it is computed again where it is used instead
  // of being carried (and spilled) across the K loops
  auto lane_again = [&]() -> int {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t & 31;
  };
  // one group of 32 short-list entries (lane n and n + 32: entry at list position pos_of(); have = the lane has one, else it
  // shadows position pos_any): writes the record, returns the upper bound of the pair distance the record implies
  auto do_group = [&](auto pos_of, bool have, int pos_any) -> float {
    const int64_t slot = s_slot[have ? pos_of() : pos_any];
    // the entry's column mask and key norms go out with the key rows, in front of the K loop (two registers across it)
    const u64 em = a.cmask[slot];
    const float2 en = reinterpret_cast<const float2 *>(a.vk_n)[slot];

    // ---- alignment: 2 tiles x (hi*hi + hi*lo + lo*hi) x 4 K-steps ----
    floatx16 k0 = {0}, k1 = {0};
    {
      const char *bk = a.vk16 + slot * 256 + 16 * hh;
      half8 bh[4], bl[4];
#pragma unroll
      for (int s = 0; s < 4; s++) {
        bh[s] = *reinterpret_cast<const half8 *>(bk + 32 * s);
        bl[s] = *reinterpret_cast<const half8 *>(bk + 128 + 32 * s);
      }
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const half8 ah0 = *reinterpret_cast<const half8 *>(kp + 32 * s);
        const half8 al0 = *reinterpret_cast<const half8 *>(kp + QK_LO + 32 * s);
        const half8 ah1 = *reinterpret_cast<const half8 *>(kp + 64 + 32 * s);
        const half8 al1 = *reinterpret_cast<const half8 *>(kp + QK_LO + 64 + 32 * s);
        k0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah0, bh[s], k0, 0, 0, 0);
        k1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah1, bh[s], k1, 0, 0, 0);
        k0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah0, bl[s], k0, 0, 0, 0);
        k1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah1, bl[s], k1, 0, 0, 0);
        k0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al0, bh[s], k0, 0, 0, 0);
        k1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al1, bh[s], k1, 0, 0, 0);
      }
    }
    u64 win;    // the union of the windows of the admissible alignments
    int kstar;  // the alignment when exactly one shift is admissible, else -1
    // (the lean forms of sc_window_dev.h, here and in the epilogue: the same values as the plain ones with a third of the VALU
    // instructions -- the kernel's time follows its instruction count, not the length of a workgroup's chain: file header)
    win::alignment_of<true>(k0, k1, nq_key, uq_key, en, hh, win, kstar);

    // ---- the 60 correlation values of the two images (the direct filter's GEMM) ----
    __builtin_amdgcn_sched_barrier(0);  // keep the loads below from being hoisted over the alignment (register pressure)
    floatx16 acc0 = {0}, acc1 = {0};
    {
      const char *brow = a.hnR + slot * (2 * DS) + 16 * hh;
      // B fragments (16 bytes per lane from 32 different rows) through a ring of WIN_RING registers sets: a slot is
      // refilled right after its MFMAs, so WIN_RING - 1 gathers per wave are in flight all the time (two buffers of five,
      // the first version, had 5..10: the kernel is bound by the latency x concurrency of this gather, not by the MFMAs)
      constexpr int R = WIN_RING;
      static_assert(W_STEPS % R == 0, "whole ring turns");
      half8 ring[R];
#pragma unroll
      for (int u = 0; u < R; u++) ring[u] = *reinterpret_cast<const half8 *>(brow + 32 * u);
#pragma unroll 1
      for (int s0 = 0; s0 < W_STEPS - R; s0 += R) {
#pragma unroll
        for (int u = 0; u < R; u++) {
          const half8 a0 = *reinterpret_cast<const half8 *>(ap + 32 * (s0 + u));
          const half8 a1 = *reinterpret_cast<const half8 *>(ap + 32 * (s0 + u + W_TILE1));
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, ring[u], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, ring[u], acc1, 0, 0, 0);
          ring[u] = *reinterpret_cast<const half8 *>(brow + 32 * (s0 + R + u));
        }
      }
#pragma unroll
      for (int u = 0; u < R; u++) {  // the last turn: nothing left to request
        const half8 a0 = *reinterpret_cast<const half8 *>(ap + 32 * (W_STEPS - R + u));
        const half8 a1 = *reinterpret_cast<const half8 *>(ap + 32 * (W_STEPS - R + u + W_TILE1));
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, ring[u], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, ring[u], acc1, 0, 0, 0);
      }
    }

    // ---- epilogue: max of S_k / n_eff(k) over the window of k* (n_eff from the two column masks, as the filter) ----
    __builtin_amdgcn_sched_barrier(0);
    // (the query mask as a value the compiler cannot follow: its rotations are then formed here, per group, instead of once
    // before pass 2 -- a dozen registers that did not fit and were spilled)
    u64 qmg = qm;
    asm volatile("" : "+v"(qmg));
    const float pv = win::preview_of<true>(acc0, acc1, qmg, em, win, kstar, hh);
    if (have && hh == 0) {
      const int pos = pos_of();
      WindowPreview o;
      o.pv = pv;
      o.ks = kstar;
      a.out[(int64_t)qi * WINDOW_P + pos] = o;
      s_pv[pos] = pv;
      s_ks[pos] = kstar;
    }
    return (have && kstar >= 0 && pv < 3.0e38f) ? pv + WINDOW_MARGIN : INFINITY;  // NaN fails the compare
  };

  // ---- the tail (wave 0, after a barrier behind the last group): tau_ub_w = the k-th smallest upper bound over ALL records
  // of the query, then the survivor list and its header.  tau_head: the k-th smallest upper bound of the head (+inf: not
  // known) -- at least k upper bounds lie at or below it, so the k-th smallest of all is among those ----
  auto write_list = [&](float tau_head, int n2) {
    const int nh = lim < WINDOW_HEAD ? lim : WINDOW_HEAD;
    const unsigned long long below = (1ull << lane) - 1ull;
    // the positions with a record, 64 at a time: the head, then what pass 2 admitted (s_pos); f(position, the lane has one)
    auto records = [&](auto f) {
      for (int p0 = 0; p0 < nh; p0 += 64) f(p0 + lane, p0 + lane < nh);
      for (int c0 = 0; c0 < n2; c0 += 64) f(c0 + lane < n2 ? s_pos[c0 + lane] : 0, c0 + lane < n2);
    };
    int nc = 0;
    records([&](int pos, bool in) {
      const float pv = s_pv[pos];
      const float ub = pv + WINDOW_MARGIN;
      const bool c = in && s_ks[pos] >= 0 && pv < 3.0e38f && ub <= tau_head;  // NaN fails the compares
      const unsigned long long bal = __ballot(c);
      if (c) s_cand[nc + __popcll(bal & below)] = ub;
      nc += __popcll(bal);
    });
    wave::lds_fence();
    float tau_w = INFINITY;
    if (nc >= a.k) {  // rank by counting, as for the head; the ranks are a permutation of 0 .. nc - 1
      for (int c0 = 0; c0 < nc; c0 += 64) {
        const int i = c0 + lane;
        const float v = i < nc ? s_cand[i] : INFINITY;
        int r = 0;
        for (int j = 0; j < nc; j++) {
          const float x = s_cand[j];
          r += (x < v || (x == v && j < i)) ? 1 : 0;
        }
        const unsigned long long b = __ballot(i < nc && r == a.k - 1);
        if (b) {
          tau_w = __shfl(v, __ffsll((long long)b) - 1);
          break;
        }
      }
    }
    int ns = 0, n_cand = 0, n_prev = 0;
    records([&](int pos, bool in) {
      const float pv = s_pv[pos];
      const int ks = s_ks[pos];
      const bool none = in && !(pv == pv);  // no preview (non-finite data): must be looked at
      const bool lb_ok = !((double)s_lb[pos] - a.eps > (double)tau_w);  // NaN / -inf bounds: always
      const bool cand = in && (none || (pv < INFINITY && lb_ok));  // +inf: no effective column in the window, never a hit
      const float lo = none ? -INFINITY : pv - WINDOW_MARGIN;
      const bool sv = cand && !(lo > tau_w);
      const unsigned long long bal = __ballot(sv);
      if (sv) {
        WindowSurvivor e;
        e.lo = lo;
        e.slot = s_slot[pos];
        e.ks = (none || ks < 0) ? -1 : ks;
        e.pos = pos;
        list[1 + ns + __popcll(bal & below)] = e;
      }
      ns += __popcll(bal);
      n_cand += __popcll(__ballot(cand));
      n_prev += __popcll(__ballot(cand && !none));
    });
    if (lane == 0) {
      WindowListHeader h;
      h.count = ns;
      h.tau_ub = tau_w;
      h.n_cand = n_cand;
      h.n_prev = n_prev;
      *reinterpret_cast<WindowListHeader *>(list) = h;
    }
  };

  // ---- pass 1: the head of the list ----
  float tau_ub;
  {
    const int cnt1 = sl_cnt < WINDOW_HEAD ? sl_cnt : WINDOW_HEAD;
    float ub = INFINITY;
    if (wave * 32 < cnt1) ub = do_group([&] { return wave * 32 + lane_again(); }, wave * 32 + n < cnt1, wave * 32);
    if (hh == 0) s_ub[wave * 32 + n] = ub;
    barrier(WP_GROUP1);
    if (sl_cnt <= WINDOW_HEAD) {  // uniform
      if (wave == 0) write_list(INFINITY, 0);
      lap(WP_TAIL);
      prof_flush();
      return;
    }

    // ---- the k-th smallest upper bound of the head: an upper bound of the final k-th best distance.  Only entries whose
    // filter bound does not exceed it can matter to the re-scoring kernel (whose own bound is at least as tight).  Rank by
    // counting, shared by the workgroup: wave w ranks its own 32 values, the two lane halves against one half of the head
    // each (every wave used to rank all 128 for itself, and only wave 0 wanted the result) ----
    {
      const int p = wave * 32 + n;
      const float v = s_ub[p];
      int r = 0;
      const float4 *u4 = reinterpret_cast<const float4 *>(s_ub) + (WINDOW_HEAD / 8) * hh;
#pragma unroll 4
      for (int j = 0; j < WINDOW_HEAD / 8; j++) {
        const float4 u = u4[j];
        const float x[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int idx = (WINDOW_HEAD / 2) * hh + 4 * j + e;
          r += (x[e] < v || (x[e] == v && idx < p)) ? 1 : 0;
        }
      }
      r += __shfl_xor(r, 32);
      // 0 <= k - 1 < WINDOW_HEAD (k <= RSX_SC_MAX_TOPK) and the ranks are a permutation of 0..127: one lane of the workgroup
      if (hh == 0 && r == a.k - 1) s_tau = v;
    }
    barrier(WP_RANK);
    tau_ub = s_tau;
  }
  // ---- pass 2: list positions WINDOW_HEAD .. WINDOW_P - 1 whose bound can still matter; the others get "no record" ----
  if (wave == 0) {
    int n2 = 0;
    for (int p0 = WINDOW_HEAD; p0 < lim; p0 += 64) {
      const int pos = p0 + lane;
      bool pass = false;
      if (pos < lim) {
        const float lb = s_lb[pos];
        pass = !((double)lb - a.eps > (double)tau_ub);  // NaN / -inf bounds: always
        if (!pass) {
          WindowPreview o;
          o.pv = __builtin_nanf("");
          o.ks = -2;
          a.out[(int64_t)qi * WINDOW_P + pos] = o;
        }
      }
      const unsigned long long bal = __ballot(pass);
      if (pass) s_pos[n2 + __popcll(bal & ((1ull << lane) - 1ull))] = pos;
      n2 += __popcll(bal);
    }
    if (lane == 0) s_n2 = n2;
  }
  barrier(WP_SELECT);
  const int n2 = s_n2;
  for (int g = wave; g * 32 < n2; g += 4) {
    const bool have = g * 32 + n < n2;
    (void)do_group([&] { return s_pos[g * 32 + lane_again()]; }, have, s_pos[g * 32]);  // (only lanes that have one ask)
    prof_groups2++;
  }
  barrier(WP_GROUP2);
  if (wave == 0) write_list(s_tau, n2);
  lap(WP_TAIL);
  prof_flush();
}

}  // namespace

int launch_window_db_keys(const double *vkey, int64_t first, int64_t count, void *vk16, float *vk_n, hipStream_t s) {
  if (count <= 0) return RSX_OK;
  hipLaunchKernelGGL(sc_win_db_keys_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, vkey, first, count,
                     static_cast<_Float16 *>(vk16), vk_n);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

int launch_window(const DbView &db, const QueryView &q, const RescoreEntry *slist, const int32_t *sl_cnt,
                  int32_t k, double eps, WindowPreview *out, WindowSurvivor *surv, hipStream_t s) {
  if (q.nq <= 0) return RSX_OK;
  WindowArgs a;
  a.hnR = static_cast<const char *>(db.hnR);
  a.vk16 = static_cast<const char *>(db.vk16);
  a.vk_n = db.vk_n;
  a.cmask = reinterpret_cast<const u64 *>(db.cmask);
  a.qdesc = q.desc;
  a.qnorm = q.norm;
  a.qvkey = q.vkey;
  a.slist = slist;
  a.sl_cnt = sl_cnt;
  a.out = out;
  a.surv = surv;
  a.eps = eps;
  a.k = k < 1 ? 1 : (k > WINDOW_HEAD ? WINDOW_HEAD : k);
  a.prof = nullptr;
#ifdef RSX_WINDOW_PROF
  constexpr size_t kProfWords = (size_t)WIN_PROF_COPIES * 4 * WIN_PROF_WORDS;
  static unsigned long long *d_prof = nullptr;  // (a profiling build: one device, one launch at a time, never freed)
  if (!d_prof) RSX_HIP(hipMalloc(reinterpret_cast<void **>(&d_prof), kProfWords * 8));
  RSX_HIP(hipMemsetAsync(d_prof, 0, kProfWords * 8, s));
  a.prof = d_prof;
#endif
  hipLaunchKernelGGL(sc_window_kernel, dim3((unsigned)q.nq), dim3(256), W_LDS, s, a);
  RSX_HIP(hipGetLastError());
#ifdef RSX_WINDOW_PROF
  {
    static unsigned long long h[kProfWords];
    RSX_HIP(hipMemcpyAsync(h, d_prof, kProfWords * 8, hipMemcpyDeviceToHost, s));
    RSX_HIP(hipStreamSynchronize(s));
    static const char *const names[WP_TOTAL + 1] = {"prologue", "pass-1 group", "ranking", "pass-2 selection", "pass-2 groups", "tail", "barriers", "total"};
    for (int w = 0; w < 4; w++) {
      double v[WIN_PROF_WORDS] = {0};
      for (int c = 0; c < WIN_PROF_COPIES; c++)
        for (int i = 0; i < WIN_PROF_WORDS; i++) v[i] += (double)h[((size_t)c * 4 + w) * WIN_PROF_WORDS + i];
      if (v[WP_COUNT] <= 0) continue;
      fprintf(stderr, "[sc_window prof] nq %d wave %d (cycles per workgroup, %.0f reported, %.3f pass-2 groups):", (int)q.nq, w, v[WP_COUNT], v[WP_GROUPS2] / v[WP_COUNT]);
      for (int r = 0; r <= WP_TOTAL; r++) fprintf(stderr, "  %s %.0f", names[r], v[r] / v[WP_COUNT]);
      fprintf(stderr, "\n");
    }
  }
#endif
  return RSX_OK;
}

const char *window_kernel_name() { return "sc_window_kernel"; }

}  // namespace sc
}  // namespace rsx
