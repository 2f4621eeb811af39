// pmc.hip -- max-clique inlier selection on gfx950: the stage between the matcher and the ORORA solver ("PMC max-clique
// prune").  Upstream takes it from TEASER++ / the PMC library; neither is in the reference
// checkout (the ORORA submodule is an empty directory: /root/reference/.gitmodules:1-3, README.md:19,26-29), so this follows
// the construction restated in oracle/pmc_ref.{h,c} -- PARITY UNPINNED -- and reproduces that oracle's selection exactly.
//
//   consistency graph   vertices = the K matches of a pair; i ~ j iff | ||src_i - src_j|| - ||dst_i - dst_j|| | < tau, evaluated
//                       without square roots in fp64 (pmc_ref.h: s = (A + B) - tau^2; edge <=> s < 0 || s^2 < 4 A B)
//   core numbers        level-synchronous peeling (exact; the result is unique)
//   greedy clique       seeds and candidates in (core descending, index ascending) order, <= MAX_SEEDS seeds
//
// Mapping.  A VERTEX SET IS ONE REGISTER PER LANE OF A WAVEFRONT: 64 lanes x 32 bits = 2048 vertices, vertex u = bit u / 64 of
// lane u % 64 (lane-interleaved, so that lane l of the adjacency build reads points l, 64 + l, ...: consecutive LDS
// addresses).  Set intersection = one v_and against a 256-byte adjacency row (one coalesced load), |P| = v_bcnt + a wave
// reduction, "is u in P" = v_readlane + shift.  The adjacency of a pair lives in a 512 KB slab of HBM (written once, read
// once by the peeling and once per picked vertex).  Three kernels per chunk of <= CHUNK pairs, each with the shape ITS phase
// wants (the first build ran all phases in one 256-thread workgroup per pair with 45 KB of LDS: three workgroups per CU, during
// the walk one of their twelve wavefronts at work, every predicate in fp64 -- 6.6 ms per 3 500 pairs; now 3.8):
//   pmc_build_kernel   a workgroup per block of 256 ROWS of a pair (the cost of a pair goes with K^2: whole pairs left the chip
//                      at 1.9 of 4 waves per SIMD), points in LDS: row i of the graph per wave iteration, 64 lanes x
//                      ceil(K / 64) columns of the predicate -- decided in fp32 wherever fp32 can, edge_f32 -- two columns per
//                      step with the next two on their way -> one word per lane -> one 256-byte row store; degree by popcount
//   pmc_cores_kernel   256 threads: core numbers by level-synchronous peeling -- frontier = alive vertices of degree <=
//                      level (all threads), the frontier rows & alive decrement their neighbours' degrees (LDS atomics, four
//                      rows in flight per wave); empty frontier -> level = the smallest remaining degree -- then a bitonic
//                      sort of (2047 - core) << 11 | index in LDS -> `order`
//   pmc_walk_kernel    ONE WAVEFRONT per pair (up to 20 pairs per CU): the greedy walk.  64 candidates of `order` are
//                      tested against P at once (ds_bpermute + ballot), the rows of the next eight members are loaded
//                      together, each is re-tested against the shrinking P before it joins; then member flags, the selected
//                      matches compacted in their original order for the solver, one info record
//   pmc_exact_kernel   (only with RSX_ORORA_PMC_EXACT, after the walk) core pruning, universal vertices, then a branch-and-bound
//                      search of the residual graph in rank order: a maximum clique per pair, see the comment above it
// Roofline: the build is VALU-issue bound (SQ_ACTIVE_INST_VALU = 100 % of the SIMD cycles at ~31 instructions per pair of
// matches: 2.4 of the 3.8 ms); peeling and walk are dependent chains per pair (barrier / load row -> and -> popcount) that last
// as long as the longest pair's, hidden by the number of pairs in flight (0.9 + 0.6 ms).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pmc.h"
#include "rsx_wave_dev.h"

namespace {

using rsx::pmc::MAX_K;
using rsx::pmc::MAX_SEEDS;
constexpr int NT = 256;
constexpr int ROWW = 64;  // words per adjacency row
// per-pair record between the kernels: core numbers, the order, the degrees, the largest core number
constexpr int META_CORE = 0, META_ORDER = 2 * MAX_K, META_DEG = 4 * MAX_K, META_HDR = 8 * MAX_K;
constexpr int META_BYTES = rsx::pmc::META_BYTES;
static_assert(META_HDR + 64 <= META_BYTES, "meta layout");

struct Args {
  const float2 *src, *dst;
  const int64_t *offsets;
  int n_pairs, first;  // this launch: pairs [first, first + gridDim.x)
  double tau2;
  uint32_t *slabs;     // [chunk][MAX_K][ROWW]
  char *meta;          // [chunk][META_BYTES]
  uint8_t *member;
  rsx_orora_pmc_info *info;
  float2 *sel_src, *sel_dst;
  int32_t *sel_cnt;
  int64_t sel_cap;  // matches the sel arrays hold
};

// the edge predicate of oracle/pmc_ref.h, operation for operation (this file is compiled with -ffp-contract=off)
__device__ __forceinline__ bool edge(double six, double siy, double dix, double diy, float2 sj, float2 dj, double tau2) {
  const double dax = (double)sj.x - six, day = (double)sj.y - siy;
  const double dbx = (double)dj.x - dix, dby = (double)dj.y - diy;
  const double A = dax * dax + day * day;
  const double B = dbx * dbx + dby * dby;
  const double sm = (A + B) - tau2;
  return (sm < 0.0) || (sm * sm < 4.0 * (A * B));
}

// the pair of this workgroup: false = not pruned (fewer than 2 / more than MAX_K matches / no room in the sel arrays)
struct Pair {
  int pair, K;
  int64_t o, K64;
  bool no_room;
};
__device__ __forceinline__ bool pair_of(const Args &a, Pair &p) {
  p.pair = a.first + (int)blockIdx.x;
  p.o = a.offsets[p.pair];
  p.K64 = a.offsets[p.pair + 1] - p.o;
  p.no_room = a.sel_src && p.o + p.K64 > a.sel_cap;
  p.K = (int)p.K64;
  return !(p.K64 < 2 || p.K64 > MAX_K || p.no_room);
}

// Everything a whole wavefront decides goes through an SGPR (readfirstlane): hipcc cannot see that `wave`, or a value every
// thread read from the same LDS word, is uniform, and structurises such branches with exec masks -- the first build of the
// peeling loop `if (tid == 0) L.level = m; continue;` parked lane 0's store behind a loop the other 63 lanes of its wave
// could not leave without it (the kernel never returned).  Uniform values in SGPRs make those branches scalar.

// The same predicate decided in fp32 wherever fp32 can decide it (round 6).  The fp64 form alone made the build 5.2 ms of a
// 7.9 ms selection -- not for its fp64 rate but for its instruction count: a wave64 VALU instruction is 4 cycles of its SIMD
// (SQ_ACTIVE_INST_VALU = SQ_INSTS_VALU quad-cycles) and the step was 36 of them.  In fp32, with u = 2^-24: A, B carry a relative
// error <= 4.2 u, v_sqrt_f32 is good to 1 ulp (2 u), so da = sqrt A, db = sqrt B are within 4.1 u of the true distances and
// x = da - db within 4.1 u (da + db) + u |x| of the true difference.  Hence, with e = 8 u (da + db):
//     |x| + e < tau (1 - 4 u)   =>  edge,        |x| - e > tau (1 + 4 u)   =>  no edge
// (tau as a float is within u of the bound, u |x| ~ u tau; the fp64 form of oracle/pmc_ref.h errs by ~1e-16; slack ~4 u (da + db)).
// Whatever is left -- pairs within ~3e-4 m of the bound at 150 m range, NaN coordinates -- takes the fp64 form; a wavefront
// skips it when none of its 64 lanes needs it (tests/test_gpu_pmc.py::test_edges_at_the_bound).
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void edge_f32(f2v si, f2v di, f2v sj, f2v dj, float tau_lo, float tau_hi, bool &yes, bool &no) {
  const f2v da2 = (sj - si) * (sj - si), db2 = (dj - di) * (dj - di);  // (v_pk_add_f32 / v_pk_mul_f32: x and y in one instruction)
  const float A = da2.x + da2.y, B = db2.x + db2.y;                      // relative error <= 4.2 u, as with the fused form
  const float da = __builtin_amdgcn_sqrtf(A), db = __builtin_amdgcn_sqrtf(B);
  const float x = fabsf(da - db), e = (da + db) * 0x1p-21f;
  yes = x + e < tau_lo;
  no = x - e > tau_hi;
}

// pmc_build_kernel: rows [256 blockIdx.y, + 256) of the consistency graph of pair blockIdx.x (rows into the slab, degrees into
// the pair's record).  A workgroup per ROW BLOCK, not per pair: the cost of a pair goes with K^2 (x 25 between 300 and 1500
// matches), and with one workgroup per pair the chip ran at 1.9 of 4 waves per SIMD (SQ_WAVE_CYCLES / GRBM_GUI_ACTIVE) waiting
// for the long ones.  Two columns per step, the next two already on their way from LDS.
constexpr int BUILD_ROWS = 256;
__global__ __launch_bounds__(NT) void pmc_build_kernel(Args a) {
  __shared__ float2 s_src[MAX_K], s_dst[MAX_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  Pair p;
  if (!pair_of(a, p)) return;
  const int K = p.K, nc = (K + 63) >> 6, nc2 = (nc + 1) & ~1;
  const int row0 = (int)blockIdx.y * BUILD_ROWS;
  if (row0 >= K) return;
  const int row1 = row0 + BUILD_ROWS < K ? row0 + BUILD_ROWS : K;
  uint32_t *adj = a.slabs + (size_t)blockIdx.x * (rsx::pmc::SLAB_BYTES / 4);
  int *g_deg = reinterpret_cast<int *>(a.meta + (size_t)blockIdx.x * META_BYTES + META_DEG);
  for (int i = tid; i < nc2 * 64 && i < MAX_K; i += NT) {  // (slots past K hold zeros: finite, and masked below)
    s_src[i] = i < K ? a.src[p.o + i] : float2{0.0f, 0.0f};
    s_dst[i] = i < K ? a.dst[p.o + i] : float2{0.0f, 0.0f};
  }
  __syncthreads();
  const float tau = (float)sqrt(a.tau2), tau_lo = tau * (1.0f - 0x1p-22f), tau_hi = tau * (1.0f + 0x1p-22f);
  uint32_t vm = 0;  // this lane's columns that exist: bit c <=> c * 64 + lane < K
  for (int c = 0; c < nc; c++) vm |= (c * 64 + lane < K) ? (1u << c) : 0u;
  const f2v *v_src = reinterpret_cast<const f2v *>(s_src), *v_dst = reinterpret_cast<const f2v *>(s_dst);
  for (int i = row0 + wave; i < row1; i += NT / 64) {
    const f2v si = v_src[i], di = v_dst[i];
    // columns from the last pair down to the first: a row's word is built by shifting the new bit in from the right
    // (w = w + w + bit: a compare into vcc and one add-with-carry), the pair after next already on its way from LDS
    uint32_t w = 0;
    int c = nc2 - 2;
    f2v sj0 = v_src[c * 64 + lane], dj0 = v_dst[c * 64 + lane], sj1 = v_src[c * 64 + 64 + lane], dj1 = v_dst[c * 64 + 64 + lane];
    for (; c >= 0; c -= 2) {
      const f2v a0 = sj0, b0 = dj0, a1 = sj1, b1 = dj1;
      const int jn = ((c - 2) * 64 + lane) & (MAX_K - 1);  // (the read before the first pair of columns is harmless and unused)
      sj0 = v_src[jn];
      dj0 = v_dst[jn];
      sj1 = v_src[(jn + 64) & (MAX_K - 1)];
      dj1 = v_dst[(jn + 64) & (MAX_K - 1)];
      bool y0, n0, y1, n1;
      edge_f32(si, di, a0, b0, tau_lo, tau_hi, y0, n0);
      edge_f32(si, di, a1, b1, tau_lo, tau_hi, y1, n1);
      if (__ballot(!(y0 || n0) || !(y1 || n1)) != 0ull) {  // (wave-uniform) somebody is too close to the bound for fp32
        const double six = si.x, siy = si.y, dix = di.x, diy = di.y;
        const bool e0 = edge(six, siy, dix, diy, float2{a0.x, a0.y}, float2{b0.x, b0.y}, a.tau2),
                   e1 = edge(six, siy, dix, diy, float2{a1.x, a1.y}, float2{b1.x, b1.y}, a.tau2);
        y0 = (y0 || n0) ? y0 : e0;
        y1 = (y1 || n1) ? y1 : e1;
      }
      w = (w << 2) | (y1 ? 2u : 0u) | (y0 ? 1u : 0u);
    }
    w &= vm;                                                   // columns past K
    if (lane == (i & 63)) w &= ~(1u << (i >> 6));              // no self loop
    adj[(size_t)i * ROWW + lane] = w;
    const int d = rsx::wave::sum_i32(__popc(w));
    if (lane == 0) g_deg[i] = d;
  }
}

struct CoreLds {
  int deg[MAX_K];
  uint32_t keys[MAX_K];    // the sort keys; before the sort: the frontier list (uint16_t[MAX_K])
  uint16_t core[MAX_K];
  uint32_t alive[ROWW];
  int red[4];
  int nfront, level, max_core;
};

__global__ __launch_bounds__(NT) void pmc_cores_kernel(Args a) {
  __shared__ CoreLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  Pair p;
  if (!pair_of(a, p)) return;
  const int K = p.K, nc = (K + 63) >> 6;
  const uint32_t *adj = a.slabs + (size_t)blockIdx.x * (rsx::pmc::SLAB_BYTES / 4);
  char *meta = a.meta + (size_t)blockIdx.x * META_BYTES;
  uint16_t *front = reinterpret_cast<uint16_t *>(L.keys);
  {
    const int *deg = reinterpret_cast<const int *>(meta + META_DEG);
    for (int i = tid; i < K; i += NT) L.deg[i] = deg[i];
  }
  if (tid < ROWW) {
    uint32_t w = 0;  // alive = every vertex < K
    for (int c = 0; c < nc; c++) w |= (c * 64 + tid < K) ? (1u << c) : 0u;
    L.alive[tid] = w;
  }
  if (tid == 0) {
    L.level = 0;
    L.max_core = 0;
  }
  __syncthreads();

  // ---- core numbers by level-synchronous peeling (one exit, three barriers per round) ----
  for (bool peeling = true; peeling;) {
    if (tid == 0) L.nfront = 0;
    __syncthreads();
    const int level = __builtin_amdgcn_readfirstlane(L.level);
    int my_min = 0x7fffffff;
    for (int v = tid; v < K; v += NT) {
      if ((L.alive[v & 63] >> (v >> 6)) & 1u) {
        const int d = L.deg[v];
        if (d <= level) {
          front[atomicAdd(&L.nfront, 1)] = (uint16_t)v;
          L.core[v] = (uint16_t)level;
          atomicAnd(&L.alive[v & 63], ~(1u << (v >> 6)));
        } else {
          my_min = min(my_min, d);
        }
      }
    }
    my_min = rsx::wave::butterfly(my_min, [](int a, int b) { return min(a, b); });
    if (lane == 0) L.red[wave] = my_min;
    __syncthreads();
    const int nf = __builtin_amdgcn_readfirstlane(L.nfront);
    if (nf == 0) {
      const int m = __builtin_amdgcn_readfirstlane(min(min(L.red[0], L.red[1]), min(L.red[2], L.red[3])));
      if (m == 0x7fffffff) peeling = false;  // nothing alive: done
      else if (tid == 0) L.level = m;        // jump to the smallest remaining degree
    } else {
      // four frontier rows per wave in flight (one row after the other made every round a chain of memory latencies)
      for (int f0 = 4 * wave; f0 < nf; f0 += 4 * (NT / 64)) {
        uint32_t wr[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          wr[q] = 0;
          if (f0 + q < nf) {
            const int u = __builtin_amdgcn_readfirstlane((int)front[f0 + q]);
            wr[q] = adj[(size_t)u * ROWW + lane];
          }
        }
        const uint32_t al = L.alive[lane];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          uint32_t w = wr[q] & al;
          while (w) {
            const int c = __ffs((int)w) - 1;
            w &= w - 1;
            atomicSub(&L.deg[c * 64 + lane], 1);
          }
        }
      }
      if (tid == 0) L.max_core = level;  // levels only grow: the last one that removed something is the largest core number
    }
    __syncthreads();  // every wave has read nfront / red and finished its decrements before the next round resets them
  }

  // ---- order = vertices by (core descending, index ascending) ----
  int n2 = 64;
  while (n2 < K) n2 <<= 1;
  for (int i = tid; i < n2; i += NT) L.keys[i] = i < K ? (((uint32_t)(2047 - L.core[i])) << 11) | (uint32_t)i : 0xffffffffu;
  __syncthreads();
  for (int k2 = 2; k2 <= n2; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += NT) {
        const int q = i ^ j;
        if (q > i) {
          const uint32_t x = L.keys[i], y = L.keys[q];
          if (((i & k2) == 0) == (x > y)) {
            L.keys[i] = y;
            L.keys[q] = x;
          }
        }
      }
      __syncthreads();
    }
  uint16_t *g_core = reinterpret_cast<uint16_t *>(meta + META_CORE), *g_order = reinterpret_cast<uint16_t *>(meta + META_ORDER);
  for (int i = tid; i < K; i += NT) {
    g_core[i] = L.core[i];
    g_order[i] = (uint16_t)(L.keys[i] & 2047u);
  }
  if (tid == 0) *reinterpret_cast<int *>(meta + META_HDR) = L.max_core;
}

// (KEEP: the exact mode's instance also leaves the greedy clique -- its 64 words and its size -- in the pair's record, where the
// degrees were; the instance every other call enqueues compiles to what it was)
constexpr int META_KEEP = META_DEG;
template <bool KEEP>
__device__ __forceinline__ void pmc_walk(const Args &a) {
  __shared__ uint16_t s_core[MAX_K], s_order[MAX_K];
  const int lane = threadIdx.x;
  Pair p;
  if (!pair_of(a, p)) {  // nothing to prune with / too large for the stage: every match passes
    if (a.member)
      for (int64_t i = lane; i < p.K64; i += 64) a.member[p.o + i] = 1;
    if (lane == 0) {
      if (a.sel_cnt) a.sel_cnt[p.pair] = -1;  // the solver reads the caller's arrays
      if (a.info)
        a.info[p.pair] = rsx_orora_pmc_info{(int32_t)(p.K64 > 0 ? p.K64 : 0), 0, 0,
                                            RSX_ORORA_PMC_PASSTHROUGH | (p.no_room && p.K64 >= 2 && p.K64 <= MAX_K ? RSX_ORORA_PMC_NO_WORKSPACE : 0)};
    }
    return;
  }
  const int K = __builtin_amdgcn_readfirstlane(p.K), nc = (K + 63) >> 6;
  const uint32_t *adj = a.slabs + (size_t)blockIdx.x * (rsx::pmc::SLAB_BYTES / 4);
  const char *meta = a.meta + (size_t)blockIdx.x * META_BYTES;
  {
    const uint16_t *g_core = reinterpret_cast<const uint16_t *>(meta + META_CORE), *g_order = reinterpret_cast<const uint16_t *>(meta + META_ORDER);
    for (int i = lane; i < K; i += 64) {
      s_core[i] = g_core[i];
      s_order[i] = g_order[i];
    }
  }
  const int max_core = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int *>(meta + META_HDR));
  __syncthreads();

  uint32_t best = 0, cm = 0;
  int best_n = 0, seeds = 0, cm_for = -1;
  for (int t = 0; t < K && seeds < MAX_SEEDS; t++) {
    const int v = __builtin_amdgcn_readfirstlane((int)s_order[t]);
    const int cv = __builtin_amdgcn_readfirstlane((int)s_core[v]);
    if (cv + 1 <= best_n || best_n == max_core + 1) break;
    if ((((uint32_t)__builtin_amdgcn_readlane((int)best, v & 63)) >> (v >> 6)) & 1u) continue;  // a member of the clique in hand
    seeds++;
    if (cm_for != best_n) {  // candidates must have core >= |best|
      cm = 0;
      for (int c = 0; c < nc; c++) {
        const int u = c * 64 + lane;
        if (u < K && (int)s_core[u] >= best_n) cm |= 1u << c;
      }
      cm_for = best_n;
    }
    uint32_t P = adj[(size_t)v * ROWW + lane] & cm;
    uint32_t C = (lane == (v & 63)) ? (1u << (v >> 6)) : 0u;
    int n = 1, np = __builtin_amdgcn_readfirstlane(rsx::wave::sum_i32(__popc(P)));
    bool abandoned = n + np <= best_n;
    for (int s = 0; s < K && np > 0 && !abandoned; s += 64) {
      const int idx = s + lane;
      const int u = idx < K ? (int)s_order[idx] : 0;
      const uint32_t pw = (uint32_t)__shfl((int)P, u & 63);
      unsigned long long mask = __ballot(idx < K && ((pw >> (u >> 6)) & 1u));
      while (mask && np > 0 && !abandoned) {
        // the next (up to) PF candidates of this chunk that were in P when the mask was taken: rows loaded together
        constexpr int PF = 8;
        int cu[PF];
        uint32_t row[PF];
        int got = 0;
#pragma unroll
        for (int q = 0; q < PF; q++) {
          cu[q] = -1;
          row[q] = 0;
          if (mask) {
            const int i0 = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            cu[q] = __builtin_amdgcn_readlane(u, i0);
            row[q] = adj[(size_t)cu[q] * ROWW + lane];
            got++;
          }
        }
#pragma unroll
        for (int q = 0; q < PF; q++) {
          if (q < got && np > 0 && !abandoned) {
            const int uq = cu[q];
            const uint32_t pq = (uint32_t)__builtin_amdgcn_readlane((int)P, uq & 63);
            if ((pq >> (uq >> 6)) & 1u) {  // still in P: joins the clique
              if (lane == (uq & 63)) C |= 1u << (uq >> 6);
              n++;
              P &= row[q];
              np = __builtin_amdgcn_readfirstlane(rsx::wave::sum_i32(__popc(P)));
              if (n + np <= best_n) abandoned = true;
            }
          }
        }
      }
    }
    if (!abandoned && n > best_n) {
      best_n = n;
      best = C;
    }
  }

  // ---- output: flags, the selected matches in their original order, the info record ----
  int run = 0;
  for (int c = 0; c < nc; c++) {  // vertex c * 64 + lane = bit c of this lane's word
    const int v = c * 64 + lane;
    const bool sel = v < K && ((best >> c) & 1u);
    if (v < K && a.member) a.member[p.o + v] = sel ? 1 : 0;
    const unsigned long long bal = __ballot(sel);
    if (sel && a.sel_src) {
      const int pos = run + __popcll(bal & ((1ull << lane) - 1ull));
      a.sel_src[p.o + pos] = a.src[p.o + v];
      a.sel_dst[p.o + pos] = a.dst[p.o + v];
    }
    run += __popcll(bal);
  }
  if (lane == 0) {
    if (a.sel_cnt) a.sel_cnt[p.pair] = best_n;
    if (a.info) a.info[p.pair] = rsx_orora_pmc_info{best_n, max_core, seeds, best_n == max_core + 1 ? RSX_ORORA_PMC_PROVEN : 0};
  }
  if (KEEP) {
    uint32_t *keep = reinterpret_cast<uint32_t *>(a.meta + (size_t)blockIdx.x * META_BYTES + META_KEEP);
    keep[lane] = best;
    if (lane == 0) keep[ROWW] = (uint32_t)best_n;
  }
}
__global__ __launch_bounds__(64) void pmc_walk_kernel(Args a) { pmc_walk<false>(a); }
__global__ __launch_bounds__(64) void pmc_walk_keep_kernel(Args a) { pmc_walk<true>(a); }

// ---- RSX_ORORA_PMC_EXACT: from the greedy clique to THE maximum clique (tests/pmc_exact_np.py restates every step) ----
// pmc_exact_kernel runs after pmc_walk_keep_kernel, ONE WAVEFRONT per pair at a time (a fixed number of workgroups stride over
// the pairs: the HBM stack is per workgroup, not per pair).  g = the greedy size.
//   proven (g == max core + 1) or |R| <= g, R = {core >= g}      -> a flag, nothing else (a few scalar loads)
//   U = the vertices of R adjacent to all of R (rows loaded eight at a time), S = R \ U in rank order, n = |S|
//   the adjacency of S re-indexed BY RANK: vertex r of S = bit r % 32 of lane r / 32, so that "the first vertex of a set in
//   rank order" is a ballot, two s_ff1 and a v_readlane -- in LDS when n <= 512 (rows of 16 words), otherwise written over the
//   row of the same vertex in the slab (row i reads only the old row of S[i]: in place)
//   greedy colouring at the root, then the depth-first search in rank order with an explicit stack of candidate sets (LDS
//   when it fits, otherwise the workgroup's HBM stack), the node budget checked in that loop -- the only one that can run long:
//   every other loop removes a vertex from a set of <= 2048 per turn.
// Every decision is a scalar (ballot / readlane / readfirstlane); no barrier; a wavefront waits for nobody.
constexpr int EX_LDS_N = 512;               // residual vertices whose adjacency fits LDS
constexpr int EX_LDS_W = EX_LDS_N / 32;     // words per row there
constexpr int EX_LDS_LEVELS = 256;          // stack levels in LDS

struct ExactArgs {
  long long budget;  // nodes per pair
  uint32_t *stack;   // [gridDim.x][MAX_K][ROWW]
  int n;             // pairs of this launch
};

struct ExactLds {
  uint32_t rows[EX_LDS_N * EX_LDS_W];
  uint32_t stk[EX_LDS_LEVELS * EX_LDS_W];
  uint16_t S[MAX_K];  // vertex r of S -> match of the pair
  uint16_t C[MAX_K];  // the clique in hand, by depth (vertices of S)
};

__device__ __forceinline__ int set_count(uint32_t x) { return __builtin_amdgcn_readfirstlane(rsx::wave::sum_i32(__popc(x))); }
__device__ __forceinline__ int set_first(uint32_t x) {  // the first vertex of a set over S, -1 = empty
  const unsigned long long m = __ballot(x != 0u);
  if (m == 0ull) return -1;
  const int t = __ffsll((long long)m) - 1;
  const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)x, t);
  return __builtin_amdgcn_readfirstlane(32 * t + (__ffs((int)w) - 1));
}
__device__ __forceinline__ uint32_t set_bit(int v, int lane) { return lane == (v >> 5) ? 1u << (v & 31) : 0u; }

struct ExactRows {
  const ExactLds *L;
  const uint32_t *adj;
  bool in_lds;
  __device__ __forceinline__ uint32_t row(int v, int lane) const {
    if (in_lds) return lane < EX_LDS_W ? L->rows[v * EX_LDS_W + lane] : 0u;
    return adj[(size_t)L->S[v] * ROWW + lane];
  }
};

// greedy sequential colouring of q in rank order; stops once more than `limit` colours are needed
__device__ __forceinline__ int ex_colours(const ExactRows &R, uint32_t q, int limit, int lane) {
  int k = 0;
  while (__ballot(q != 0u) != 0ull) {
    k++;
    if (k > limit) break;
    uint32_t c = q;
    for (int v = set_first(c); v >= 0; v = set_first(c)) {
      const uint32_t bit = set_bit(v, lane);
      c &= ~R.row(v, lane) & ~bit;
      q &= ~bit;
    }
  }
  return k;
}

__device__ __forceinline__ void ex_flag(const Args &a, int pair, int flags, int lane) {
  if (lane == 0 && a.info) a.info[pair].flags = flags;
}

__device__ __forceinline__ void exact_pair(const Args &a, const ExactArgs &x, int b, ExactLds &L, int lane) {
  const int pair = a.first + b;
  const int64_t o = a.offsets[pair], K64 = a.offsets[pair + 1] - o;
  if (K64 < 2 || K64 > MAX_K || (a.sel_src && o + K64 > a.sel_cap)) return;  // passed through by the walk
  const int K = __builtin_amdgcn_readfirstlane((int)K64), nc = (K + 63) >> 6;
  uint32_t *adj = a.slabs + (size_t)b * (rsx::pmc::SLAB_BYTES / 4);
  const char *meta = a.meta + (size_t)b * META_BYTES;
  const uint16_t *g_core = reinterpret_cast<const uint16_t *>(meta + META_CORE), *g_order = reinterpret_cast<const uint16_t *>(meta + META_ORDER);
  const uint32_t *keep = reinterpret_cast<const uint32_t *>(meta + META_KEEP);
  const int max_core = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int *>(meta + META_HDR));
  const int g = __builtin_amdgcn_readfirstlane((int)keep[ROWW]);
  if (g == max_core + 1) return ex_flag(a, pair, RSX_ORORA_PMC_PROVEN | RSX_ORORA_PMC_MAXIMUM, lane);

  // 1. R = the vertices of core number >= g: the first nR entries of `order`
  uint32_t Rm = 0;
  for (int c = 0; c < nc; c++) {
    const int v = c * 64 + lane;
    if (v < K && (int)g_core[v] >= g) Rm |= 1u << c;
  }
  const int nR = set_count(Rm);
  if (nR <= g) return ex_flag(a, pair, RSX_ORORA_PMC_MAXIMUM, lane);

  // 2. U = adjacent to all of R (into the clique), S = the rest, in rank order
  uint32_t Um = 0;
  int n = 0;
  for (int i0 = 0; i0 < nR; i0 += 8) {
    int vv[8];
    uint32_t rw[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      vv[q] = 0;
      rw[q] = 0;
      if (i0 + q < nR) {
        vv[q] = __builtin_amdgcn_readfirstlane((int)g_order[i0 + q]);
        rw[q] = adj[(size_t)vv[q] * ROWW + lane];
      }
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
      if (i0 + q < nR) {
        const int v = vv[q];
        if (set_count(rw[q] & Rm) == nR - 1) {
          if (lane == (v & 63)) Um |= 1u << (v >> 6);
        } else {
          if (lane == 0) L.S[n] = (uint16_t)v;
          n++;
        }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  const int u = nR - n, need = g - u;
  int best = need > 0 ? need : 0;
  bool improved = need < 0, exhausted = false;  // need < 0: U alone is larger than the greedy clique
  uint32_t bestm = 0;

  if (n > 0) {
    // 3. the adjacency of S by rank
    const bool in_lds = n <= EX_LDS_N;
    int levels = (n < max_core + 1 - u ? n : max_core + 1 - u) + 1;  // depth <= the largest clique of S
    if (levels > MAX_K) levels = MAX_K;                               // (what the workgroup's HBM stack holds)
    const bool stk_lds = in_lds && levels <= EX_LDS_LEVELS;
    uint32_t *gstk = x.stack + (size_t)blockIdx.x * ((size_t)MAX_K * ROWW);
    for (int i0 = 0; i0 < n; i0 += 4) {
      int vv[4];
      uint32_t rw[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        vv[q] = 0;
        rw[q] = 0;
        if (i0 + q < n) {
          vv[q] = __builtin_amdgcn_readfirstlane((int)L.S[i0 + q]);
          rw[q] = adj[(size_t)vv[q] * ROWW + lane];
        }
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (i0 + q < n) {
          uint32_t nw = 0;
          for (int c = 0; c * 64 < n; c++) {
            const int j = c * 64 + lane;
            const int w = j < n ? (int)L.S[j] : 0;
            const uint32_t word = (uint32_t)__shfl((int)rw[q], w & 63);
            const unsigned long long m = __ballot(j < n && ((word >> (w >> 6)) & 1u));
            if (lane == 2 * c) nw = (uint32_t)m;
            if (lane == 2 * c + 1) nw = (uint32_t)(m >> 32);
          }
          if (in_lds) {
            if (lane < EX_LDS_W) L.rows[(i0 + q) * EX_LDS_W + lane] = nw;
          } else {
            adj[(size_t)vv[q] * ROWW + lane] = nw;
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    const ExactRows R{&L, adj, in_lds};
    // candidates need core >= u + best: a prefix of S
    auto alive_of = [&](int bst) {
      int cnt = 0;
      for (int i = lane; i < n; i += 64) cnt += (int)g_core[L.S[i]] >= u + bst ? 1 : 0;
      const int m = __builtin_amdgcn_readfirstlane(rsx::wave::sum_i32(cnt)) - 32 * lane;
      return m >= 32 ? 0xffffffffu : m <= 0 ? 0u : (1u << m) - 1u;
    };
    auto stk_get = [&](int d) { return stk_lds ? (lane < EX_LDS_W ? L.stk[d * EX_LDS_W + lane] : 0u) : gstk[(size_t)d * ROWW + lane]; };
    auto stk_put = [&](int d, uint32_t P) {
      if (stk_lds) {
        if (lane < EX_LDS_W) L.stk[d * EX_LDS_W + lane] = P;
      } else {
        gstk[(size_t)d * ROWW + lane] = P;
      }
    };
    uint32_t alive = alive_of(best);
    if (ex_colours(R, alive, best, lane) > best) {
      // 4. depth-first in rank order; Cm = the clique in hand = C[0 .. d)
      long long nodes = 0;
      uint32_t Cm = 0;
      int d = 0;
      stk_put(0, alive);
      for (;;) {
        uint32_t Pd = stk_get(d) & alive;
        const int np = set_count(Pd);
        if (np == 0 || d + np <= best) {
          if (d == 0) break;
          d--;
          Cm &= ~set_bit(__builtin_amdgcn_readfirstlane((int)L.C[d]), lane);
          continue;
        }
        if (nodes >= x.budget) {
          exhausted = true;
          break;
        }
        nodes++;
        const int v = set_first(Pd);
        const uint32_t bit = set_bit(v, lane);
        Pd &= ~bit;
        stk_put(d, Pd);
        if (d + 1 > best) {
          best = d + 1;
          improved = true;
          bestm = Cm | bit;
          alive = alive_of(best);
        }
        const uint32_t Pn = Pd & R.row(v, lane) & alive;
        const int nn = set_count(Pn);
        if (nn == 0 || d + 1 + nn <= best) continue;
        if (d + 1 + ex_colours(R, Pn, best - d - 1, lane) <= best) continue;
        if (d + 2 > levels) continue;  // (cannot happen: a clique of S larger than the core bound allows)
        if (lane == 0) L.C[d] = (uint16_t)v;
        __builtin_amdgcn_wave_barrier();
        Cm |= bit;
        d++;
        stk_put(d, Pn);
      }
    }
  }
  if (exhausted) return ex_flag(a, pair, RSX_ORORA_PMC_BUDGET, lane);
  if (!improved) return ex_flag(a, pair, RSX_ORORA_PMC_MAXIMUM, lane);

  // ---- a larger clique: U + the clique of S, back in the pair's own numbering; flags, compaction and info as the walk's ----
  uint32_t cl = Um;
  for (int i = set_first(bestm); i >= 0; i = set_first(bestm)) {
    bestm &= ~set_bit(i, lane);
    const int v = __builtin_amdgcn_readfirstlane((int)L.S[i]);
    if (lane == (v & 63)) cl |= 1u << (v >> 6);
  }
  const int size = u + best;
  int run = 0;
  for (int c = 0; c < nc; c++) {
    const int v = c * 64 + lane;
    const bool sel = v < K && ((cl >> c) & 1u);
    if (v < K && a.member) a.member[o + v] = sel ? 1 : 0;
    const unsigned long long bal = __ballot(sel);
    if (sel && a.sel_src) {
      const int pos = run + __popcll(bal & ((1ull << lane) - 1ull));
      a.sel_src[o + pos] = a.src[o + v];
      a.sel_dst[o + pos] = a.dst[o + v];
    }
    run += __popcll(bal);
  }
  if (lane == 0) {
    if (a.sel_cnt) a.sel_cnt[pair] = size;
    if (a.info) {
      a.info[pair].size = size;
      a.info[pair].flags = RSX_ORORA_PMC_MAXIMUM | (size == max_core + 1 ? RSX_ORORA_PMC_PROVEN : 0);
    }
  }
}

__global__ __launch_bounds__(64) void pmc_exact_kernel(Args a, ExactArgs x) {
  __shared__ ExactLds L;
  const int lane = threadIdx.x;
  for (int b = blockIdx.x; b < x.n; b += gridDim.x) {
    exact_pair(a, x, b, L, lane);
    __builtin_amdgcn_wave_barrier();  // (the next pair's S / rows / stack are written after this pair's last read)
  }
}

}  // namespace

namespace rsx {
namespace pmc {

// Chunks of <= CHUNK pairs, one after the other on the caller's stream.  (Measured and not kept: two chunks in flight, the
// VALU-bound build of chunk c + 1 on the caller's stream beside the peeling + walk of chunk c on a side stream -- the
// peeling and the walk last as long as their LONGEST pair's chain of barriers and memory latencies whatever the number of
// pairs (0.5 - 0.65 ms each for 875 pairs as for 2 048), so four chunks of 875 pairs cost 5.3 ms against 5.0 ms for two
// chunks in sequence, and one chunk of all 3 500 is the fastest.)
int launch(Workspace &ws, int device, const float2 *d_src, const float2 *d_dst, const int64_t *d_offsets, int n_pairs, double tau,
           uint8_t *d_member, rsx_orora_pmc_info *d_info, float2 *d_sel_src, float2 *d_sel_dst, int32_t *d_sel_cnt, int64_t sel_cap, hipStream_t s,
           int64_t exact_budget) {
  (void)device;
  if (n_pairs <= 0) return RSX_OK;
  if (!(tau > 0.0)) return rsx::fail(RSX_ERR_BAD_ARG, "the consistency bound (tim_noise_bound) must be positive");
  const int chunk = n_pairs < CHUNK ? n_pairs : CHUNK;
  RSX_TRY(ws.slabs.reserve((size_t)chunk * SLAB_BYTES, s, false));
  RSX_TRY(ws.meta.reserve((size_t)chunk * META_BYTES, s, false));
  const bool exact = exact_budget > 0;
  const int slots = chunk < EXACT_SLOTS ? chunk : EXACT_SLOTS;
  if (exact) RSX_TRY(ws.stack.reserve((size_t)slots * SLAB_BYTES, s, false));
  Args a;
  a.src = d_src;
  a.dst = d_dst;
  a.offsets = d_offsets;
  a.n_pairs = n_pairs;
  a.tau2 = tau * tau;
  a.slabs = ws.slabs.as<uint32_t>();
  a.meta = ws.meta.as<char>();
  a.member = d_member;
  a.info = d_info;
  a.sel_src = d_sel_src;
  a.sel_dst = d_sel_dst;
  a.sel_cnt = d_sel_cnt;
  a.sel_cap = sel_cap;
  for (int first = 0; first < n_pairs; first += chunk) {
    const int n = n_pairs - first < chunk ? n_pairs - first : chunk;
    a.first = first;
    hipLaunchKernelGGL(pmc_build_kernel, dim3((unsigned)n, (unsigned)(MAX_K / BUILD_ROWS)), dim3(NT), 0, s, a);
    hipLaunchKernelGGL(pmc_cores_kernel, dim3((unsigned)n), dim3(NT), 0, s, a);
    if (!exact) {
      hipLaunchKernelGGL(pmc_walk_kernel, dim3((unsigned)n), dim3(64), 0, s, a);
    } else {
      hipLaunchKernelGGL(pmc_walk_keep_kernel, dim3((unsigned)n), dim3(64), 0, s, a);
      const ExactArgs x{(long long)exact_budget, ws.stack.as<uint32_t>(), n};
      hipLaunchKernelGGL(pmc_exact_kernel, dim3((unsigned)(n < slots ? n : slots)), dim3(64), 0, s, a, x);
    }
  }
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

}  // namespace pmc
}  // namespace rsx
