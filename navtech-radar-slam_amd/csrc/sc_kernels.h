// sc_kernels.h -- launch wrappers of the ScanContext HIP kernels (sc_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rsx_common.h"

namespace rsx {
namespace sc {

constexpr int NR = RSX_SC_NUM_RING;
constexpr int NS = RSX_SC_NUM_SECTOR;
constexpr int DS = RSX_SC_DESC_SIZE;

// One column of the packed image (DbView::pk).  A radar feature cloud has z = 0, so every occupied bin of a descriptor column
// holds the same value: the column is 20 bits, that value and its norm.  An entry is PACKABLE when every element of every
// column is +0.0 (all bits zero) or bit-equal to ONE finite value of that column (the values of two columns may differ); a
// -0.0, a NaN, an inf or two different non-zero values in a column make it unpackable.  An unpackable entry still has a
// record (the array has no holes; its content describes nothing) and counts in the handle's counter of unpackable entries.
struct PackedCol {
  uint32_t bits;  // bit r = ring r of the column is occupied (element != +0.0)
  float val;      // the value of the occupied rings (+0.0: empty column)
  double norm;    // DbView::norm of the column
};
static_assert(sizeof(PackedCol) == 16, "one 16-byte load per column");

// One database shard in HBM (SoA, see DESIGN.md "Data layout"):
struct DbView {
  const float *desc;   // [n_local][60][20] fp32, sector-major == Eigen col-major order
  const double *vkey;  // [n_local][60] sector keys (SC.cpp:214-227)
  const double *norm;  // [n_local][60] column norms (shift-invariant part of SC.cpp:78,81)
  const float *rkey;   // [n_local][20] ring keys as float (SC.cpp:198-211 + 62-66)
  const void *hnT;     // filter image: column-normalised fp16, tile-major (sc_filter.hip); 2400 B per entry
  const uint64_t *cmask;  // [n_local] bit j = column j has a non-zero norm; bit 63 = non-finite element
  const void *spT;     // spectral filter image: fp16 Z15 spectra, tile-major (sc_spec.hip); 2432 B per entry
  const float *sp_aux; // [n_local] sqrt of the spectral energy outside f = 0 (error budget of the spectral filter)
  const void *hnR;     // the fp16 filter image once more, entry-major [n_local][1200] (sc_window.hip gathers single entries)
  const void *vk16;    // [n_local][128] fp16: sector key scaled by a power of two, hi[64] | lo[64] (sc_window.hip)
  const float *vk_n;   // [n_local][2] l2 norm of the scaled key (NaN: no matrix-core alignment for this entry), of the key
  const PackedCol *pk; // [n_local][60] packed columns, 960 B per entry (the packed form of sc_rescore_wave_kernel)
  int64_t n_local;
  int64_t idx_base;    // global index of local slot s = idx_base + s * idx_stride
  int64_t idx_stride;
  int32_t sum_order;   // RSX_SC_SUM_*: the order of the sums the reference takes through Eigen (sc_redux_dev.h)
};

// Element of the bound matrix the filter hands to the short-list selection and the re-scoring: fp16, converted with
// round-toward-zero.  A bound v is only ever used as "skip the pair when v - eps > tau": a positive v rounded toward zero
// is still a lower bound, a negative v stays <= 0 <= every distance, +-inf and NaN survive.  Against fp32 this halves the
// matrix (8192 x 10 000: 0.33 -> 0.16 GB written by the filter and read twice by the selection per step) for < 2^-10
// relative looseness (eps is 1.25e-3).
using lb_t = _Float16;
typedef _Float16 lb2_t __attribute__((ext_vector_type(2)));
// Histogram of the bounds the short-list selection and the re-scoring share: RESCORE_BINS bins over [0, 1), bounds outside
// land in the end bins.  bin(x) <= b  <=>  x < (b + 1) / RESCORE_BINS exactly (power-of-two scaling), so a "bound < edge" test
// selects whole bins.
constexpr int RESCORE_BINS = 2048;
#ifdef __HIPCC__
__device__ __forceinline__ lb_t lb_pack(float v) {
  return __builtin_bit_cast(lb2_t, __builtin_amdgcn_cvt_pkrtz(v, 0.0f))[0];
}
__device__ __forceinline__ int lb_bin(float d) {
  if (!(d > 0.0f)) return 0;  // negative, -inf, NaN
  const float x = d * (float)RESCORE_BINS;
  return x >= (float)(RESCORE_BINS - 1) ? RESCORE_BINS - 1 : (int)x;
}
__device__ __forceinline__ float lb_bin_edge(int b) {  // upper edge of bin b as a "bound < edge" test
  return b < 0 ? -INFINITY : (b >= RESCORE_BINS - 1 ? INFINITY : (float)(b + 1) / (float)RESCORE_BINS);
}
__device__ __forceinline__ int lb_edge_bin(float edge) {  // the inverse: the bin whose upper edge this is
  return edge == -INFINITY ? -1 : (edge == INFINITY ? RESCORE_BINS - 1 : (int)(edge * (float)RESCORE_BINS) - 1);
}
__device__ __forceinline__ float lb_bin_lo(int b) {  // lower edge of bin b (bin 0 also takes what is below 0)
  return b <= 0 ? -INFINITY : (float)b / (float)RESCORE_BINS;
}
#endif

struct QueryView {
  const float *desc;   // [nq][1200]
  const double *vkey;  // [nq][60]
  const double *norm;  // [nq][60]
  int32_t nq;
};

// keys for n descriptors (device pointers)
int launch_keys(const float *desc, int64_t n, double *vkey, double *norm, float *rkey, hipStream_t s, int sum_order);

// descriptor from one point cloud resident in device memory, written to out_desc (1200 floats)
// followed by its keys
int launch_build(const void *d_pts, int64_t n_pts, int64_t stride_bytes, double lidar_height,
                 double max_radius, float *out_desc, double *out_vkey, double *out_norm,
                 float *out_rkey, hipStream_t s, int sum_order);

// number of partial top-k slots per query the pair kernel will produce for this problem
int pair_num_slots(int64_t n_items, int32_t nq);
size_t pair_partial_bytes(int64_t n_items, int32_t nq, int32_t k);

// score nq queries against db entries.
//   gather == nullptr: local slots [first, first+n_items); else slots gather[0..n_items)
//   n_eligible: only entries with global index < min(n_eligible, q_elig[q] if given) are ranked
//   out_dist/out_shift (optional, [nq][n_items]): every pair, eligibility ignored
//   d_partial (optional): workspace of pair_partial_bytes(); d_topk [nq][k] receives the merged
//   result sorted by (dist, index), padded with {1e7,0,0}
int launch_pairs(const DbView &db, const QueryView &q, const int32_t *gather, int64_t first,
                 int64_t n_items, int64_t n_eligible, const int64_t *q_elig, double *out_dist,
                 int32_t *out_shift, rsx_sc_hit *d_partial, rsx_sc_hit *d_topk, int32_t k,
                 hipStream_t s);

// one launch per new keyframe: descriptor + keys from the cloud AND every per-entry image of the query path (sc_spec.hip
// sc_insert_kernel).  n_clouds clouds: points [d_offs[b], d_offs[b + 1]) of d_pts go to local slot first_slot + b
// (d_offs = nullptr: one cloud of n_pts points)
int launch_insert(const void *d_pts, const int64_t *d_offs, int64_t n_pts, int64_t n_clouds, int64_t stride_bytes,
                  double lidar_height, double max_radius, int64_t first_slot, float *desc, double *vkey, double *norm,
                  float *rkey, void *hnT, void *hnR, uint64_t *cmask, void *spT, float *aux, const double *tw, void *vk16,
                  float *vk_n, PackedCol *pk, uint32_t *n_unpackable, hipStream_t s, int sum_order);

// merge [nparts][nq][k] -> [nq][k]
int launch_merge(const rsx_sc_hit *d_parts, int32_t nparts, int32_t nq, int32_t k, rsx_sc_hit *d_out,
                 hipStream_t s);

// d_lb[q][c] (ld elements per row, nq rows) = d_blocks[c / block_ld][q0 + q][c % block_ld]: the column blocks the filter
// shards of a replicated DB deliver (block b starts block_stride elements after block b - 1) as one bound matrix
int launch_gather_bounds(const lb_t *d_blocks, int64_t block_ld, int64_t block_stride, int64_t q0, int32_t nq, lb_t *d_lb,
                         int64_t ld, hipStream_t s);

// exact k-NN over ring keys [0, n_search) with nanoflann's float L2 (NF.hpp:383-408);
// d_dist_ws: n_search floats of workspace; out_idx[k] (unfilled = 0), out_found[1]
int launch_knn(const float *rkeys, int64_t n_search, const float *qkey, int32_t k, float *d_dist_ws,
               int32_t *out_idx, float *out_dist, int32_t *out_found, hipStream_t s);

// ---- exact re-scoring behind the filter ----
constexpr int RESCORE_SHORTLIST_CAP = 2048;  // short-list positions per query (sl_cnt <= this; stride of the record array)
// Only the HEAD of a short list is stored as records: the bins up to the first one whose cumulative count reaches
// RESCORE_HEAD (clamped to the last bin of the list).  sc_window_kernel uses positions below min(sl_cnt, WINDOW_P) and
// nothing else (it LOADS all WINDOW_P slots of the query's stride at its start, before it knows sl_cnt, and drops the rest:
// the array must be allocated at its full stride for every query of a launch, written or not); sc_rescore_wave_kernel
// re-derives the positions behind the head from the query's row of bounds.
constexpr int RESCORE_HEAD = 512;
static_assert(RESCORE_HEAD >= RSX_SC_WINDOW_P && RESCORE_HEAD <= RESCORE_SHORTLIST_CAP,
              "the head must cover every list position sc_window_kernel may read (WINDOW_P)");
constexpr int RESCORE_NUM_THR = 6;           // round edges t_0..t_4 and t_cap
// per query: RESCORE_NUM_THR float edges, then RESCORE_NUM_THR int32 counts (short-list entries below each edge:
// the list is ordered by bin, so round r is the range [count[r-1], count[r])), then the head: its last bin (int32, -1 = no
// head) and its end position = the number of records stored
constexpr int RESCORE_THR_HEAD_BIN = 2 * RESCORE_NUM_THR, RESCORE_THR_HEAD_END = 2 * RESCORE_NUM_THR + 1;
constexpr int RESCORE_THR_STRIDE = 16;       // 64 bytes per query
static_assert(RESCORE_THR_HEAD_END < RESCORE_THR_STRIDE, "layout");
// the re-scoring kernels' bookkeeping (profiling only): RESCORE_STAT_COPIES blocks of RESCORE_STAT_WORDS u64 counters; a query
// adds to block (query index % copies) -- one shared block made 8192 waves queue up on a single cache line of atomics (measured:
// +0.15-0.23 ms on a 3.4 ms step); the host sums the blocks
constexpr int RESCORE_STAT_WORDS = 24, RESCORE_STAT_COPIES = 64;
struct WindowPreview;
struct WindowSurvivor;
struct RescoreEntry {
  float lb;      // filter bound
  int32_t slot;  // local DB slot
};
// short list of every query: the eligible entries with bound < t_cap, where t_cap is the largest
// histogram-bin edge with at most RESCORE_SHORTLIST_CAP bounds below it (+inf when all fit, -inf
// when not even the first bin fits), and the round edges (first_target << r bounds, r = 0..4)
// first_target: bounds in round 0; round r covers first_target << r
// slist receives the records of the head only (positions [0, head end), ordered by bin); sl_cnt, the edges and their
// counts describe the WHOLE list
int launch_select(const DbView &db, const lb_t *lb, int64_t ld_lb, int64_t n_items, int32_t nq, int64_t n_eligible,
                  const int64_t *q_elig, int32_t first_target, RescoreEntry *slist, int32_t *sl_cnt, float *thr,
                  hipStream_t s);
// one wave per query: list positions of rounds [round_begin, round_end) of ascending bound with tau tightening
// (round_end = RESCORE_ALL_ROUNDS: also the entries beyond the short list); writes the top-k it knows.
// List positions behind the head launch_select stored are taken from the row of bounds lb (bin by bin, ascending slot
// inside a bin), so lb, ld_lb, n_items, n_eligible and q_elig must be the ones launch_select got.
// surv: the survivor lists launch_window wrote for the same short lists (what of the head of every list is left to score);
// tau_src (optional): a top-k that covers more than this shard -- its k-th distance caps tau;
// seed (optional): this shard's hits from an earlier stage, merged into the output.
// packed: every entry of db is packable (PackedCol) -- the kernel reads db.pk instead of db.desc / db.norm and the sector key
// only where it aligns; same records, same statistics
constexpr int RESCORE_ALL_ROUNDS = RESCORE_NUM_THR + 1;
int launch_rescore(const DbView &db, const QueryView &q, const lb_t *lb, int64_t ld_lb, int64_t n_items,
                   int64_t n_eligible, const int64_t *q_elig, const RescoreEntry *slist, const int32_t *sl_cnt,
                   const float *thr, double eps, int32_t round_begin, int32_t round_end, const rsx_sc_hit *tau_src,
                   const rsx_sc_hit *seed, rsx_sc_hit *d_out, int32_t k, hipStream_t s, unsigned long long *d_stats,
                   const WindowSurvivor *surv, bool packed);

// ---- MFMA lower-bound filter (sc_filter.hip) ----
constexpr int FILTER_QIMG_BYTES = 9984;  // LDS image of one query (two displaced fp16 copies)
constexpr int FILTER_QIMG_ODD = 4960;    // byte offset of the copy read by odd shifts (holds q2[4..]); = 96 mod 256
constexpr int FILTER_QIMG_MASK_OFF = 4928;  // the query's column mask (u64) sits in the gap between the copies
constexpr float FILTER_ACC_SCALE = 1073741824.0f;  // 2^30: both fp16 images are scaled by 2^15
constexpr int FILTER_DB_BYTES_PER_ENTRY = 2 * DS;
double filter_eps();
size_t filter_qimg_bytes(int32_t nq);
// fp16 filter images and packed columns of local slots [first, first+count) (needs their norms); *n_unpackable (device) grows
// by the number of these entries that are not packable
int launch_db_images(const float *desc, const double *norm, int64_t first, int64_t count, void *hnT, void *hnR,
                     uint64_t *cmask, PackedCol *pk, uint32_t *n_unpackable, hipStream_t s);
int launch_query_images(const float *desc, const double *norm, int32_t nq, void *qimg, hipStream_t s);
// lb[q*ld_lb + slot] = lower bound of dist(query q, local slot), slots [0, n_items); +inf when no
// shift has an effective column (never a hit), -inf when the pair must be re-scored regardless
// plan (optional, with plan_ws of filter_plan_bytes(n_items) bytes): the queries' eligibility limits
// min(n_eligible, q_elig[q]) do not decrease with q, so the (tile-block, query) pairs a query cannot see
// are skipped altogether (their lb entries stay unwritten; they lie outside the query's eligible rows)
struct FilterPlanInput {
  int64_t n_eligible;
  const int64_t *q_elig;
};
size_t filter_plan_bytes(int64_t n_items);
// the plan itself (device): tb_qmin in units of `qgroup` queries (1: direct filter, 4: spectral filter's query
// tiles), tb_cum = exclusive prefix sums of ceil(nq / qgroup) - tb_qmin; both inside plan_ws
int launch_filter_plan(const DbView &db, const FilterPlanInput &plan, int32_t nq, int64_t n_items, int32_t qgroup,
                       void *plan_ws, const int32_t **tb_qmin, const int64_t **tb_cum, hipStream_t s);
int launch_filter(const DbView &db, const void *qimg, int32_t nq, int64_t n_items, lb_t *lb, int64_t ld_lb,
                  const FilterPlanInput *plan, void *plan_ws, hipStream_t s);
const char *pair_kernel_name();
const char *filter_kernel_name();

// ---- spectral form of the filter (sc_spec.hip): same bounds contract, ~7x fewer MFMAs ----
constexpr int SPEC_QIMG_BYTES = 4736;       // stream image of a query (sc_spec.hip); the mask image and flag byte follow the images
constexpr int SPEC_DB_BYTES_PER_ENTRY = 2432;
size_t spec_qimg_bytes(int32_t nq);
// tw: the twiddle table of the spectra, SPEC_TWIDDLE_DOUBLES doubles of device memory filled once by launch_spec_twiddles (with
// the device's own cospi / sinpi: every image kernel below reads it instead of evaluating the 15 factors per wavefront)
constexpr int SPEC_TWIDDLE_DOUBLES = 32;
int launch_spec_twiddles(double *tw, hipStream_t s);
int launch_spec_db_images(const float *desc, const double *norm, int64_t first, int64_t count, void *spT, float *aux,
                          const double *tw, hipStream_t s);
int launch_spec_query_images(const float *desc, const double *norm, int32_t nq, void *qimg, const double *tw, hipStream_t s);
// sc_spec2_filter_kernel: two waves per SIMD, the entry tile split by frequency
int launch_spec_filter(const DbView &db, const void *qimg, int32_t nq, int64_t n_items, lb_t *lb, int64_t ld_lb,
                       const int32_t *tb_qmin, const int64_t *tb_cum, hipStream_t s);
const char *spec2_filter_kernel_name();

// ---- window previews of the short lists on the matrix cores (sc_window.hip) ----
// For the first WINDOW_P short-list entries of every query: the sector-key alignment k* (SC.cpp:93-113) from an fp16
// hi/lo-split correlation (unique within its error bound, else "no preview") and the fp16 direct-form correlation of
// the two images evaluated over the window k* +- 3 only: pv with |pv - dist(query, entry)| <= WINDOW_MARGIN.  The
// re-scoring kernel uses (k*, pv) instead of its own VALU alignment + fp32 preview.
constexpr int WINDOW_P = RSX_SC_WINDOW_P;               // short-list positions per query that can get a record
constexpr int WINDOW_HEAD = 128;                         // the head of the list: always processed (pass 1)
constexpr float WINDOW_MARGIN = RSX_SC_WINDOW_MARGIN;    // same arithmetic as the direct filter: its error budget (sc_filter.hip)
constexpr int WINDOW_QK_BYTES = 4624;                    // key image of a query (sc_window.hip)
static_assert(WINDOW_P % 64 == 0 && WINDOW_HEAD == 128 && WINDOW_P > WINDOW_HEAD, "layout");
// Positions WINDOW_HEAD .. WINDOW_P - 1 are processed (pass 2) only when their filter bound does not exceed the k-th
// smallest upper bound the head yields; the others get the record {NaN, -2} = "none".
struct WindowPreview {
  float pv;    // NaN: no preview (non-finite data, or no record); +inf: no effective column in the window(s)
  int32_t ks;  // >= 0: k* in bits 0..5 and, in bits 8..14, which of the window shifts k* - 3 + t can be the minimum at all
               // (the others are more than 2 margins above the best preview); -1: not unique within the error bound -- pv is
               // then a lower bound only (union of the windows); -2: no record
};
// What the window kernel hands to the re-scoring kernel: per query one header and, behind it, the list positions below
// min(sl_cnt, WINDOW_P) that can still reach the top-k, in any order.  tau_ub is the k-th smallest pv + WINDOW_MARGIN over ALL
// records of the query with a unique alignment and a finite preview (+inf with fewer than k of them): every such record is a
// distinct eligible entry of this shard's list, so tau_ub is an upper bound of the shard's final k-th best distance.  A
// position is listed when pv - WINDOW_MARGIN <= tau_ub and its filter bound - eps <= tau_ub, or when its preview is NaN.
struct WindowSurvivor {
  float lo;      // pv - WINDOW_MARGIN: a lower bound of the pair distance; -inf: no preview (non-finite data), must be scored
  int32_t slot;  // local DB slot
  int32_t ks;    // (k* | shift mask << 8) as in WindowPreview, or -1: the alignment is not known
  int32_t pos;   // short-list position (the rounds of a launch are position ranges)
};
struct WindowListHeader {
  int32_t count;    // survivors behind the header
  float tau_ub;     // see above
  int32_t n_cand;   // (statistics) positions whose filter bound - eps does not exceed tau_ub and whose preview is not +inf
  int32_t n_prev;   // (statistics) those of them with a preview
};
static_assert(sizeof(WindowSurvivor) == 16 && sizeof(WindowListHeader) == 16, "one 16-byte load each");
constexpr int WINDOW_LIST_STRIDE = WINDOW_P + 1;  // 16-byte units per query: the header, then up to WINDOW_P survivors
int launch_window_db_keys(const double *vkey, int64_t first, int64_t count, void *vk16, float *vk_n, hipStream_t s);
// q: the kernel builds the queries' fp16 image and key image itself, in LDS, from q.desc / q.norm / q.vkey; out: [nq][WINDOW_P];
// surv: [nq][WINDOW_LIST_STRIDE], the header of EVERY query is written (an empty list included)
// k: the top-k the query batch asks for; eps: the filter's error budget (filter_eps())
int launch_window(const DbView &db, const QueryView &q, const RescoreEntry *slist, const int32_t *sl_cnt,
                  int32_t k, double eps, WindowPreview *out, WindowSurvivor *surv, hipStream_t s);
const char *window_kernel_name();

// ---- one query in one launch (sc_q1.hip): the live detector's regime, nq <= Q1_MAX_NQ ----
// Streams the fp16 image + key image of every eligible entry once (2672 B per entry), previews every pair on the matrix cores
// (alignment + window, as sc_window.hip does for the heads of the short lists) and scores the few entries the previews cannot
// exclude exactly, all inside one launch; records identical to launch_pairs / the filtered path.
// ws: q1_workspace_bytes() of device memory; d_ticket: q1_ticket_bytes() of arrival counters, zero before the first launch
// (every launch leaves them zero again) and touched by nothing else
constexpr int Q1_MAX_NQ = 16;
int q1_grid(int64_t n_items, int32_t k, int32_t nq);
size_t q1_workspace_bytes(int64_t n_items, int32_t nq, int32_t k);
size_t q1_ticket_bytes();
int launch_q1(const DbView &db, const float *d_q, int32_t nq, int64_t n_items, int64_t n_eligible, const int64_t *q_elig,
              int32_t k, rsx_sc_hit *d_out, void *ws, unsigned *d_ticket, unsigned long long *d_stats, hipStream_t s);
const char *q1_kernel_name();

// ---- the reference's public helper methods on arbitrary double descriptors (sc_helpers.hip) ----
// op 0: keys of d_a (out_d = ring key [20] + sector key [60]); 1: distDirectSC(d_a, d_b) -> out_d[0];
// 2: fastAlignUsingVkey(d_a, d_b) (60-element keys) -> out_i[0]; 3: distanceBtnScanContext -> out_d[0], out_i[0]
int launch_helper(int op, const double *d_a, const double *d_b, double *d_out_d, int32_t *d_out_i, hipStream_t s, int sum_order);

// optional hipEvent bracket around the dominant (pair) kernel
struct PairProfiler {
  bool on = false;
  static constexpr int kMax = 4096;
  std::unique_ptr<Event[]> ev;  // 2*kMax events with timing, created lazily
  int used = 0;
};
void set_pair_profiler(PairProfiler *p);  // thread-local hook consulted by launch_pairs

}  // namespace sc
}  // namespace rsx
