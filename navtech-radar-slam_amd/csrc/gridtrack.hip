// gridtrack.hip -- following a sensor through the radar grid map on gfx950: per scan a correlative match on the grid around a
// constant-velocity prediction, the refinement below the cell, and the composition of the motion -- whole sequences in one launch, one
// workgroup per sequence, the state (pose, motion, count: 104 bytes) resident in HBM.  What rsx_cfear_tracker_* is to CFEAR's
// registration.  None of this is in the reference checkout: the rule is the one stated in include/rsx.h and restated in
// tests/gridtrack_np.py (PARITY UNPINNED): fp64 on plain operations, nothing fused, every expression in the order written, so the
// records are the restatement's byte for byte.
//
// gmt_track: one workgroup of 256 threads per sequence loops over the sequence's scans of the push; the state is read at entry and
// written at exit; no workgroup reads what another writes, no atomics on device memory, no grid barrier.  Per scan:
//   the glue     mul, inv, renorm and the lost rule are computed by every thread from the same numbers: the same bits in every thread,
//                every branch on them workgroup-uniform, no broadcast.
//   the scoring  for each rotation in turn the cloud's cells go into LDS (fill_cells) and slot_sums runs -- the functions of
//                gridmatch_dev.h that gmm_score runs with one workgroup per rotation; here the rotations are serial, 2K + 1 <= 17.
//   the volume   (2K + 1)(2V + 1)(2U + 1) <= 17^3 = 4913 words, in LDS: it never leaves the chip.
//   the pick     pick_record of gridmatch_dev.h, the code gmm_pick runs, on the volume in LDS.
//   the refine   refine_record of gridrefine_dev.h, the code gmr_refine runs.
// Static LDS: cells 32768 + slot partials 4096 + volume 19652 + pick 3080 + refine 384 = 59980 bytes, under the 64 KB of a workgroup;
// two workgroups fit the 160 KB of a CU.
// The handle owns the state and the staging of its host entry and nothing else: the plane, the mutex, the stream and the stream order
// are the map's, so a push is ordered with the map's own calls like a refine.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "gridloc_host.h"
#include "gridmap.h"
#include "gridmatch_dev.h"
#include "gridrefine_dev.h"

#pragma STDC FP_CONTRACT OFF

namespace {

using rsx::fail;
using rsx::GRIDMAP_LIKE_MARGIN;
using namespace rsx::gridmatch_dev;  // NT, PLACE, MatchGeo, Rotations, job_points, skip_status, fill_cells, slot_sums, pick_record, PickLds
using rsx::gridrefine_dev::refine_record;
using rsx::gridrefine_dev::RefineGeo;
using rsx::gridrefine_dev::RefineLds;
namespace gridloc = rsx::gridloc;

constexpr int MAX_POINTS = RSX_GRIDMAP_MATCH_MAX_POINTS;
constexpr int MAX_K = RSX_GRIDMAP_TRACK_MAX_ANGLE_STEPS, MAX_UV = RSX_GRIDMAP_TRACK_MAX_CELLS;
constexpr int MAX_VOLUME = (2 * MAX_K + 1) * (2 * MAX_UV + 1) * (2 * MAX_UV + 1);
constexpr int MAX_SEQUENCES = 4096;
static_assert(PLACE + MAX_UV + 3 < GRIDMAP_LIKE_MARGIN, "a shifted read must stay in the frame");
static_assert(sizeof(rsx_gridmap_track_params) == 88 && sizeof(rsx_gridmap_track_result) == 344, "record layouts of include/rsx.h");

using Tables = Rotations<MAX_K>;

// a sequence's state in HBM
struct TrackState {
  double P[6], M[6];
  int32_t n, pad;
};
static_assert(sizeof(TrackState) == 104, "");

struct TrackConsts {
  rsx_gridmap_refine_params refine;
  unsigned min_score;
  int predict;
  int total_scans;  // the records that the output has room for
};

__device__ __forceinline__ void mul6(const double *A, const double *B, double *o) {
  o[0] = A[0] * B[0] + A[1] * B[3];
  o[1] = A[0] * B[1] + A[1] * B[4];
  o[2] = (A[0] * B[2] + A[1] * B[5]) + A[2];
  o[3] = A[3] * B[0] + A[4] * B[3];
  o[4] = A[3] * B[1] + A[4] * B[4];
  o[5] = (A[3] * B[2] + A[4] * B[5]) + A[5];
}

__device__ __forceinline__ void inv6(const double *A, double *o) {
  o[0] = A[0], o[1] = A[3], o[2] = -(A[0] * A[2] + A[3] * A[5]);
  o[3] = A[1], o[4] = A[4], o[5] = -(A[1] * A[2] + A[4] * A[5]);
}

// one Newton step towards a unit first column; the second column is rebuilt from the first
__device__ __forceinline__ void renorm6(const double *T, double *o) {
  const double n2 = T[0] * T[0] + T[3] * T[3];
  const double f = 1.5 - 0.5 * n2;
  const double c = T[0] * f, s = T[3] * f;
  o[0] = c, o[1] = -s, o[2] = T[2], o[3] = s, o[4] = c, o[5] = T[5];
}

__global__ __launch_bounds__(NT) void gmt_track(const float *__restrict__ xy, int64_t stride, const int64_t *__restrict__ offsets,
                                                const int32_t *__restrict__ n_scans, TrackState *__restrict__ state, Tables tab, MatchGeo g,
                                                RefineGeo rg, TrackConsts k, const uint8_t *__restrict__ plane,
                                                const uint8_t *__restrict__ origin, rsx_gridmap_track_result *__restrict__ out) {
  __shared__ unsigned cell[MAX_POINTS];  // byte offset of a point's cell in the framed plane, one rotation at a time
  __shared__ unsigned red[NT * 4];
  __shared__ unsigned vol[MAX_VOLUME];
  __shared__ PickLds pick_lds;
  __shared__ RefineLds refine_lds;
  const int tid = threadIdx.x, seq = blockIdx.x;
  int n_mine = n_scans[seq];
  if (n_mine <= 0) return;  // (workgroup-uniform, as every branch below)
  int64_t first_scan = 0;
  for (int q = 0; q < seq; q++) first_scan += n_scans[q] > 0 ? n_scans[q] : 0;
  if (first_scan >= (int64_t)k.total_scans) return;
  if ((int64_t)n_mine > (int64_t)k.total_scans - first_scan) n_mine = (int)((int64_t)k.total_scans - first_scan);
  const int nk = 2 * g.K + 1, nv = 2 * g.V + 1, nu = 2 * g.U + 1;
  TrackState *st = state + seq;
  double P[6], M[6];
#pragma unroll
  for (int q = 0; q < 6; q++) P[q] = st->P[q], M[q] = st->M[q];
  int seen = st->n;
  for (int sc = 0; sc < n_mine; sc++) {
    const int64_t scan = first_scan + sc;
    int64_t first;
    const int64_t n64 = job_points(offsets, (int)scan, &first);
    // ---- 1. the start pose ----
    double start[6];
    if (seen == 0 || k.predict == 0) {
#pragma unroll
      for (int q = 0; q < 6; q++) start[q] = P[q];
    } else {
      double pm[6];
      mul6(P, M, pm);
      renorm6(pm, start);
    }
    // ---- 2. the match: the volume rotation by rotation into LDS, then the pick ----
    if (!skip_status(start, n64)) {
      const int n = (int)n64;
      for (int kk = 0; kk < nk; kk++) {
        fill_cells(g, GRIDMAP_LIKE_MARGIN, xy, stride, first, n, start, (double)tab.c[kk], (double)tab.s[kk], cell);
        __syncthreads();
        unsigned *row = vol + kk * nv * nu;
        slot_sums(
            plane, cell, red, n, nv, nu, [&](int vi, int gi) { return (unsigned)((vi - g.V) * (int)g.pitch + (4 * gi - g.U)); },
            [&](int vi, int ui, unsigned sum) { row[vi * nu + ui] = sum; });
        __syncthreads();  // (the cells and the partials are written again; the pick reads the volume)
      }
    }
    const rsx_gridmap_match_result m = pick_record(xy, stride, first, n64, start, tab, g, vol, &pick_lds);
    // ---- 3, 4. lost, or refined ----
    const bool lost = m.status != 0 || m.score < k.min_score;
    rsx_gridmap_track_result *o = out + scan;
    if (lost) {
#pragma unroll
      for (int q = 0; q < 6; q++) P[q] = start[q];
      if (tid == 0) memset(&o->refine, 0, sizeof(o->refine));
    } else {
      const rsx_gridmap_refine_result r = refine_record(xy + first * stride, stride, n64, m.transform, rg, k.refine, origin, &refine_lds);
      double fresh[6];
      renorm6(r.transform, fresh);
      if (seen > 0) {
        double ip[6];
        inv6(P, ip);
        mul6(ip, fresh, M);
      }
#pragma unroll
      for (int q = 0; q < 6; q++) P[q] = fresh[q];
      if (tid == 0) o->refine = r;
    }
    // ---- 5. the count and the record ----
    seen++;
    if (tid == 0) {
#pragma unroll
      for (int q = 0; q < 6; q++) o->transform[q] = P[q], o->start[q] = start[q];
      o->match = m;
      o->flags = lost ? RSX_GRIDMAP_TRACK_LOST : 0;
      o->reserved = 0;
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < 6; q++) st->P[q] = P[q], st->M[q] = M[q];
    st->n = seen;
  }
}

int resolve(const rsx_gridmap_track_params *params, rsx_gridmap_track_params &dp) {
  rsx_gridmap_track_default_params(&dp);
  if (params) dp = *params;
  RSX_TRY(gridloc::check_window_params(dp.match, MAX_K, MAX_UV));
  if (dp.match.reserved != 0) return fail(RSX_ERR_BAD_ARG, "match.reserved must be 0");
  RSX_TRY(gridloc::check_refine_params(dp.refine));
  if (dp.predict != 0 && dp.predict != 1) return fail(RSX_ERR_BAD_ARG, "predict %d is neither 0 nor 1", dp.predict);
  if (dp.reserved[0] != 0 || dp.reserved[1] != 0) return fail(RSX_ERR_BAD_ARG, "reserved words of rsx_gridmap_track_params must be 0");
  return RSX_OK;
}

bool finite_pose(const double *t) {
  for (int q = 0; q < 6; q++)
    if (!std::isfinite(t[q])) return false;
  return true;
}

TrackState fresh_state(const double *pose6) {
  TrackState st{};
  for (int q = 0; q < 6; q++) st.P[q] = pose6[q];
  st.M[0] = st.M[4] = 1.0;
  return st;
}

}  // namespace

struct rsx_gridmap_tracker {
  rsx_gridmap *map = nullptr;  // its plane, mutex, stream and stream order; it outlives the tracker
  int32_t n_sequences = 0;
  rsx::DevBuf state;               // TrackState [n_sequences]
  rsx::DevBuf xy, off, nsc, out;   // staging of the host entry
};

namespace {

// the one launch of a push (the caller holds the map's mutex and has entered s)
int launch_track(rsx_gridmap_tracker *h, const float *d_xy, int64_t stride, const int64_t *d_off, const int32_t *d_nsc, int32_t total_scans,
                 const rsx_gridmap_track_params &p, rsx_gridmap_track_result *d_out, hipStream_t s) {
  rsx_gridmap *map = h->map;
  const Tables tab(p.match.angle_steps, p.match.angle_step);
  const MatchGeo g = gridloc::match_geo(map, p.match.angle_steps, p.match.x_cells, p.match.y_cells, (unsigned)map->like_pitch());
  const RefineGeo rg = gridloc::refine_geo(map);
  TrackConsts k{};
  k.refine = p.refine;
  k.min_score = p.min_score;
  k.predict = p.predict;
  k.total_scans = total_scans;
  hipLaunchKernelGGL(gmt_track, dim3((unsigned)h->n_sequences), dim3(NT), 0, s, d_xy, stride, d_off, d_nsc, h->state.as<TrackState>(), tab, g, rg, k,
                     map->like.as<uint8_t>(), (const uint8_t *)map->like_origin(), d_out);
  RSX_HIP(hipGetLastError());
  return RSX_OK;
}

// host states -> the handle's, from sequence `at` on; synchronous (the caller holds the map's mutex)
int upload_states(rsx_gridmap_tracker *h, const std::vector<TrackState> &st, int32_t at) {
  rsx_gridmap *map = h->map;
  RSX_HIP(hipSetDevice(map->device));
  hipStream_t s = map->stream;
  RSX_TRY(map->order.enter(s));
  RSX_TRY(h->state.reserve((size_t)h->n_sequences * sizeof(TrackState), s, false));
  RSX_HIP(hipMemcpyAsync(h->state.as<TrackState>() + at, st.data(), st.size() * sizeof(TrackState), hipMemcpyHostToDevice, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
}

}  // namespace

extern "C" {

int rsx_gridmap_track_default_params(rsx_gridmap_track_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  memset(p, 0, sizeof(*p));
  RSX_TRY(rsx_gridmap_match_default_params(&p->match));
  p->match.angle_steps = 2;
  p->match.x_cells = 2;
  p->match.y_cells = 2;
  RSX_TRY(rsx_gridmap_refine_default_params(&p->refine));
  p->min_score = 0u;
  p->predict = 1;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_tracker_create(rsx_gridmap *map, int32_t n_sequences, rsx_gridmap_tracker **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  if (!map) return fail(RSX_ERR_BAD_ARG, "null map");
  if (n_sequences < 1 || n_sequences > MAX_SEQUENCES) return fail(RSX_ERR_BAD_ARG, "n_sequences %d outside [1, %d]", n_sequences, MAX_SEQUENCES);
  std::unique_ptr<rsx_gridmap_tracker> h(new (std::nothrow) rsx_gridmap_tracker());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->map = map;
  h->n_sequences = n_sequences;
  const double identity[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  const std::vector<TrackState> st((size_t)n_sequences, fresh_state(identity));
  std::lock_guard<std::mutex> lk(map->mu);
  RSX_TRY(upload_states(h.get(), st, 0));
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_tracker_destroy(rsx_gridmap_tracker *h) try {
  if (!h) return RSX_OK;
  {
    rsx_gridmap *map = h->map;
    std::lock_guard<std::mutex> lk(map->mu);
    (void)hipSetDevice(map->device);
    if (map->order.enter(map->stream) == RSX_OK) (void)hipStreamSynchronize(map->stream);  // (a push on any stream has drained)
  }
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_tracker_reset(rsx_gridmap_tracker *h, const double *poses) try {
  if (!h || !poses) return fail(RSX_ERR_BAD_ARG, "bad arg");
  std::vector<TrackState> st((size_t)h->n_sequences);
  for (int32_t q = 0; q < h->n_sequences; q++) {
    if (!finite_pose(poses + 6 * (size_t)q)) return fail(RSX_ERR_BAD_ARG, "the pose of sequence %d is not finite", q);
    st[(size_t)q] = fresh_state(poses + 6 * (size_t)q);
  }
  std::lock_guard<std::mutex> lk(h->map->mu);
  return upload_states(h, st, 0);
} RSX_CATCH_ALL

int rsx_gridmap_tracker_set_pose(rsx_gridmap_tracker *h, int32_t sequence, const double *pose6) try {
  if (!h || !pose6) return fail(RSX_ERR_BAD_ARG, "bad arg");
  if (sequence < 0 || sequence >= h->n_sequences) return fail(RSX_ERR_BAD_ARG, "sequence %d outside [0, %d)", sequence, h->n_sequences);
  if (!finite_pose(pose6)) return fail(RSX_ERR_BAD_ARG, "the pose is not finite");
  const std::vector<TrackState> st(1, fresh_state(pose6));
  std::lock_guard<std::mutex> lk(h->map->mu);
  return upload_states(h, st, sequence);
} RSX_CATCH_ALL

int rsx_gridmap_tracker_state(rsx_gridmap_tracker *h, double *out_poses, double *out_motions, int32_t *out_counts) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::vector<TrackState> st((size_t)h->n_sequences);
  rsx_gridmap *map = h->map;
  std::lock_guard<std::mutex> lk(map->mu);
  RSX_HIP(hipSetDevice(map->device));
  hipStream_t s = map->stream;
  RSX_TRY(map->order.enter(s));
  RSX_HIP(hipMemcpyAsync(st.data(), h->state.p, st.size() * sizeof(TrackState), hipMemcpyDeviceToHost, s));
  RSX_HIP(hipStreamSynchronize(s));
  for (size_t q = 0; q < st.size(); q++) {
    if (out_poses) memcpy(out_poses + 6 * q, st[q].P, sizeof(st[q].P));
    if (out_motions) memcpy(out_motions + 6 * q, st[q].M, sizeof(st[q].M));
    if (out_counts) out_counts[q] = st[q].n;
  }
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_gridmap_tracker_push_device(rsx_gridmap_tracker *h, const float *d_xy, const int64_t *d_offsets, int32_t point_stride,
                                    const int32_t *d_n_scans, int32_t total_scans, const rsx_gridmap_track_params *params,
                                    rsx_gridmap_track_result *d_out, void *stream) try {
  if (!d_xy || !d_offsets || !d_n_scans || !d_out || total_scans < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  if (point_stride < 2) return fail(RSX_ERR_BAD_ARG, "point_stride %d below 2", point_stride);
  rsx_gridmap_track_params dp;
  RSX_TRY(resolve(params, dp));
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  rsx_gridmap *map = h->map;
  std::lock_guard<std::mutex> lk(map->mu);
  RSX_TRY(gridloc::have_likelihood(map));
  if (total_scans == 0) return RSX_OK;
  RSX_HIP(hipSetDevice(map->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : map->stream;
  RSX_TRY(map->order.enter(s));
  return launch_track(h, d_xy, point_stride, d_offsets, d_n_scans, total_scans, dp, d_out, s);
} RSX_CATCH_ALL

int rsx_gridmap_tracker_push(rsx_gridmap_tracker *h, const float *xy, const int64_t *offsets, const int32_t *n_scans,
                             const rsx_gridmap_track_params *params, rsx_gridmap_track_result *out) try {
  if (!xy || !offsets || !n_scans || !out) return fail(RSX_ERR_BAD_ARG, "bad arg");
  rsx_gridmap_track_params dp;
  RSX_TRY(resolve(params, dp));
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  int64_t total = 0;
  for (int32_t q = 0; q < h->n_sequences; q++) {
    if (n_scans[q] < 0) return fail(RSX_ERR_BAD_ARG, "n_scans[%d] = %d is negative", q, n_scans[q]);
    total += n_scans[q];
  }
  if (total > INT32_MAX) return fail(RSX_ERR_BAD_ARG, "too many scans");
  if (total > 0) {
    RSX_TRY(rsx::check_offsets(offsets, (int32_t)total, "rsx_gridmap_tracker_push"));
    for (int64_t j = 0; j < total; j++)
      if (offsets[j + 1] - offsets[j] > MAX_POINTS)
        return fail(RSX_ERR_BAD_ARG, "scan %lld has %lld points, more than %d", (long long)j, (long long)(offsets[j + 1] - offsets[j]), MAX_POINTS);
  }
  rsx_gridmap *map = h->map;
  std::lock_guard<std::mutex> lk(map->mu);
  RSX_TRY(gridloc::have_likelihood(map));  // (before the success of a push with no scans: a map that is not ready refuses that one too)
  if (total == 0) return RSX_OK;
  const size_t n = (size_t)total;
  RSX_HIP(hipSetDevice(map->device));
  hipStream_t s = map->stream;
  RSX_TRY(map->order.enter(s));
  RSX_TRY(rsx::stage_up(h->xy, xy, (size_t)offsets[total] * 8, s));
  RSX_TRY(rsx::stage_up(h->off, offsets, (n + 1) * 8, s));
  RSX_TRY(rsx::stage_up(h->nsc, n_scans, (size_t)h->n_sequences * 4, s));
  RSX_TRY(rsx::stage_room(h->out, n * sizeof(rsx_gridmap_track_result), s));
  RSX_TRY(launch_track(h, h->xy.as<float>(), 2, h->off.as<int64_t>(), h->nsc.as<int32_t>(), (int32_t)total, dp, h->out.as<rsx_gridmap_track_result>(), s));
  RSX_TRY(rsx::stage_down(out, h->out, n * sizeof(rsx_gridmap_track_result), s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
