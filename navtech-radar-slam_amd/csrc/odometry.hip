// odometry.hip -- the per-sequence pipeline of the upstream file-based odometry.cpp entry, device resident and batched.
//
// What the reference runs per scan (its ORORA submodule, an empty directory in the reference checkout: .gitmodules:1-3;
// README.md:26-29,54-60; launch/navtech_radar_slam_mulran.launch:5-8): polar image -> cen2019 keypoints -> Cartesian image
// -> ORB descriptors -> BFMatcher knnMatch(2) + ratio against the previous scan -> ORORA (GNC rotation, A-COTE
// translation) -> pose composition.  The sequence is on disk, so every scan and every consecutive pair is independent
// until the final composition: a WINDOW of n scans goes through each stage in ONE launch chain --
//     the ONE selected extractor (rsx_odometry::keypoints: cen2019 until rsx_odometry_set_cen2018 / _kstrongest / _cfar selects another),
//     Cartesian images, descriptors, consecutive matches in both directions, cross check + correspondence lists (odo_cross / odo_gather),
//     and ORORA over all pairs of the window in one call, max-clique selection first (DESIGN.md 4.11 names every launch).
// That is the default configuration.  The setters of the estimator side (rsx_odometry_set_estimator, _set_cfear, _set_cfear_tracking,
// _set_compensation, _set_phasecorr) change ONE value, OdoConfig, under the rules of check_config; what a configuration builds per scan,
// which pair stage registers the consecutive pairs (src = this scan, dst = the previous one) and what is carried to the next window is
// answered once per push by needs_of -- OdoNeeds below says it field by field, and enqueue_match has one branch per pair stage
// -- with every intermediate (keypoints, descriptors, matches, correspondences) in HBM; one upload of the images and one
// download of 48 bytes per scan (+ the keypoints when the caller wants /orora/cloud_local).  The last scan of a window
// stays on the device as the "previous scan" of the next one.  Pose composition stays on the host (sequential, trivial).
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>

#include "cen2018.h"
#include "cfar.h"
#include "cfear.h"
#include "keypoints_host.h"
#include "kstrongest.h"
#include "mocomp.h"
#include "phasecorr.h"
#include "ransac.h"

namespace {

#ifndef RSX_ODO_WINDOW
#define RSX_ODO_WINDOW 64
#endif
constexpr int MAX_WINDOW = RSX_ODO_WINDOW;  // scans per internal launch chain (workspace: ~26 MB per scan and extraction lane, two lanes)

// one block per consecutive pair j (slots A = first + j, B = A + 1): keep prev keypoint i when fwd[i] = k >= 0 and
// bwd[k] = i, in ascending i (the order the host loop of round 2 produced); src = the CURRENT scan's point, dst = the
// previous scan's point, so that ORORA returns the motion of the sensor expressed in the previous frame.
// DT (motion-compensated RANSAC): also the time between the two measurements of a match, from the azimuth rows of its two
// keypoints (targets [slot][stride][2], row first): dt = (float)(dt_scan (1 + (a_cur - a_prev) / rows)) -- include/rsx.h
// AZ (rsx_odometry_set_compensation): the two azimuth rows themselves, for csrc/mocomp.hip
template <bool DT, bool AZ = false>
__device__ __forceinline__ void cross_pair(const float *__restrict__ xy, const int32_t *__restrict__ counts, int stride, int first,
                                           const int32_t *__restrict__ fwd, const int32_t *__restrict__ bwd, float2 *__restrict__ stage_src,
                                           float2 *__restrict__ stage_dst, int32_t *__restrict__ pair_cnt, const int32_t *__restrict__ targets,
                                           int rows, double dt_scan, float *__restrict__ stage_dt, int32_t *__restrict__ stage_acur = nullptr,
                                           int32_t *__restrict__ stage_aprev = nullptr) {
  __shared__ unsigned s_w[4];
  const int j = blockIdx.x, A = first + j, B = A + 1;
  const int nA = counts[A] < stride ? counts[A] : stride, nB = counts[B] < stride ? counts[B] : stride;
  const int32_t *f = fwd + (int64_t)j * stride, *b = bwd + (int64_t)j * stride;
  const float2 *pa = reinterpret_cast<const float2 *>(xy) + (int64_t)A * stride, *pb = reinterpret_cast<const float2 *>(xy) + (int64_t)B * stride;
  float2 *ss = stage_src + (int64_t)j * stride, *sd = stage_dst + (int64_t)j * stride;
  unsigned run = 0;
  for (int base = 0; base < nA; base += 256) {
    const int i = base + threadIdx.x;
    int k = -1;
    if (i < nA) {
      k = f[i];
      if (k >= nB || (k >= 0 && b[k] != i)) k = -1;
    }
    const unsigned long long bal = __ballot(k >= 0);
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_w[w] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned before = run, total = 0;
    for (unsigned ww = 0; ww < 4; ww++) {
      if (ww < w) before += s_w[ww];
      total += s_w[ww];
    }
    if (k >= 0) {
      const unsigned pos = before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
      ss[pos] = pb[k];
      sd[pos] = pa[i];
      if constexpr (DT) {
        const int a_prev = targets[((int64_t)A * stride + i) * 2], a_cur = targets[((int64_t)B * stride + k) * 2];
        stage_dt[(int64_t)j * stride + pos] = (float)(dt_scan * (1.0 + (double)(a_cur - a_prev) / (double)rows));
      }
      if constexpr (AZ) {
        stage_aprev[(int64_t)j * stride + pos] = targets[((int64_t)A * stride + i) * 2];
        stage_acur[(int64_t)j * stride + pos] = targets[((int64_t)B * stride + k) * 2];
      }
    }
    run += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) pair_cnt[j] = (int32_t)run;
}

__global__ __launch_bounds__(256) void odo_cross(const float *__restrict__ xy, const int32_t *__restrict__ counts, int stride, int first,
                                                 const int32_t *__restrict__ fwd, const int32_t *__restrict__ bwd,
                                                 float2 *__restrict__ stage_src, float2 *__restrict__ stage_dst, int32_t *__restrict__ pair_cnt) {
  cross_pair<false>(xy, counts, stride, first, fwd, bwd, stage_src, stage_dst, pair_cnt, nullptr, 0, 0.0, nullptr);
}

__global__ __launch_bounds__(256) void odo_cross_dt(const float *__restrict__ xy, const int32_t *__restrict__ counts, int stride, int first,
                                                    const int32_t *__restrict__ fwd, const int32_t *__restrict__ bwd,
                                                    float2 *__restrict__ stage_src, float2 *__restrict__ stage_dst, int32_t *__restrict__ pair_cnt,
                                                    const int32_t *__restrict__ targets, int rows, double dt_scan, float *__restrict__ stage_dt) {
  cross_pair<true>(xy, counts, stride, first, fwd, bwd, stage_src, stage_dst, pair_cnt, targets, rows, dt_scan, stage_dt);
}

__global__ __launch_bounds__(256) void odo_cross_az(const float *__restrict__ xy, const int32_t *__restrict__ counts, int stride, int first,
                                                    const int32_t *__restrict__ fwd, const int32_t *__restrict__ bwd,
                                                    float2 *__restrict__ stage_src, float2 *__restrict__ stage_dst, int32_t *__restrict__ pair_cnt,
                                                    const int32_t *__restrict__ targets, int32_t *__restrict__ stage_acur,
                                                    int32_t *__restrict__ stage_aprev) {
  cross_pair<false, true>(xy, counts, stride, first, fwd, bwd, stage_src, stage_dst, pair_cnt, targets, 0, 0.0, nullptr, stage_acur, stage_aprev);
}

// one block per pair: contiguous correspondence arrays + the offsets rsx_orora_register_batch_device wants
__global__ __launch_bounds__(256) void odo_gather(const float2 *__restrict__ stage_src, const float2 *__restrict__ stage_dst,
                                                  const int32_t *__restrict__ pair_cnt, int n_pairs, int stride, float2 *__restrict__ src,
                                                  float2 *__restrict__ dst, int64_t *__restrict__ offsets) {
  __shared__ long long s_w[4];
  const int j = blockIdx.x;
  long long before = 0;
  for (int r = threadIdx.x; r < j; r += 256) before += pair_cnt[r];
  before = rsx::wave::butterfly(before, rsx::wave::Add{});
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = before;
  __syncthreads();
  before = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  const int n = pair_cnt[j];
  for (int i = threadIdx.x; i < n; i += 256) {
    src[before + i] = stage_src[(int64_t)j * stride + i];
    dst[before + i] = stage_dst[(int64_t)j * stride + i];
  }
  if (threadIdx.x == 0) {
    offsets[j] = before;
    if (j == n_pairs - 1) offsets[n_pairs] = before + n;
  }
}

// behind odo_gather (its offsets): the staged dt of every pair to where its matches went
__global__ __launch_bounds__(256) void odo_gather_dt(const float *__restrict__ stage_dt, const int64_t *__restrict__ offsets, int stride,
                                                     float *__restrict__ dt) {
  const int j = blockIdx.x;
  const int64_t o = offsets[j], n = offsets[j + 1] - o;
  for (int64_t i = threadIdx.x; i < n; i += 256) dt[o + i] = stage_dt[(int64_t)j * stride + i];
}

// the same for the staged azimuth rows of both sides
__global__ __launch_bounds__(256) void odo_gather_az(const int32_t *__restrict__ stage_acur, const int32_t *__restrict__ stage_aprev,
                                                     const int64_t *__restrict__ offsets, int stride, int32_t *__restrict__ a_cur,
                                                     int32_t *__restrict__ a_prev) {
  const int j = blockIdx.x;
  const int64_t o = offsets[j], n = offsets[j + 1] - o;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    a_cur[o + i] = stage_acur[(int64_t)j * stride + i];
    a_prev[o + i] = stage_aprev[(int64_t)j * stride + i];
  }
}

// compensation: a pair whose first pass has status != 0 keeps its first result
__global__ __launch_bounds__(64) void odo_keep_first(const rsx_orora_result *__restrict__ pass1, int n_pairs, rsx_orora_result *__restrict__ pass2) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_pairs) return;
  const rsx_orora_result r = pass1[j];
  if (r.status != 0) pass2[j] = r;
}

// a RANSAC estimator's results in the records rsx_odometry_scan carries (include/rsx.h, rsx_odometry_set_estimator)
__global__ __launch_bounds__(64) void odo_ransac_results(const rsx_ransac_result *__restrict__ in, int n_pairs, rsx_orora_result *__restrict__ out) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_pairs) return;
  const rsx_ransac_result r = in[j];
  rsx_orora_result o;
  o.x = r.x;
  o.y = r.y;
  o.yaw = r.yaw;
  o.iterations = r.hypotheses;
  o.rot_inliers = o.trans_inliers = r.inliers;
  o.status = r.status;
  out[j] = o;
}

// CFEAR: group i of a slot layout owns elements [i * stride, i * stride + counts[i]) (clamp: at most stride of them): the
// ranges csrc/cfear.hip's launches read
__global__ __launch_bounds__(64) void odo_cfear_ranges(const int32_t *__restrict__ counts, int n, int64_t stride, int clamp,
                                                       int64_t *__restrict__ begin, int64_t *__restrict__ end) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int64_t c = counts[i] > 0 ? counts[i] : 0;
  if (clamp && c > stride) c = stride;
  begin[i] = (int64_t)i * stride;
  end[i] = (int64_t)i * stride + c;
}

// CFEAR's results in the records rsx_odometry_scan carries (include/rsx.h, rsx_odometry_set_cfear)
__global__ __launch_bounds__(64) void odo_cfear_results(const rsx_cfear_result *__restrict__ in, int n_pairs, rsx_orora_result *__restrict__ out,
                                                        int32_t *__restrict__ pair_cnt) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_pairs) return;
  const rsx_cfear_result r = in[j];
  rsx_orora_result o;
  o.x = r.x;
  o.y = r.y;
  o.yaw = r.yaw;
  o.iterations = r.iterations;
  o.rot_inliers = o.trans_inliers = r.correspondences;
  o.status = r.status;
  out[j] = o;
  pair_cnt[j] = r.correspondences;
}

// CFEAR with keyframe tracking: the tracker's poses of the n scans of a window as the relative motions rsx_odometry_scan carries.
// Pair (scan i - 1, scan i) gets P_{i-1}^-1 o P_i; the pose before scan 0 is prev (the last scan of the window before), which is then
// replaced by this window's last pose.  One workgroup
__global__ __launch_bounds__(64) void odo_cfear_track_results(const rsx_cfear_track_result *__restrict__ tr, int n, int first, double *prev,
                                                              rsx_orora_result *__restrict__ out, int32_t *__restrict__ pair_cnt) {
  for (int i = first + (int)threadIdx.x; i < n; i += 64) {
    const rsx_cfear_track_result c = tr[i];
    const double px = i > 0 ? tr[i - 1].x : prev[0], py = i > 0 ? tr[i - 1].y : prev[1], pyaw = i > 0 ? tr[i - 1].yaw : prev[2];
    double sn, cs;
    sincos(pyaw, &sn, &cs);
    const double dx = c.x - px, dy = c.y - py;
    rsx_orora_result o;
    o.x = cs * dx + sn * dy;
    o.y = cs * dy - sn * dx;
    o.yaw = c.yaw - pyaw;
    o.iterations = c.reg.iterations;
    o.rot_inliers = o.trans_inliers = c.reg.correspondences;
    o.status = c.reg.status;
    out[i - first] = o;
    pair_cnt[i - first] = c.reg.correspondences;
  }
  __syncthreads();  // (prev has been read)
  if (threadIdx.x == 0) {
    prev[0] = tr[n - 1].x;
    prev[1] = tr[n - 1].y;
    prev[2] = tr[n - 1].yaw;
  }
}

// phase correlation (rsx_odometry_set_phasecorr): the pair list of a window for csrc/phasecorr.hip's pair stage.  Pair j is (src, dst) =
// spectrum slots (first + j + 1, first + j): this scan, the previous one.  res == nullptr: every pair (ESTIMATE).  Otherwise only the
// pairs the selected estimator FAILED on (FALLBACK): status != 0, except `carried` (CFEAR's 8: max_iterations reached, the pose is
// carried); the others get (-1, -1), on which the pair stage computes nothing
__global__ __launch_bounds__(64) void odo_pc_pairs(const rsx_orora_result *__restrict__ res, int n_pairs, int first, int carried,
                                                   int32_t *__restrict__ pairs) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_pairs) return;
  const bool take = !res || (res[j].status != 0 && res[j].status != carried);
  pairs[2 * j] = take ? first + j + 1 : -1;
  pairs[2 * j + 1] = take ? first + j : -1;
}

// phase correlation's results in the records rsx_odometry_scan carries (include/rsx.h, rsx_odometry_set_phasecorr), for the pairs of
// the list; the others' records stay.  pair_cnt (ESTIMATE; null in FALLBACK: the matcher's count stays): 0, there are no matches
__global__ __launch_bounds__(64) void odo_pc_results(const rsx_phasecorr_result *__restrict__ in, const int32_t *__restrict__ pairs, int n_pairs,
                                                     double max_peak_ratio, double min_peak, rsx_orora_result *__restrict__ out,
                                                     int32_t *__restrict__ pair_cnt) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_pairs) return;
  if (pair_cnt) pair_cnt[j] = 0;
  if (pairs[2 * j] < 0) return;
  const rsx_phasecorr_result r = in[j];
  rsx_orora_result o;
  o.x = r.x;
  o.y = r.y;
  o.yaw = r.theta;
  o.iterations = -1 - r.half_turn;
  o.rot_inliers = __double2int_rn(r.peak * 1e6);
  o.trans_inliers = __double2int_rn(r.peak_ratio * 1e6);
  int st = r.status == RSX_PHASECORR_STATUS_ROTATION ? 1 : 0;
  if ((max_peak_ratio > 0.0 && r.peak_ratio > max_peak_ratio) || (min_peak > 0.0 && r.peak < min_peak)) st |= 2;
  o.status = st ? RSX_ODOMETRY_STATUS_PHASECORR | st : 0;
  out[j] = o;
}

}  // namespace

// Round 6: several windows in flight.  A window is two stages: EXTRACTION (cen2019, Cartesian images, descriptors: the wide
// kernels, independent of every other window) and MATCHING (consecutive matches, cross check, max-clique selection, solver:
// a chain of small grids -- one or two workgroups per pair -- that leaves most of the device idle, and the only stage that
// needs the previous window); what the two are under another configuration, OdoNeeds below says.
// While window g is matched, windows g + 1 AND g + 2 are extracted, on two extraction LANES (a
// stream, a cen2019 handle and a front-end handle each; window g takes lane g & 1): the extraction chain has its own narrow
// launches (the selection kernels of cen2019: one workgroup per image) that a second chain fills -- two independent handles
// on one device reach 66.7 k scans/s where one with a single lane reaches 59.3 k.  What the stages hand over -- keypoints,
// descriptors, counts, slots 0 .. n of a SET -- exists three times (window g works in set g % 3); the extraction stage ends
// by copying its last scan into slot 0 of the NEXT set ("the previous scan" of window g + 1).
//   lane g & 1:        E(g):   [wait M(g-3)]  cen2019, Cartesian, describe -> set g%3   [wait M(g-2)]  carry -> set (g+1)%3 slot 0
//   matching stream:   M(g):   [wait E(g), E(g-1)]  match, cross, gather, select + solve -> pinned results g%3
// The host enqueues M(g), then E(g + 2), and only then waits for M(g).
constexpr int N_SETS = 3, N_LANES = 2;

// what the setters of the estimator side select: the ONE value they change, and only to one that check_config accepts
struct OdoConfig {
  int estimator = RSX_ESTIMATOR_ORORA;  // the SELECTED estimator: ORORA, RANSAC, MCRANSAC or CFEAR, never PHASECORR
  bool track = false;  // rsx_odometry_set_cfear_tracking: the keyframe tracker in place of the pair registration
  bool comp = false;  // rsx_odometry_set_compensation
  enum class Pc : uint8_t { off, estimate, fallback } pc = Pc::off;  // rsx_odometry_set_phasecorr: in place of the selected estimator | beside it
};

// what a configuration needs, every question asked once (needs_of) per push: the stages below read these answers, never the configuration
enum class PairStage { features, cfear_pairs, cfear_track, phasecorr };
struct OdoNeeds {
  PairStage stage;  // M(g): matcher, cross check + the estimator | one CFEAR registration launch | one CFEAR tracker launch | phase correlation
  bool desc;  // E(g): Cartesian images and descriptors; the keypoints (xy, counts, desc, valid) are carried
  bool sp, sp_times;  // E(g): CFEAR's surface points, carried; with the records' times (the tracker's compensation)
  bool spectra;  // E(g): the phase-correlation spectra, carried
  size_t pc_F, pc_A;  // bytes of a slot of the two spectrum arrays (0 without spectra)
  bool ransac;  // features: a RANSAC estimator in place of ORORA
  bool match_dt;  // features: the azimuth rows of a match gathered as its dt (MC-RANSAC)
  bool match_rows;  // features: gathered as rows (compensation: a second pass on the compensated matches into results2, out_xy from xy_comp)
  bool fallback;  // M(g): phase correlation once more, over the pairs the stage failed on
};

struct OdoSet {
  rsx::DevBuf az, targets, xy, counts, desc, valid;  // slot 0 = the previous scan, slots 1 .. MAX_WINDOW = the window (whichever extractor wrote them)
  rsx::DevBuf sp, sp_counts, pt_begin, pt_end;  // CFEAR only: surface points [slot][RSX_CFEAR_MAX_SURFACE_POINTS], their counts, the point ranges
  rsx::DevBuf sp_tau;  // CFEAR tracking with compensation only: the records' times, laid out like sp
  rsx::DevBuf pc_F, pc_A;  // phase correlation only: the spectra [slot][N][N] and the angle spectra [slot][N / 2 - 4][N] (csrc/phasecorr.hip)
  rsx::PinnedBuf pin;  // pinned: counts[MAX_WINDOW + 1], pair_cnt[MAX_WINDOW], results[MAX_WINDOW], then the staged azimuth grids
};

struct rsx_odometry {
  int device = 0, rows = 0, cols = 0;
  rsx_odometry_params prm{};
  std::mutex mu;
  rsx::Stream lane_stream[N_LANES], match_stream, copy_stream;
  rsx::Event ev_up, ev_e[N_SETS], ev_m[N_SETS];
  enum class Keypoints { cen2019, cen2018, kstrongest, cfar } keypoints = Keypoints::cen2019;  // the extractor E(g) runs (set_keypoints)
  rsx::Owned<rsx_cen2019, rsx_cen2019_destroy> cen[N_LANES];  // (its parameters: prm.cen)
  rsx::Owned<rsx_cen2018, rsx_cen2018_destroy> cen18[N_LANES];  // created at the first rsx_odometry_set_cen2018, kept across switches
  rsx_cen2018_params cen18_prm{};
  rsx::Owned<rsx_kstrongest, rsx_kstrongest_destroy> kstr[N_LANES];  // created at the first rsx_odometry_set_kstrongest, kept across switches
  rsx_kstrongest_params kstr_prm{};
  rsx::Owned<rsx_cfar, rsx_cfar_destroy> cfar[N_LANES];  // created at the first rsx_odometry_set_cfar, kept across switches
  rsx_cfar_params cfar_prm{};
  rsx::Owned<rsx_frontend, rsx_frontend_destroy> fe[N_LANES];
  rsx::Owned<rsx_orora, rsx_orora_destroy> reg;
  OdoConfig cfg;
  rsx::Owned<rsx_ransac, rsx_ransac_destroy> ransac;  // created at the first rsx_odometry_set_estimator that asks for one
  rsx_ransac_params ransac_prm{};
  rsx::DevBuf ransac_res, stage_dt, dt;  // allocated only with a RANSAC estimator (stage_dt, dt: MC-RANSAC)
  rsx_cfear_params cfear_prm{};  // rsx_odometry_set_cfear
  rsx::DevBuf cfear_res, sp_begin, sp_end;  // allocated only with CFEAR: results of a window, the record ranges of its slots
  rsx::DevBuf cfear_index;  // CFEAR without tracking: the cell-index workspace of a window's pair registration (20 MiB)
  rsx_cfear_track_params track_prm{};
  rsx::DevBuf track_state, track_res, track_n, track_prev;  // allocated only with tracking: the sequence's state (csrc/cfear_track.hip), a
                                                            // window's results, its scan count, the pose of the scan before it
  rsx_mocomp_params comp_prm{};
  rsx::DevBuf stage_acur, stage_aprev, a_cur, a_prev, src2, dst2, results2, xy_comp;  // allocated only with compensation
  rsx_odometry_phasecorr_params pc_prm{};
  rsx_phasecorr_params pc_tables_of{};  // what pc_tables was made for (n == 0: nothing yet)
  rsx::DevBuf pc_tables, pc_work, pc_pairs, pc_res;  // one set of tables for both lanes and the matching stream; a window's pair workspace, list and results
  struct { const uint8_t *d_imgs; int64_t image_stride; int32_t row_stride; } pc_imgs[N_SETS]{};  // where E(g) read window g's images: M(g) samples them again
  OdoSet set[N_SETS];
  rsx::DevBuf imgs[N_SETS], fwd, bwd, stage_src, stage_dst, pair_cnt, src, dst, offsets, results;
  uint64_t windows = 0;  // windows enqueued since creation: window g works in set[g % N_SETS] on lane g & 1
  bool have_prev = false;
};

using rsx::fail;
using Keypoints = rsx_odometry::Keypoints;

namespace {

constexpr size_t PIN_COUNTS = 0, PIN_PAIRS = 4 * (MAX_WINDOW + 1), PIN_RES = PIN_PAIRS + 4 * MAX_WINDOW + 4,
                 PIN_AZ = (PIN_RES + sizeof(rsx_orora_result) * MAX_WINDOW + 255) / 256 * 256;
size_t pin_bytes(const rsx_odometry *h) { return PIN_AZ + (size_t)h->rows * 4 * MAX_WINDOW; }

using Pc = OdoConfig::Pc;

// the rules of a configuration, each once: RSX_OK, or the first one `c` breaks (its message names the calls that lift the conflict)
int check_config(const OdoConfig &c) {
  const bool cfear = c.estimator == RSX_ESTIMATOR_CFEAR, pc = c.pc != Pc::off;
  if (c.track && !cfear) return fail(RSX_ERR_BAD_ARG, "CFEAR registration is not selected (rsx_odometry_set_cfear first)");
  if (c.comp && c.estimator == RSX_ESTIMATOR_MCRANSAC)
    return fail(RSX_ERR_BAD_ARG, "compensation and motion-compensated RANSAC exclude each other: it has its own motion model "
                                 "(rsx_odometry_set_compensation(h, NULL) or rsx_odometry_set_estimator with another estimator first)");
  if (c.comp && cfear)
    return fail(RSX_ERR_BAD_ARG, "compensation and CFEAR registration exclude each other: CFEAR has no matches to compensate "
                                 "(rsx_odometry_set_compensation(h, NULL) or rsx_odometry_set_cfear(h, NULL) first)");
  if (c.comp && pc)
    return fail(RSX_ERR_BAD_ARG, "compensation and phase correlation exclude each other: phase correlation reads the scans as measured "
                                 "(rsx_odometry_set_compensation(h, NULL) or rsx_odometry_set_phasecorr(h, NULL) first)");
  if (c.track && pc)
    return fail(RSX_ERR_BAD_ARG, "the CFEAR tracker and phase correlation, estimator or fallback, exclude each other: the tracker has no pairs "
                                 "(rsx_odometry_set_cfear_tracking(h, NULL) or rsx_odometry_set_phasecorr(h, NULL) first)");
  return RSX_OK;
}

OdoNeeds needs_of(const rsx_odometry *h) {
  const OdoConfig &c = h->cfg;
  OdoNeeds n{};
  n.stage = c.pc == Pc::estimate                  ? PairStage::phasecorr
            : c.estimator != RSX_ESTIMATOR_CFEAR ? PairStage::features
            : c.track                            ? PairStage::cfear_track
                                                 : PairStage::cfear_pairs;
  const bool features = n.stage == PairStage::features;
  n.desc = features;  // (phase correlation as the estimator reports the keypoints and matches none: no descriptors, nothing of them carried)
  n.sp = n.stage == PairStage::cfear_pairs || n.stage == PairStage::cfear_track;
  n.sp_times = n.stage == PairStage::cfear_track && h->track_prm.compensate;
  n.spectra = c.pc != Pc::off;  // (slot 0 of a set is only read while the handle holds a scan, and N cannot change then)
  if (n.spectra) rsx::phasecorr::workspace_bytes(h->pc_prm.pc.n, &n.pc_F, &n.pc_A, nullptr);
  n.ransac = features && c.estimator != RSX_ESTIMATOR_ORORA;
  n.match_dt = features && c.estimator == RSX_ESTIMATOR_MCRANSAC;
  n.match_rows = features && c.comp;
  n.fallback = c.pc == Pc::fallback;  // (never with compensation or the tracker: the records it replaces are h->results)
  return n;
}

// the arrays of an OdoSet with a slot per scan (slot 0 = the previous scan), in the order the carry copies them: reserved for
// MAX_WINDOW + 1 slots of `bytes` when `on`, and the window's last slot copied into slot 0 of the next set when `carried`
struct SlotArray { rsx::DevBuf OdoSet::*buf; size_t bytes; bool keep, on, carried; };  // (keep: the contents, when the buffer grows)
using SlotArrays = std::array<SlotArray, 10>;
SlotArrays slot_arrays(const rsx_odometry *h, const OdoNeeds &need) {
  constexpr size_t SP = RSX_CFEAR_MAX_SURFACE_POINTS;
  const size_t K = (size_t)h->prm.max_keypoints;
  return {{{&OdoSet::pc_F, need.pc_F, true, need.spectra, need.spectra},
           {&OdoSet::pc_A, need.pc_A, true, need.spectra, need.spectra},
           {&OdoSet::sp, SP * sizeof(rsx_cfear_surface_point), true, need.sp, need.sp},
           {&OdoSet::sp_counts, 4, true, need.sp, need.sp},
           {&OdoSet::sp_tau, SP * 4, false, need.sp_times, false},  // (the tracker reads the window's own slots only)
           {&OdoSet::xy, K * 8, true, true, need.desc},  // (every extractor writes xy, counts and targets, whatever reads them)
           {&OdoSet::desc, K * 32, true, true, need.desc},
           {&OdoSet::valid, K, true, true, need.desc},
           {&OdoSet::counts, 4, true, true, need.desc},
           {&OdoSet::targets, K * 8, false, true, need.match_dt || need.match_rows}}};  // (the rows of the previous scan's keypoints: the straddling pair)
}

int reserve_all(rsx_odometry *h, const OdoNeeds &need, const SlotArrays &slots, size_t ibytes, hipStream_t s) {
  const size_t K = (size_t)h->prm.max_keypoints, S = MAX_WINDOW + 1;
  for (rsx::DevBuf &b : h->imgs) RSX_TRY(b.reserve(ibytes * MAX_WINDOW, s, false));
  for (OdoSet &q : h->set) {
    RSX_TRY(q.az.reserve((size_t)h->rows * 4 * MAX_WINDOW, s, false));
    for (const SlotArray &a : slots)
      if (a.on) RSX_TRY((q.*a.buf).reserve(S * a.bytes, s, a.keep));
    if (need.sp)
      for (rsx::DevBuf *b : {&q.pt_begin, &q.pt_end}) RSX_TRY(b->reserve((size_t)MAX_WINDOW * 8, s, false));
  }
  for (rsx::DevBuf *b : {&h->fwd, &h->bwd}) RSX_TRY(b->reserve((size_t)MAX_WINDOW * K * 4, s, false));
  for (rsx::DevBuf *b : {&h->stage_src, &h->stage_dst, &h->src, &h->dst}) RSX_TRY(b->reserve((size_t)MAX_WINDOW * K * 8, s, false));
  RSX_TRY(h->pair_cnt.reserve((size_t)MAX_WINDOW * 4, s, false));
  RSX_TRY(h->offsets.reserve((size_t)(MAX_WINDOW + 1) * 8, s, false));
  RSX_TRY(h->results.reserve((size_t)MAX_WINDOW * sizeof(rsx_orora_result), s, false));
  if (need.sp) {
    RSX_TRY(h->cfear_res.reserve((size_t)MAX_WINDOW * sizeof(rsx_cfear_result), s, false));
    for (rsx::DevBuf *b : {&h->sp_begin, &h->sp_end}) RSX_TRY(b->reserve(S * 8, s, false));
    if (need.stage == PairStage::cfear_track) {
      RSX_TRY(h->track_state.reserve(rsx::cfear::track_state_bytes(), s, false));
      RSX_TRY(h->track_res.reserve((size_t)MAX_WINDOW * sizeof(rsx_cfear_track_result), s, false));
      RSX_TRY(h->track_n.reserve(4, s, false));
      RSX_TRY(h->track_prev.reserve(24, s, false));
    } else RSX_TRY(h->cfear_index.reserve(rsx::cfear::keyframe_index_bytes(MAX_WINDOW), s, false));
  }
  if (need.ransac) RSX_TRY(h->ransac_res.reserve((size_t)MAX_WINDOW * sizeof(rsx_ransac_result), s, false));
  if (need.match_dt)
    for (rsx::DevBuf *b : {&h->stage_dt, &h->dt}) RSX_TRY(b->reserve((size_t)MAX_WINDOW * K * 4, s, false));
  if (need.match_rows) {
    for (rsx::DevBuf *b : {&h->stage_acur, &h->stage_aprev, &h->a_cur, &h->a_prev}) RSX_TRY(b->reserve((size_t)MAX_WINDOW * K * 4, s, false));
    for (rsx::DevBuf *b : {&h->src2, &h->dst2, &h->xy_comp}) RSX_TRY(b->reserve((size_t)MAX_WINDOW * K * 8, s, false));
    RSX_TRY(h->results2.reserve((size_t)MAX_WINDOW * sizeof(rsx_orora_result), s, false));
  }
  if (need.spectra) {
    size_t per_pair;
    rsx::phasecorr::workspace_bytes(h->pc_prm.pc.n, nullptr, nullptr, &per_pair);
    RSX_TRY(h->pc_work.reserve((size_t)MAX_WINDOW * per_pair + 64, s, false));
    RSX_TRY(h->pc_pairs.reserve((size_t)MAX_WINDOW * 8, s, false));
    RSX_TRY(h->pc_res.reserve((size_t)MAX_WINDOW * sizeof(rsx_phasecorr_result), s, false));
  }
  return RSX_OK;
}

// E(g): window g (n <= MAX_WINDOW scans whose images are at d_imgs, device) through the selected extractor and what `need` asks of every
// scan into set g % 3, then its last scan into slot 0 of the next set.  Asynchronous on the stream of lane g & 1.
int enqueue_extract(rsx_odometry *h, const OdoNeeds &need, const SlotArrays &slots, uint64_t g, const uint8_t *d_imgs, int n, int64_t img_stride, int32_t row_stride,
                    const float *azimuths, int32_t azimuths_per_image) {
  const int lane = (int)(g & 1);
  hipStream_t s = h->lane_stream[lane];
  OdoSet &q = h->set[g % N_SETS], &nx = h->set[(g + 1) % N_SETS];
  const int K = h->prm.max_keypoints;
  const size_t slot_xy = (size_t)K * 2;
  RSX_HIP(hipStreamWaitEvent(s, h->ev_m[g % N_SETS], 0));  // M(g - 3) read this set (a no-op before the event's first record)
  // the azimuth grids go to the device once: cen2019's polar -> Cartesian and the Cartesian image both read them there.
  // Staged in pinned memory so that the copy does not wait for the stream (the area was last read by E(g - 3): long done)
  const size_t na = (size_t)h->rows * (azimuths_per_image ? n : 1);
  float *paz = reinterpret_cast<float *>(static_cast<char *>(q.pin.p) + PIN_AZ);
  std::memcpy(paz, azimuths, na * 4);
  RSX_HIP(hipMemcpyAsync(q.az.p, paz, na * 4, hipMemcpyHostToDevice, s));
  int32_t *d_counts = q.counts.as<int32_t>();
  auto keypoints = [&](auto extract_batch_device, auto *cen, const auto *prm) {
    return extract_batch_device(cen, d_imgs, n, img_stride, row_stride, h->prm.col_offset, prm, q.az.as<float>(), azimuths_per_image,
                                h->prm.radar_resolution, q.targets.as<int32_t>() + slot_xy, q.xy.as<float>() + slot_xy, K, d_counts + 1, s);
  };
  switch (h->keypoints) {
    case Keypoints::cen2019: RSX_TRY(keypoints(rsx_cen2019_extract_batch_device, h->cen[lane].get(), &h->prm.cen)); break;
    case Keypoints::cen2018: RSX_TRY(keypoints(rsx_cen2018_extract_batch_device, h->cen18[lane].get(), &h->cen18_prm)); break;
    case Keypoints::kstrongest: RSX_TRY(keypoints(rsx_kstrongest_extract_batch_device, h->kstr[lane].get(), &h->kstr_prm)); break;
    case Keypoints::cfar: RSX_TRY(keypoints(rsx_cfar_extract_batch_device, h->cfar[lane].get(), &h->cfar_prm)); break;
  }
  if (need.spectra) {  // the spectra of every scan into slots 1 .. n; M(g) samples the images once more
    h->pc_imgs[g % N_SETS] = {d_imgs, img_stride, row_stride};
    RSX_TRY(rsx::phasecorr::launch_spectra(h->pc_prm.pc, h->rows, h->cols, h->pc_tables.p, {d_imgs, img_stride, row_stride, h->prm.col_offset}, n,
                                           reinterpret_cast<float2 *>(q.pc_F.as<char>() + need.pc_F), reinterpret_cast<float2 *>(q.pc_A.as<char>() + need.pc_A),
                                           nullptr, s));
  }
  if (need.sp) {  // the surface points of every scan
    constexpr size_t SP = RSX_CFEAR_MAX_SURFACE_POINTS;
    hipLaunchKernelGGL(odo_cfear_ranges, dim3((unsigned)(n + 63) / 64), dim3(64), 0, s, d_counts + 1, n, (int64_t)K, 1, q.pt_begin.as<int64_t>(),
                       q.pt_end.as<int64_t>());
    RSX_HIP(hipGetLastError());
    if (need.sp_times)  // with the records' times: a keypoint's azimuth row is the first word of its target
      RSX_TRY(rsx::cfear::launch_surface_timed(q.xy.as<float>() + slot_xy, q.targets.as<int32_t>() + slot_xy, 2, h->rows, q.pt_begin.as<int64_t>(),
                                               q.pt_end.as<int64_t>(), n, h->cfear_prm, q.sp.as<rsx_cfear_surface_point>() + SP,
                                               q.sp_tau.as<float>() + SP, (int32_t)SP, q.sp_counts.as<int32_t>() + 1, nullptr, s));
    else
      RSX_TRY(rsx::cfear::launch_surface(q.xy.as<float>() + slot_xy, q.pt_begin.as<int64_t>(), q.pt_end.as<int64_t>(), n, h->cfear_prm,
                                         q.sp.as<rsx_cfear_surface_point>() + SP, (int32_t)SP, q.sp_counts.as<int32_t>() + 1, nullptr, s));
  }
  if (need.desc) {
    // the Cartesian image of scan i through scan i's OWN azimuth grid (already in HBM for cen2019): results do not depend on
    // how the sequence is cut into windows, and nothing about the grids is looked at on the host
    RSX_TRY(rsx_frontend_cartesian_batch_device_az(h->fe[lane].get(), d_imgs, n, img_stride, row_stride, h->prm.col_offset, q.az.as<float>(),
                                                   azimuths_per_image ? (int64_t)h->rows : 0, h->prm.radar_resolution, s));
    RSX_TRY(rsx_frontend_describe_batch_device(h->fe[lane].get(), q.xy.as<float>() + slot_xy, d_counts + 1, n, K, q.desc.as<uint8_t>() + (size_t)K * 32,
                                               q.valid.as<uint8_t>() + (size_t)K, s));
  }
  // the last scan of the window becomes the previous scan of the next one (slot 0 of the next set, which M(g - 2) read; the
  // next window's own extraction, on the other lane, writes slots 1 .. n of that set only)
  RSX_HIP(hipStreamWaitEvent(s, h->ev_m[(g + 1) % N_SETS], 0));
  for (const SlotArray &a : slots)
    if (a.carried) RSX_HIP(hipMemcpyAsync((nx.*a.buf).p, (q.*a.buf).as<char>() + (size_t)n * a.bytes, a.bytes, hipMemcpyDeviceToDevice, s));
  RSX_HIP(hipEventRecord(h->ev_e[g % N_SETS], s));
  return RSX_OK;
}

// M(g): the consecutive pairs of window g (with the previous scan in slot 0 when there is one) through the pair stage of `need`,
// the results on their way to the set's pinned area.  Asynchronous on the matching stream.  *first_out: 0 when slot 0 takes part.
int enqueue_match(rsx_odometry *h, const OdoNeeds &need, uint64_t g, int n, int *first_out, bool want_xy) {
  hipStream_t s = h->match_stream;
  OdoSet &q = h->set[g % N_SETS];
  const int K = h->prm.max_keypoints;
  RSX_HIP(hipStreamWaitEvent(s, h->ev_e[g % N_SETS], 0));
  RSX_HIP(hipStreamWaitEvent(s, h->ev_e[(g + N_SETS - 1) % N_SETS], 0));  // E(g - 1): its carry into slot 0 (the other lane's stream)
  int32_t *d_counts = q.counts.as<int32_t>();
  const int first = h->have_prev ? 0 : 1, n_pairs = n - first;
  *first_out = first;
  // phase correlation over the pairs of the list odo_pc_pairs writes: src = spectrum slot first + j + 1 = image first + j of window g
  // (image = slot - 1), dst = slot first + j, slot 0 being the scan the window before carried here.  As the fallback only over the pairs
  // the stage before it failed on (CFEAR's status 8 is no failure: max_iterations reached, the pose is carried)
  auto phasecorr = [&](bool fallback) -> int {
    int32_t *pairs = h->pc_pairs.as<int32_t>();
    rsx_orora_result *rec = h->results.as<rsx_orora_result>();
    const dim3 grid((unsigned)(n_pairs + 63) / 64), blk(64);
    hipLaunchKernelGGL(odo_pc_pairs, grid, blk, 0, s, fallback ? rec : (const rsx_orora_result *)nullptr, n_pairs, first,
                       need.stage == PairStage::cfear_pairs ? 8 : 0, pairs);
    RSX_HIP(hipGetLastError());
    const auto &im = h->pc_imgs[g % N_SETS];
    RSX_TRY(rsx::phasecorr::launch_pairs(h->pc_prm.pc, h->rows, h->cols, h->pc_tables.p, {im.d_imgs, im.image_stride, im.row_stride, h->prm.col_offset}, n,
                                         -1, q.pc_F.as<float2>(), q.pc_A.as<float2>(), n + 1, pairs, n_pairs, h->pc_work.p,
                                         h->pc_res.as<rsx_phasecorr_result>(), s));
    hipLaunchKernelGGL(odo_pc_results, grid, blk, 0, s, h->pc_res.as<rsx_phasecorr_result>(), pairs, n_pairs, h->pc_prm.max_peak_ratio,
                       h->pc_prm.min_peak, rec, fallback ? (int32_t *)nullptr : h->pair_cnt.as<int32_t>());
    RSX_HIP(hipGetLastError());
    return RSX_OK;
  };
  int64_t *b = h->sp_begin.as<int64_t>(), *e = h->sp_end.as<int64_t>();
  auto sp_ranges = [&]() -> int {  // CFEAR: the record ranges of slots 0 .. n of the set's surface points into b, e
    hipLaunchKernelGGL(odo_cfear_ranges, dim3((unsigned)(n + 1 + 63) / 64), dim3(64), 0, s, q.sp_counts.as<int32_t>(), n + 1,
                       (int64_t)RSX_CFEAR_MAX_SURFACE_POINTS, 0, b, e);
    RSX_HIP(hipGetLastError());
    return RSX_OK;
  };
  if (need.stage == PairStage::phasecorr) {
    if (n_pairs > 0) RSX_TRY(phasecorr(false));
  } else if (need.stage == PairStage::cfear_track) {  // one tracker launch over the window's scans (slots 1 .. n), its state in the handle
    if (!h->have_prev) RSX_HIP(hipMemsetAsync(h->track_state.p, 0, rsx::cfear::track_state_bytes(), s));  // a new sequence
    RSX_TRY(sp_ranges());
    RSX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->track_n.p), n, 1, s));
    RSX_TRY(rsx::cfear::launch_track(q.sp.as<rsx_cfear_surface_point>(), need.sp_times ? q.sp_tau.as<float>() : nullptr, b + 1, e + 1, h->track_n.as<int32_t>(), 1,
                                     h->cfear_prm, h->track_prm, h->track_state.p, h->track_res.as<rsx_cfear_track_result>(), s));
    hipLaunchKernelGGL(odo_cfear_track_results, dim3(1), dim3(64), 0, s, h->track_res.as<rsx_cfear_track_result>(), n, first,
                       h->track_prev.as<double>(), h->results.as<rsx_orora_result>(), h->pair_cnt.as<int32_t>());
    RSX_HIP(hipGetLastError());
  } else if (n_pairs > 0 && need.stage == PairStage::cfear_pairs) {  // one registration launch over the pairs; src = slot first + j + 1, dst = slot first + j
    RSX_TRY(sp_ranges());
    const rsx_cfear_surface_point *sp = q.sp.as<rsx_cfear_surface_point>();
    RSX_TRY(rsx::cfear::launch_register(sp, b + first + 1, e + first + 1, sp, b + first, e + first, n_pairs, nullptr, h->cfear_prm,
                                        h->cfear_index.p, h->cfear_res.as<rsx_cfear_result>(), s));
    hipLaunchKernelGGL(odo_cfear_results, dim3((unsigned)(n_pairs + 63) / 64), dim3(64), 0, s, h->cfear_res.as<rsx_cfear_result>(), n_pairs,
                       h->results.as<rsx_orora_result>(), h->pair_cnt.as<int32_t>());
    RSX_HIP(hipGetLastError());
  } else if (n_pairs > 0) {  // features: matcher, cross check, correspondence lists and the estimator
    RSX_TRY(rsx_frontend_match_consecutive_device(h->fe[g & 1].get(), q.desc.as<uint8_t>(), q.valid.as<uint8_t>(), d_counts, K, first, n_pairs,
                                                  h->prm.frontend.ratio, h->fwd.as<int32_t>(), h->bwd.as<int32_t>(), s));
    auto cross = [&](auto kernel, auto... more) {  // the cross check; `more`: what it stages beside the matches, and from what
      hipLaunchKernelGGL(kernel, dim3((unsigned)n_pairs), dim3(256), 0, s, q.xy.as<float>(), d_counts, K, first, h->fwd.as<int32_t>(),
                         h->bwd.as<int32_t>(), h->stage_src.as<float2>(), h->stage_dst.as<float2>(), h->pair_cnt.as<int32_t>(), more...);
    };
    if (need.match_rows) cross(odo_cross_az, q.targets.as<int32_t>(), h->stage_acur.as<int32_t>(), h->stage_aprev.as<int32_t>());
    else if (need.match_dt) cross(odo_cross_dt, q.targets.as<int32_t>(), h->rows, h->ransac_prm.dt_scan, h->stage_dt.as<float>());
    else cross(odo_cross);
    hipLaunchKernelGGL(odo_gather, dim3((unsigned)n_pairs), dim3(256), 0, s, h->stage_src.as<float2>(), h->stage_dst.as<float2>(),
                       h->pair_cnt.as<int32_t>(), n_pairs, K, h->src.as<float2>(), h->dst.as<float2>(), h->offsets.as<int64_t>());
    if (need.match_dt)
      hipLaunchKernelGGL(odo_gather_dt, dim3((unsigned)n_pairs), dim3(256), 0, s, h->stage_dt.as<float>(), h->offsets.as<int64_t>(), K, h->dt.as<float>());
    if (need.match_rows)
      hipLaunchKernelGGL(odo_gather_az, dim3((unsigned)n_pairs), dim3(256), 0, s, h->stage_acur.as<int32_t>(), h->stage_aprev.as<int32_t>(),
                         h->offsets.as<int64_t>(), K, h->a_cur.as<int32_t>(), h->a_prev.as<int32_t>());
    RSX_HIP(hipGetLastError());
    auto estimate = [&](const float *d_src, const float *d_dst, rsx_orora_result *d_res) -> int {
      if (!need.ransac) return rsx_orora_register_batch_device(h->reg.get(), d_src, d_dst, h->offsets.as<int64_t>(), n_pairs, &h->prm.orora, d_res, s);
      RSX_TRY(rsx_ransac_estimate_batch_device(h->ransac.get(), d_src, d_dst, need.match_dt ? h->dt.as<float>() : nullptr, h->offsets.as<int64_t>(),
                                               n_pairs, &h->ransac_prm, h->ransac_res.as<rsx_ransac_result>(), nullptr, s));
      hipLaunchKernelGGL(odo_ransac_results, dim3((unsigned)(n_pairs + 63) / 64), dim3(64), 0, s, h->ransac_res.as<rsx_ransac_result>(), n_pairs, d_res);
      RSX_HIP(hipGetLastError());
      return RSX_OK;
    };
    RSX_TRY(estimate(h->src.as<float>(), h->dst.as<float>(), h->results.as<rsx_orora_result>()));
    if (need.match_rows) {  // estimated, compensated with its own estimate, estimated again: every pair of the window in each launch
      RSX_TRY(rsx::mocomp::launch_matches(h->src.as<float>(), h->dst.as<float>(), h->a_cur.as<int32_t>(), h->a_prev.as<int32_t>(),
                                          h->offsets.as<int64_t>(), n_pairs, h->results.p, sizeof(rsx_orora_result), offsetof(rsx_orora_result, status),
                                          h->comp_prm, h->src2.as<float>(), h->dst2.as<float>(), nullptr, s));
      RSX_TRY(estimate(h->src2.as<float>(), h->dst2.as<float>(), h->results2.as<rsx_orora_result>()));
      hipLaunchKernelGGL(odo_keep_first, dim3((unsigned)(n_pairs + 63) / 64), dim3(64), 0, s, h->results.as<rsx_orora_result>(), n_pairs,
                         h->results2.as<rsx_orora_result>());
      RSX_HIP(hipGetLastError());
    }
  }
  if (need.fallback && n_pairs > 0) RSX_TRY(phasecorr(true));  // (never with compensation or the tracker: the records are h->results)
  const rsx::DevBuf &res = need.match_rows ? h->results2 : h->results;
  if (need.match_rows && want_xy)  // /orora/cloud_local: scan i under the velocity of the pair (i - 1, i); the first scan of a sequence as measured
    RSX_TRY(rsx::mocomp::launch_slots(q.xy.as<float>() + (size_t)K * 2, q.targets.as<int32_t>() + (size_t)K * 2, d_counts + 1, K, n, first, res.p,
                                      sizeof(rsx_orora_result), offsetof(rsx_orora_result, status), h->comp_prm, h->xy_comp.as<float>(), s));
  char *pin = static_cast<char *>(q.pin.p);
  RSX_HIP(hipMemcpyAsync(pin + PIN_COUNTS, d_counts, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, s));
  if (n_pairs > 0) {
    RSX_HIP(hipMemcpyAsync(pin + PIN_PAIRS, h->pair_cnt.p, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, s));
    RSX_HIP(hipMemcpyAsync(pin + PIN_RES, res.p, (size_t)n_pairs * sizeof(rsx_orora_result), hipMemcpyDeviceToHost, s));
  }
  RSX_HIP(hipEventRecord(h->ev_m[g % N_SETS], s));
  h->have_prev = true;
  return RSX_OK;
}

// wait for M(g), fill out[0..n) (+ the keypoints)
int finish_window(rsx_odometry *h, const OdoNeeds &need, uint64_t g, int n, int first, rsx_odometry_scan *out, float *out_xy, int32_t max_xy) {
  OdoSet &q = h->set[g % N_SETS];
  const int K = h->prm.max_keypoints;
  const size_t slot_xy = (size_t)K * 2;
  char *pin = static_cast<char *>(q.pin.p);
  RSX_HIP(hipEventSynchronize(h->ev_m[g % N_SETS]));
  const int32_t *hc = reinterpret_cast<const int32_t *>(pin + PIN_COUNTS), *hp = reinterpret_cast<const int32_t *>(pin + PIN_PAIRS);
  const rsx_orora_result *hr = reinterpret_cast<const rsx_orora_result *>(pin + PIN_RES);
  for (int i = 0; i < n; i++) {
    rsx_odometry_scan &o = out[i];
    std::memset(&o, 0, sizeof(o));
    o.n_keypoints = hc[1 + i];
    const int pair = first ? i - 1 : i;  // index of the pair (scan i-1, scan i) in this window
    if (pair >= 0) {
      o.reg = hr[pair];
      o.n_matches = hp[pair];
    } else {
      o.reg.status = 3;  // the first scan of a sequence: there is no previous scan
    }
  }
  if (out_xy && max_xy > 0) {  // (set g % 3 is not written again before E(g + 3), which the host enqueues after this returns)
    hipStream_t s = h->match_stream;
    for (int i = 0; i < n; i++) {
      const int c = hc[1 + i] < K ? hc[1 + i] : K, wn = c < max_xy ? c : max_xy;
      if (wn > 0)
        RSX_HIP(hipMemcpyAsync(out_xy + (size_t)i * max_xy * 2,
                               need.match_rows ? h->xy_comp.as<float>() + (size_t)i * slot_xy : q.xy.as<float>() + (size_t)(1 + i) * slot_xy,
                               (size_t)wn * 8, hipMemcpyDeviceToHost, s));
    }
    RSX_HIP(hipStreamSynchronize(s));
  }
  return RSX_OK;
}

// after an error in the middle of a sequence: nothing in flight, the next scan starts a new sequence
void abandon(rsx_odometry *h) {
  for (hipStream_t ls : h->lane_stream) (void)hipStreamSynchronize(ls);
  (void)hipStreamSynchronize(h->match_stream);
  h->have_prev = false;
}

// the azimuth grids are host arrays here: every grid must ascend (the Cartesian remap divides by az[1] - az[0] on the
// device, frontend.hip az_row_of: a zero or negative step would give NaN row indices and NaN images instead of a status)
int check_azimuths(const rsx_odometry *h, const float *azimuths, int32_t per_image, int32_t n_scans) {
  if (h->rows < 2) return RSX_OK;
  const int grids = per_image ? n_scans : 1;
  for (int g = 0; g < grids; g++) {
    const float *az = azimuths + (size_t)g * h->rows;
    if (!((double)az[1] - (double)az[0] > 0.0)) return fail(RSX_ERR_BAD_ARG, "azimuths must increase (scan %d)", g);
  }
  return RSX_OK;
}

// the arguments of rsx_odometry_push / rsx_odometry_push_device (imgs: host or device)
int check_push(rsx_odometry *h, const uint8_t *imgs, int32_t n_scans, int64_t image_stride_bytes, int32_t row_stride, const float *azimuths,
               int32_t azimuths_per_image, const rsx_odometry_scan *out, int32_t max_xy) {
  if (!h || !imgs || !azimuths || !out || n_scans < 0 || max_xy < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  if (n_scans == 0) return RSX_OK;
  RSX_TRY(rsx::check_polar_layout(h->rows, h->cols, n_scans, image_stride_bytes, row_stride, h->prm.col_offset));
  return check_azimuths(h, azimuths, azimuths_per_image, n_scans);
}

// the windows of one call, three in flight: E(0), E(1), then per window M(g), E(g + 2) -- two extractions run beside this window's
// matching -- and the wait for M(g).  stage(w, g, b0, n) enqueues E(g) of the call's window w (scans b0 .. b0 + n) once its images
// are where the extraction can read them
template <typename Stage>
int push_windows(rsx_odometry *h, const OdoNeeds &need, int32_t n_scans, rsx_odometry_scan *out, float *out_xy, int32_t max_xy, Stage &&stage) {
  const int nwin = (n_scans + MAX_WINDOW - 1) / MAX_WINDOW;
  auto extract = [&](int w, uint64_t g) -> int {
    const int b0 = w * MAX_WINDOW;
    return stage(w, g, b0, n_scans - b0 < MAX_WINDOW ? n_scans - b0 : MAX_WINDOW);
  };
  int st = extract(0, h->windows);
  if (st == RSX_OK && nwin > 1) st = extract(1, h->windows + 1);
  for (int w = 0; w < nwin && st == RSX_OK; w++) {
    const uint64_t g = h->windows + (uint64_t)w;
    const int b0 = w * MAX_WINDOW, n = n_scans - b0 < MAX_WINDOW ? n_scans - b0 : MAX_WINDOW;
    int first = 0;
    st = enqueue_match(h, need, g, n, &first, out_xy && max_xy > 0);
    if (st == RSX_OK && w + 2 < nwin) st = extract(w + 2, g + 2);
    if (st == RSX_OK) st = finish_window(h, need, g, n, first, out + b0, out_xy ? out_xy + (size_t)b0 * max_xy * 2 : nullptr, max_xy);
  }
  h->windows += (uint64_t)nwin;
  if (st != RSX_OK) abandon(h);
  return st;
}

// rsx_odometry_set_cen2018 / rsx_odometry_set_kstrongest / rsx_odometry_set_cfar: params == NULL selects cen2019 again; otherwise extractor `which` with
// *params (checked), its handle of every lane (h->*lanes) created when first needed and kept across later switches
template <typename P, typename H, auto Destroy>
int set_keypoints(rsx_odometry *h, Keypoints which, const P *params, int (*check_params)(const P &), int (*create)(int, int32_t, int32_t, H **),
                  rsx::Owned<H, Destroy> (rsx_odometry::*lanes)[N_LANES], P rsx_odometry::*prm) {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->have_prev) return fail(RSX_ERR_BAD_ARG, "the handle holds a scan: rsx_odometry_reset first (one pair, one extractor)");
  if (!params) {
    h->keypoints = Keypoints::cen2019;
    return RSX_OK;
  }
  RSX_TRY(check_params(*params));
  for (auto &lane : h->*lanes) {
    if (lane) continue;
    H *c = nullptr;
    RSX_TRY(create(h->device, h->rows, h->cols, &c));
    lane.reset(c);
  }
  h->*prm = *params;
  h->keypoints = which;
  return RSX_OK;
}

// The setters of the estimator side, all in this one sequence: candidate(c, p) turns the current configuration and the setter's stored
// parameters (h->*prm) into the call's and checks the parameters; check_config on the candidate; and only then both are stored -- a call
// that fails leaves the configuration as it was.  one: what a sequence has one of
template <typename P, typename Candidate>
int set_config(rsx_odometry *h, const char *one, P rsx_odometry::*prm, Candidate &&candidate) {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->have_prev) return fail(RSX_ERR_BAD_ARG, "the handle holds a scan: rsx_odometry_reset first (one sequence, one %s)", one);
  OdoConfig c = h->cfg;
  P p = h->*prm;
  RSX_TRY(candidate(c, p));
  RSX_TRY(check_config(c));
  h->*prm = p;
  h->cfg = c;
  return RSX_OK;
}

}  // namespace

extern "C" {

int rsx_odometry_default_params(rsx_odometry_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  std::memset(p, 0, sizeof(*p));
  rsx_cen2019_default_params(&p->cen);
  rsx_frontend_default_params(&p->frontend);
  rsx_orora_default_params(&p->orora);
  p->orora.flags |= RSX_ORORA_PMC;  // the upstream pipeline prunes the matches to the max clique before the solver (csrc/pmc.hip)
  p->radar_resolution = 0.0595f;  // Navtech CIR204-H range bin [m] (MulRan)
  p->col_offset = 11;             // metadata bytes in front of every polar_oxford_form row
  p->max_keypoints = 16384;  // = rsx_orora_max_correspondences(): a pair can never exceed the solver's capacity
  p->device = 0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_odometry_create(const rsx_odometry_params *params, int32_t rows, int32_t cols, rsx_odometry **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  rsx_odometry_params p;
  rsx_odometry_default_params(&p);
  if (params) p = *params;
  if (p.max_keypoints < 16 || p.max_keypoints > rsx_orora_max_correspondences())
    return fail(RSX_ERR_BAD_ARG, "max_keypoints %d outside [16, %d]", p.max_keypoints, rsx_orora_max_correspondences());
  if (p.col_offset < 0 || !(p.radar_resolution > 0.0f)) return fail(RSX_ERR_BAD_ARG, "bad col_offset / radar_resolution");
  std::unique_ptr<rsx_odometry> h(new (std::nothrow) rsx_odometry());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = p.device;
  h->rows = rows;
  h->cols = cols;
  h->prm = p;
  for (int l = 0; l < N_LANES; l++) {
    rsx_cen2019 *cen = nullptr;
    rsx_frontend *fe = nullptr;
    RSX_TRY(rsx_cen2019_create(p.device, rows, cols, &cen));
    h->cen[l].reset(cen);
    RSX_TRY(rsx_frontend_create(p.device, rows, cols, &p.frontend, &fe));
    h->fe[l].reset(fe);
  }
  rsx_orora *reg = nullptr;
  RSX_TRY(rsx_orora_create(p.device, &reg));
  h->reg.reset(reg);
  if (p.orora.flags & RSX_ORORA_PMC) RSX_TRY(rsx_orora_reserve(reg, (int64_t)MAX_WINDOW * p.max_keypoints));
  hipError_t e = hipSetDevice(p.device);
  for (rsx::Stream &ls : h->lane_stream)
    if (e == hipSuccess) e = ls.create();
  if (e == hipSuccess) e = h->match_stream.create();
  if (e == hipSuccess) e = h->copy_stream.create();
  if (e == hipSuccess) e = h->ev_up.create();
  for (int i = 0; i < N_SETS; i++) {
    if (e == hipSuccess) e = h->ev_e[i].create();
    if (e == hipSuccess) e = h->ev_m[i].create();
  }
  if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RSX_ERR_OOM : RSX_ERR_HIP, "odometry create: %s", hipGetErrorString(e));
  for (OdoSet &q : h->set) RSX_TRY(q.pin.reserve(pin_bytes(h.get())));
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_odometry_destroy(rsx_odometry *h) try {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  for (hipStream_t ls : h->lane_stream)
    if (ls) (void)hipStreamSynchronize(ls);
  if (h->match_stream) (void)hipStreamSynchronize(h->match_stream);
  if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_odometry_reset(rsx_odometry *h) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  h->have_prev = false;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_odometry_window(void) { return MAX_WINDOW; }

int rsx_odometry_set_cen2018(rsx_odometry *h, const rsx_cen2018_params *params) try {
  return set_keypoints(h, Keypoints::cen2018, params, rsx::cen2018_check_params, rsx_cen2018_create, &rsx_odometry::cen18, &rsx_odometry::cen18_prm);
} RSX_CATCH_ALL

int rsx_odometry_set_kstrongest(rsx_odometry *h, const rsx_kstrongest_params *params) try {
  return set_keypoints(h, Keypoints::kstrongest, params, rsx::kstrongest_check_params, rsx_kstrongest_create, &rsx_odometry::kstr, &rsx_odometry::kstr_prm);
} RSX_CATCH_ALL

int rsx_odometry_set_cfar(rsx_odometry *h, const rsx_cfar_params *params) try {
  return set_keypoints(h, Keypoints::cfar, params, rsx::cfar_check_params, rsx_cfar_create, &rsx_odometry::cfar, &rsx_odometry::cfar_prm);
} RSX_CATCH_ALL

int rsx_odometry_set_estimator(rsx_odometry *h, int estimator, const rsx_ransac_params *params) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  if (estimator == RSX_ESTIMATOR_CFEAR) return fail(RSX_ERR_BAD_ARG, "RSX_ESTIMATOR_CFEAR is selected with rsx_odometry_set_cfear, which carries its parameters");
  if (estimator == RSX_ESTIMATOR_PHASECORR)
    return fail(RSX_ERR_BAD_ARG, "RSX_ESTIMATOR_PHASECORR is selected with rsx_odometry_set_phasecorr, which carries its parameters");
  if (estimator != RSX_ESTIMATOR_ORORA && estimator != RSX_ESTIMATOR_RANSAC && estimator != RSX_ESTIMATOR_MCRANSAC)
    return fail(RSX_ERR_BAD_ARG, "unknown estimator %d", estimator);
  const bool ransac = estimator != RSX_ESTIMATOR_ORORA;
  return set_config(h, "estimator", &rsx_odometry::ransac_prm, [&](OdoConfig &c, rsx_ransac_params &p) -> int {
    c.estimator = estimator;
    c.track = false;  // (tracking belongs to CFEAR)
    if (c.pc == Pc::estimate) c.pc = Pc::off;  // (selecting an estimator leaves the one that stood in for it)
    if (!ransac) return RSX_OK;
    rsx_ransac_default_params(&p);
    if (params) p = *params;
    if (estimator == RSX_ESTIMATOR_MCRANSAC) p.flags |= RSX_RANSAC_MOTION_COMPENSATED;
    else p.flags &= ~RSX_RANSAC_MOTION_COMPENSATED;
    RSX_TRY(rsx::ransac_check_params(p));
    if (h->ransac) return RSX_OK;  // (the estimator's handle: made once, kept whatever becomes of this call)
    rsx_ransac *r = nullptr;
    RSX_TRY(rsx_ransac_create(h->device, &r));
    h->ransac.reset(r);
    return RSX_OK;
  });
} RSX_CATCH_ALL

int rsx_odometry_set_compensation(rsx_odometry *h, const rsx_mocomp_params *params) try {
  return set_config(h, "model", &rsx_odometry::comp_prm, [&](OdoConfig &c, rsx_mocomp_params &p) -> int {
    c.comp = params != nullptr;
    if (!params) return RSX_OK;
    p = *params;
    p.rows = h->rows;
    return rsx::mocomp::check_params(p);
  });
} RSX_CATCH_ALL

int rsx_odometry_set_cfear(rsx_odometry *h, const rsx_cfear_params *params) try {
  return set_config(h, "estimator", &rsx_odometry::cfear_prm, [&](OdoConfig &c, rsx_cfear_params &p) -> int {
    c.estimator = params ? RSX_ESTIMATOR_CFEAR : RSX_ESTIMATOR_ORORA;
    if (!params) c.track = false;
    if (c.pc == Pc::estimate) c.pc = Pc::off;  // (as rsx_odometry_set_estimator)
    if (!params) return RSX_OK;
    p = *params;
    return rsx::cfear::check_params(p);
  });
} RSX_CATCH_ALL

int rsx_odometry_set_cfear_tracking(rsx_odometry *h, const rsx_cfear_track_params *params) try {
  return set_config(h, "estimator", &rsx_odometry::track_prm, [&](OdoConfig &c, rsx_cfear_track_params &p) -> int {
    c.track = params != nullptr;
    if (!params) return RSX_OK;
    p = *params;
    RSX_TRY(rsx::cfear::check_track_params(p));
    if (p.compensate && h->rows > 65536) return fail(RSX_ERR_BAD_ARG, "compensate = 1 takes images of at most 65536 rows");
    return RSX_OK;
  });
} RSX_CATCH_ALL

int rsx_odometry_default_phasecorr_params(rsx_odometry_phasecorr_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  std::memset(p, 0, sizeof(*p));
  rsx_phasecorr_default_params(&p->pc);
  p->mode = RSX_ODOMETRY_PHASECORR_ESTIMATE;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_odometry_set_phasecorr(rsx_odometry *h, const rsx_odometry_phasecorr_params *params) try {
  return set_config(h, "estimator", &rsx_odometry::pc_prm, [&](OdoConfig &c, rsx_odometry_phasecorr_params &p) -> int {
    c.pc = Pc::off;  // (NULL: back to the state before, the selected estimator alone)
    if (!params) return RSX_OK;
    p = *params;
    if (p.mode != RSX_ODOMETRY_PHASECORR_ESTIMATE && p.mode != RSX_ODOMETRY_PHASECORR_FALLBACK) return fail(RSX_ERR_BAD_ARG, "unknown mode %d", p.mode);
    c.pc = p.mode == RSX_ODOMETRY_PHASECORR_ESTIMATE ? Pc::estimate : Pc::fallback;
    if (!(p.max_peak_ratio >= 0.0) || !std::isfinite(p.max_peak_ratio) || !(p.min_peak >= 0.0) || !std::isfinite(p.min_peak))
      return fail(RSX_ERR_BAD_ARG, "max_peak_ratio and min_peak must not be negative");
    p.pc.range_resolution = (double)h->prm.radar_resolution;
    RSX_TRY(rsx::phasecorr::check_params(p.pc, h->rows, h->cols));
    RSX_TRY(check_config(c));  // (before the tables: a refused call makes none)
    if (std::memcmp(&h->pc_tables_of, &p.pc, sizeof(p.pc)) == 0) return RSX_OK;  // (nothing is in flight: every push is synchronous)
    RSX_HIP(hipSetDevice(h->device));
    h->pc_tables_of = rsx_phasecorr_params{};
    RSX_TRY(rsx::phasecorr::make_tables(p.pc, h->rows, h->cols, h->pc_tables, h->match_stream));
    h->pc_tables_of = p.pc;
    return RSX_OK;
  });
} RSX_CATCH_ALL

int rsx_odometry_push_device(rsx_odometry *h, const uint8_t *d_imgs, int32_t n_scans, int64_t image_stride_bytes, int32_t row_stride,
                             const float *azimuths, int32_t azimuths_per_image, rsx_odometry_scan *out, float *out_xy, int32_t max_xy) try {
  RSX_TRY(check_push(h, d_imgs, n_scans, image_stride_bytes, row_stride, azimuths, azimuths_per_image, out, max_xy));
  if (n_scans == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  const OdoNeeds need = needs_of(h);
  const SlotArrays slots = slot_arrays(h, need);
  RSX_TRY(reserve_all(h, need, slots, 0, h->match_stream));
  return push_windows(h, need, n_scans, out, out_xy, max_xy, [&](int, uint64_t g, int b0, int n) {
    return enqueue_extract(h, need, slots, g, d_imgs + (int64_t)b0 * image_stride_bytes, n, image_stride_bytes, row_stride,
                           azimuths + (azimuths_per_image ? (size_t)b0 * h->rows : 0), azimuths_per_image);
  });
} RSX_CATCH_ALL

int rsx_odometry_push(rsx_odometry *h, const uint8_t *imgs, int32_t n_scans, int64_t image_stride_bytes, int32_t row_stride,
                      const float *azimuths, int32_t azimuths_per_image, rsx_odometry_scan *out, float *out_xy, int32_t max_xy) try {
  RSX_TRY(check_push(h, imgs, n_scans, image_stride_bytes, row_stride, azimuths, azimuths_per_image, out, max_xy));
  if (n_scans == 0) return RSX_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  const size_t ibytes = (size_t)h->rows * row_stride;
  const OdoNeeds need = needs_of(h);
  const SlotArrays slots = slot_arrays(h, need);
  RSX_TRY(reserve_all(h, need, slots, ibytes, h->match_stream));
  // three image buffers: the upload of window w + 2 (copy stream) runs while the kernels of windows w and w + 1 do
  struct CopyDone {  // the caller's host images must not be in flight when this call returns, error or not
    hipStream_t cs;
    ~CopyDone() { (void)hipStreamSynchronize(cs); }
  } copy_done{h->copy_stream};
  return push_windows(h, need, n_scans, out, out_xy, max_xy, [&](int w, uint64_t g, int b0, int n) -> int {  // E(g) behind its upload
    // (the buffer was read by the extraction of window w - 3: long done.  With phase correlation M(w - 3) read it as well: push_windows
    // stages window w in the iteration of window w - 2, whose predecessor ended with finish_window's wait for M(w - 3), and a call
    // returns with every M behind it.  Keep that order: an upload staged before that wait would overwrite images a pair stage reads)
    uint8_t *d_imgs = h->imgs[w % N_SETS].as<uint8_t>();
    RSX_TRY(rsx::upload_images(d_imgs, imgs + (int64_t)b0 * image_stride_bytes, n, ibytes, image_stride_bytes, h->copy_stream));
    RSX_HIP(hipEventRecord(h->ev_up, h->copy_stream));
    RSX_HIP(hipStreamWaitEvent(h->lane_stream[g & 1], h->ev_up, 0));
    return enqueue_extract(h, need, slots, g, d_imgs, n, (int64_t)ibytes, row_stride, azimuths + (azimuths_per_image ? (size_t)b0 * h->rows : 0), azimuths_per_image);
  });
} RSX_CATCH_ALL

int rsx_host_alloc_pinned(size_t bytes, void **out) try {
  if (!out || bytes == 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  *out = nullptr;
  if (rsx_device_count() <= 0) return fail(RSX_ERR_NO_DEVICE, "no HIP device visible (librsx has no CPU fallback)");
  RSX_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_host_free_pinned(void *p) try {
  if (p) RSX_HIP(hipHostFree(p));
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
