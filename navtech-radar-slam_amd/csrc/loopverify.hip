// loopverify.hip -- the keyframe-cloud store of the pose-graph node and what the reference does with it: loop
// verification behind a ScanContext candidate (submap assembly -> VoxelGrid -> ICP -> gate) and the map cloud.
//
// Reference (pgo/SC-A-LOAM/src/laserPosegraphOptimization.cpp = PGO.cpp):
//   keyframeLaserClouds.push_back(thisKeyFrameDS)        PGO.cpp:482-487  the 0.4 m VoxelGrid output of every keyframe
//   local2global                                         PGO.cpp:199-220  p -> pcl::getTransformation(pose) * p, float
//   loopFindNearKeyframesCloud(cloud, key, size, root)   PGO.cpp:329-352  keyframes key - size .. key + size, each in ITS
//                                                        OWN local frame, all moved by the pose of keyframe `root`,
//                                                        concatenated, VoxelGrid 0.4 m
//   doICPVirtualRelative(loop, curr)                     PGO.cpp:355-406  source = submap(curr, 0, root = loop), target =
//                                                        submap(loop, 25, root = loop); ICP 150 m / 100 / 1e-6 / 1e-6;
//                                                        accepted iff converged && fitness <= 0.3; Euler angles;
//                                                        poseFrom.between(identity)
//   pubMap                                               PGO.cpp:631-655  every SKIP_FRAMES-th keyframe by its own pose,
//                                                        concatenated, VoxelGrid
//
// MI355X mapping: the keyframe clouds live back to back in ONE HBM array of float4 {x, y, z, intensity} (append-only, like
// the reference's vector), so the +-25-keyframe submap of a loop candidate is one contiguous slice.  A verification is TWO
// launches and one read-back (round 5): vg_coop_kernel transforms both slices by the root pose as it reads them and
// VoxelGrid-filters them (voxelgrid.hip; the sizes stay in device memory), icp_persistent_kernel aligns them (icp.hip).
// A radar keyframe is ~10^3 points, a submap <= 51 of them: the chain is latency-bound (grid barriers, coherent loads) and
// the nearest-neighbour scan VALU-bound; no HBM roofline applies.  Rounds 1-4: ~180 launches and 26 host synchronisations.
//
// Parity: the transform is bit-exact float (mul / add in the reference's order, no contraction), the VoxelGrid is
// bit-identical to oracle/voxelgrid_ref.c, the ICP within 1e-4 of oracle/icp_ref.c -- the chain is checked against
// oracle/loopverify_ref.c (tests/test_gpu_loopverify.py).  PCL / GTSAM are absent from the reference checkout: their
// pieces (getTransformation, getTranslationAndEulerAngles, VoxelGrid, ICP, Pose3::between) follow the published sources:
// parity unpinned; the control flow is the reference's own.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "icp.h"
#include "loopverify.h"
#include "rsx_common.h"
#include "voxelgrid.h"

namespace {

using rsx::vg::Mat34;  // row-major 3 x 4

// pcl::getTransformation(float x, float y, float z, float roll, float pitch, float yaw): the Affine3f overload the
// reference reaches from local2global (PGO.cpp:206; its Pose6D doubles are narrowed at the call), computed on the host
// in float like PCL does
Mat34 pose_matrix(const double *pose6) {
  const float x = (float)pose6[0], y = (float)pose6[1], z = (float)pose6[2];
  const float roll = (float)pose6[3], pitch = (float)pose6[4], yaw = (float)pose6[5];
  const float A = std::cos(yaw), B = std::sin(yaw), C = std::cos(pitch), D = std::sin(pitch), E = std::cos(roll), F = std::sin(roll);
  const float DE = D * E, DF = D * F;
  Mat34 t;
  t.m[0] = A * C;  t.m[1] = A * DF - B * E;  t.m[2] = B * F + A * DE;  t.m[3] = x;
  t.m[4] = B * C;  t.m[5] = A * E + B * DF;  t.m[6] = B * DE - A * F;  t.m[7] = y;
  t.m[8] = -D;     t.m[9] = C * F;           t.m[10] = C * E;          t.m[11] = z;
  return t;
}

// host points (float x, y, z at byte offsets 0, 4, 8 of each stride, intensity at ioff or none) -> packed float4
__global__ __launch_bounds__(256) void lv_pack(const char *__restrict__ pts, int64_t n, int64_t stride, int ioff, float4 *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *p = reinterpret_cast<const float *>(pts + i * stride);
  out[i] = float4{p[0], p[1], p[2], ioff >= 0 ? *reinterpret_cast<const float *>(pts + i * stride + ioff) : 0.0f};
}

// pubMap (PGO.cpp:640-645): every point of a KEPT keyframe through the pose of its keyframe, kept keyframes back to back in
// keyframe order (what `*laserCloudMapPGO += *local2global(...)` builds).  kf_of[i] = keyframe of point i
struct KfMap {
  Mat34 T;
  long long src_first;  // first point of the keyframe in the store
  long long dst_first;  // ... in the concatenated map cloud; < 0: the keyframe is skipped
};
__global__ __launch_bounds__(256) void lv_transform_each(const float4 *__restrict__ in, const int32_t *__restrict__ kf_of, int64_t n,
                                                         const KfMap *__restrict__ km, float4 *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const KfMap k = km[kf_of[i]];
  if (k.dst_first < 0) return;
  const float4 p = in[i];
  const Mat34 &T = k.T;
  float4 o;
  o.x = T.m[0] * p.x + T.m[1] * p.y + T.m[2] * p.z + T.m[3];
  o.y = T.m[4] * p.x + T.m[5] * p.y + T.m[6] * p.z + T.m[7];
  o.z = T.m[8] * p.x + T.m[9] * p.y + T.m[10] * p.z + T.m[11];
  o.w = p.w;
  out[k.dst_first + (i - k.src_first)] = o;
}

__global__ __launch_bounds__(256) void lv_fill_kf(int32_t *__restrict__ kf_of, int64_t first, int64_t n, int32_t kf) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) kf_of[first + i] = kf;
}

}  // namespace

struct rsx_kfstore {
  int device = 0;
  std::mutex mu;
  rsx::Stream stream;
  rsx::DevBuf clouds;        // float4 per point, keyframes back to back
  rsx::DevBuf kf_of;         // int32 per point: its keyframe
  std::vector<int64_t> off;  // keyframe i = points [off[i], off[i + 1])
  rsx::DevBuf stage, work_s, work_t, tf;
  rsx::Owned<rsx_voxelgrid, rsx_voxelgrid_destroy> vg_s, vg_t;
  rsx::Owned<rsx_icp, rsx_icp_destroy> icp;
};

using rsx::fail;

namespace {

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

// append n packed float4 points that are in device memory (on the store's stream)
int append_device(rsx_kfstore *h, const float4 *d_pts, int64_t n, int32_t *out_index) {
  hipStream_t s = h->stream;
  const int64_t first = h->off.back(), kf = (int64_t)h->off.size() - 1;
  if (kf >= 0x7fffffff) return fail(RSX_ERR_RANGE, "too many keyframes");
  RSX_TRY(h->clouds.reserve((size_t)(first + n + 1) * 16, s, true));
  RSX_TRY(h->kf_of.reserve((size_t)(first + n + 1) * 4, s, true));
  if (n > 0) {
    RSX_HIP(hipMemcpyAsync(h->clouds.as<float4>() + first, d_pts, (size_t)n * 16, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(lv_fill_kf, dim3(blocks_of(n)), dim3(256), 0, s, h->kf_of.as<int32_t>(), first, n, (int32_t)kf);
    RSX_HIP(hipGetLastError());
  }
  h->off.push_back(first + n);
  if (out_index) *out_index = (int32_t)kf;
  return RSX_OK;
}

// the slice of the store loopFindNearKeyframesCloud (PGO.cpp:329-352) concatenates: keyframes key - size .. key + size
void submap_slice(const rsx_kfstore *h, int64_t key, int64_t size, int64_t *first, int64_t *n) {
  const int64_t nkf = (int64_t)h->off.size() - 1;
  int64_t lo = key - size, hi = key + size;
  if (lo < 0) lo = 0;
  if (hi > nkf - 1) hi = nkf - 1;
  *first = 0;
  *n = 0;
  if (lo > hi) return;
  *first = h->off[lo];
  *n = h->off[hi + 1] - *first;
}

// loopFindNearKeyframesCloud on the device: transform (local2global by the root pose) and VoxelGrid in ONE launch
// -> *d_out (owned by vg, valid until its next call), *n_out
int submap_device(rsx_kfstore *h, rsx_voxelgrid *vg, int64_t key, int64_t size, const Mat34 &T, float leaf, const float **d_out,
                  int64_t *n_out) {
  *d_out = nullptr;
  *n_out = 0;
  int64_t first = 0, n = 0;
  submap_slice(h, key, size, &first, &n);
  if (n <= 0) return RSX_OK;  // nearKeyframes->empty()
  hipStream_t s = h->stream;
  std::lock_guard<std::mutex> lk(rsx::vg::mutex_of(vg));
  rsx::vg::JobIn in{vg, h->clouds.as<float4>() + first, n, 16, 12, &T, leaf, n};
  rsx::vg::DeviceCloud dc;
  RSX_TRY(rsx::vg::enqueue(&in, 1, s, &dc));
  long long cnt = 0;
  RSX_HIP(hipMemcpyAsync(&cnt, dc.d_count, sizeof(cnt), hipMemcpyDeviceToHost, s));
  RSX_HIP(hipStreamSynchronize(s));
  if (cnt < 0) return fail(RSX_ERR_HIP, "a grid barrier of the cooperative VoxelGrid kernel gave up after 5 s: its workgroups were not all resident");
  *d_out = dc.d_out;
  *n_out = cnt;
  return RSX_OK;
}

// the VoxelGrid launch of a verification (doICPVirtualRelative, PGO.cpp:361-362): source = keyframe curr alone, target =
// loop +- history_keyframe_search_num, both moved by the ONE root pose T and filtered by ONE cooperative kernel on stream s,
// into the store's two VoxelGrid handles; an empty slice (nearKeyframes->empty()) is no job.  The caller holds the mutexes of
// both handles.  -> per cloud (0 source, 1 target): the slice's size, and the output and its count in device memory (null
// for an empty slice).  rsx_loop_verify and the diagnostic rsx_loop_verify_clouds both launch through here.
struct PairClouds {
  int64_t np[2];
  const float *d_cloud[2];
  const long long *d_cnt[2];
};
int enqueue_pair(rsx_kfstore *h, int32_t loop_idx, int32_t curr_idx, const Mat34 &T, const rsx_loop_verify_params &p, hipStream_t s,
                 PairClouds *out) {
  int64_t first[2];
  submap_slice(h, curr_idx, 0, &first[0], &out->np[0]);
  submap_slice(h, loop_idx, p.history_keyframe_search_num, &first[1], &out->np[1]);
  rsx_voxelgrid *vgs[2] = {h->vg_s.get(), h->vg_t.get()};
  rsx::vg::JobIn jobs[2];
  rsx::vg::DeviceCloud dc[2];
  int which[2], nj = 0;
  for (int c = 0; c < 2; c++) {
    out->d_cloud[c] = nullptr;
    out->d_cnt[c] = nullptr;
    if (out->np[c] > 0) {
      jobs[nj] = rsx::vg::JobIn{vgs[c], h->clouds.as<float4>() + first[c], out->np[c], 16, 12, &T, p.leaf, out->np[c]};
      which[nj++] = c;
    }
  }
  if (nj) RSX_TRY(rsx::vg::enqueue(jobs, nj, s, dc));
  for (int j = 0; j < nj; j++) {
    out->d_cloud[which[j]] = dc[j].d_out;
    out->d_cnt[which[j]] = dc[j].d_count;
  }
  return RSX_OK;
}

// arguments of a verification -> the parameters in force, the keyframe indices checked (the caller holds the store's mutex)
int verify_args(rsx_kfstore *h, int32_t loop_idx, int32_t curr_idx, const rsx_loop_verify_params *params, rsx_loop_verify_params *p) {
  rsx_loop_verify_default_params(p);
  if (params) *p = *params;
  if (p->history_keyframe_search_num < 0 || !(p->leaf > 0.0f)) return fail(RSX_ERR_BAD_ARG, "bad loop-verification params");
  const int64_t nkf = (int64_t)h->off.size() - 1;
  if (loop_idx < 0 || loop_idx >= nkf || curr_idx < 0 || curr_idx >= nkf) return fail(RSX_ERR_RANGE, "keyframe index out of range (%lld stored)", (long long)nkf);
  return RSX_OK;
}

}  // namespace

namespace rsx {
namespace kf {

std::mutex &mutex_of(rsx_kfstore *h) { return h->mu; }
int device_of(rsx_kfstore *h) { return h->device; }
int append_device_locked(rsx_kfstore *h, const void *d_xyzi, int64_t n, int32_t *out_index) {
  try {
    h->off.reserve(h->off.size() + 1);
  } catch (...) {
    return fail(RSX_ERR_OOM, "host alloc");
  }
  RSX_HIP(hipSetDevice(h->device));
  RSX_TRY(append_device(h, static_cast<const float4 *>(d_xyzi), n, out_index));
  RSX_HIP(hipStreamSynchronize(h->stream));
  return RSX_OK;
}
int keyframe_device_locked(rsx_kfstore *h, int32_t index, const float **d_xyzi, int64_t *n) {
  if (index < 0 || index >= (int64_t)h->off.size() - 1) return fail(RSX_ERR_BAD_ARG, "keyframe %d out of range (%lld stored)", index, (long long)h->off.size() - 1);
  *d_xyzi = reinterpret_cast<const float *>(h->clouds.as<float4>() + h->off[index]);
  *n = h->off[index + 1] - h->off[index];
  return RSX_OK;
}

}  // namespace kf
}  // namespace rsx

extern "C" {

int rsx_kfstore_create(int device, rsx_kfstore **out) try {
  if (!out) return fail(RSX_ERR_BAD_ARG, "null out");
  *out = nullptr;
  RSX_TRY(rsx::check_device(device));
  std::unique_ptr<rsx_kfstore> h(new (std::nothrow) rsx_kfstore());
  if (!h) return fail(RSX_ERR_OOM, "host alloc");
  h->device = device;
  h->off.push_back(0);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = h->stream.create();
  if (e != hipSuccess) return fail(RSX_ERR_HIP, "create: %s", hipGetErrorString(e));
  rsx_voxelgrid *vg_s = nullptr, *vg_t = nullptr;
  rsx_icp *icp = nullptr;
  RSX_TRY(rsx_voxelgrid_create(device, &vg_s));
  h->vg_s.reset(vg_s);
  RSX_TRY(rsx_voxelgrid_create(device, &vg_t));
  h->vg_t.reset(vg_t);
  RSX_TRY(rsx_icp_create(device, &icp));
  h->icp.reset(icp);
  *out = h.release();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_kfstore_destroy(rsx_kfstore *h) try {
  if (!h) return RSX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_kfstore_add(rsx_kfstore *h, const void *pts, size_t n, size_t stride_bytes, int32_t intensity_offset, int32_t *out_index) try {
  if (!h || (!pts && n)) return fail(RSX_ERR_BAD_ARG, "null arg");
  if (stride_bytes < 12 || (stride_bytes & 3)) return fail(RSX_ERR_BAD_ARG, "stride_bytes must be >= 12 and a multiple of 4");
  if (intensity_offset >= 0 && ((intensity_offset & 3) || (size_t)intensity_offset + 4 > stride_bytes))
    return fail(RSX_ERR_BAD_ARG, "intensity_offset outside the point");
  if (n > 0x7fffffffull) return fail(RSX_ERR_RANGE, "cloud too large");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int64_t first = h->off.back();
  RSX_TRY(h->clouds.reserve((size_t)(first + (int64_t)n + 1) * 16, s, true));
  RSX_TRY(h->kf_of.reserve((size_t)(first + (int64_t)n + 1) * 4, s, true));
  const int64_t kf = (int64_t)h->off.size() - 1;
  if (kf >= 0x7fffffff) return fail(RSX_ERR_RANGE, "too many keyframes");
  h->off.reserve(h->off.size() + 1);
  if (n) {
    RSX_TRY(h->stage.reserve(n * stride_bytes, s, false));
    RSX_HIP(hipMemcpyAsync(h->stage.p, pts, n * stride_bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(lv_pack, dim3(blocks_of((int64_t)n)), dim3(256), 0, s, static_cast<const char *>(h->stage.p), (int64_t)n,
                       (int64_t)stride_bytes, (int)intensity_offset, h->clouds.as<float4>() + first);
    hipLaunchKernelGGL(lv_fill_kf, dim3(blocks_of((int64_t)n)), dim3(256), 0, s, h->kf_of.as<int32_t>(), first, (int64_t)n, (int32_t)kf);
    RSX_HIP(hipGetLastError());
    RSX_HIP(hipStreamSynchronize(s));  // the caller's buffer is free on return (the reference copies by value, PGO.cpp:487)
  }
  h->off.push_back(first + (int64_t)n);
  if (out_index) *out_index = (int32_t)kf;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_kfstore_add_device(rsx_kfstore *h, const void *d_xyzi, size_t n, int32_t *out_index) try {
  if (!h || (!d_xyzi && n)) return fail(RSX_ERR_BAD_ARG, "null arg");
  if (n > 0x7fffffffull) return fail(RSX_ERR_RANGE, "cloud too large");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  h->off.reserve(h->off.size() + 1);
  RSX_TRY(append_device(h, static_cast<const float4 *>(d_xyzi), (int64_t)n, out_index));
  RSX_HIP(hipStreamSynchronize(h->stream));
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_kfstore_size(rsx_kfstore *h, int64_t *n_keyframes, int64_t *n_points) try {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n_keyframes) *n_keyframes = (int64_t)h->off.size() - 1;
  if (n_points) *n_points = h->off.back();
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_kfstore_get(rsx_kfstore *h, int32_t index, float *out_xyzi, int64_t max_out, int64_t *out_count) try {
  if (!h || !out_count || (!out_xyzi && max_out > 0)) return fail(RSX_ERR_BAD_ARG, "null arg");
  std::lock_guard<std::mutex> lk(h->mu);
  if (index < 0 || index >= (int64_t)h->off.size() - 1) return fail(RSX_ERR_RANGE, "keyframe %d out of range", index);
  const int64_t first = h->off[index], n = h->off[index + 1] - first;
  *out_count = n;
  const int64_t w = n < max_out ? n : max_out;
  if (w > 0) {
    RSX_HIP(hipSetDevice(h->device));
    RSX_HIP(hipMemcpyAsync(out_xyzi, h->clouds.as<float4>() + first, (size_t)w * 16, hipMemcpyDeviceToHost, h->stream));
    RSX_HIP(hipStreamSynchronize(h->stream));
  }
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_loop_verify_default_params(rsx_loop_verify_params *p) try {
  if (!p) return fail(RSX_ERR_BAD_ARG, "null params");
  p->history_keyframe_search_num = 25;  // PGO.cpp:358
  p->leaf = 0.4f;                       // PGO.cpp:687-689
  p->fitness_threshold = 0.3;           // PGO.cpp:384
  rsx_icp_default_params(&p->icp);      // PGO.cpp:374-378
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_loop_submap(rsx_kfstore *h, int32_t key, int32_t submap_size, const double *root_pose6, float leaf, float *out_xyzi,
                    int64_t max_out, int64_t *out_count) try {
  if (!h || !root_pose6 || !out_count || (!out_xyzi && max_out > 0)) return fail(RSX_ERR_BAD_ARG, "null arg");
  if (submap_size < 0 || !(leaf > 0.0f)) return fail(RSX_ERR_BAD_ARG, "bad submap size / leaf");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  const float *d = nullptr;
  int64_t n = 0;
  RSX_TRY(submap_device(h, h->vg_t.get(), key, submap_size, pose_matrix(root_pose6), leaf, &d, &n));
  *out_count = n;
  const int64_t w = n < max_out ? n : max_out;
  if (w > 0) {
    RSX_HIP(hipMemcpyAsync(out_xyzi, d, (size_t)w * 16, hipMemcpyDeviceToHost, h->stream));
    RSX_HIP(hipStreamSynchronize(h->stream));
  }
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_loop_verify(rsx_kfstore *h, int32_t loop_idx, int32_t curr_idx, const double *root_pose6, const rsx_loop_verify_params *params,
                    rsx_loop_verify_result *out) try {
  if (!h || !root_pose6 || !out) return fail(RSX_ERR_BAD_ARG, "null arg");
  rsx_loop_verify_params p;
  std::memset(out, 0, sizeof(*out));
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_TRY(verify_args(h, loop_idx, curr_idx, params, &p));
  RSX_HIP(hipSetDevice(h->device));
  const Mat34 T = pose_matrix(root_pose6);  // the ONE root pose both clouds are moved by (PGO.cpp:340,361-362)
  // two launches and one read-back: (1) both submaps -- source = keyframe curr alone (PGO.cpp:361), target = loop +- 25
  // (PGO.cpp:362) -- transformed by the root pose and VoxelGrid-filtered by ONE cooperative kernel, their sizes left in device
  // memory; (2) the persistent ICP kernel, which reads the sizes there.  All on the ICP handle's stream.
  rsx_icp_result ir;
  int64_t ns = 0, nt = 0;
  {
    std::lock_guard<std::mutex> lks(rsx::vg::mutex_of(h->vg_s.get()));
    std::lock_guard<std::mutex> lkt(rsx::vg::mutex_of(h->vg_t.get()));
    std::lock_guard<std::mutex> lki(rsx::icp::mutex_of(h->icp.get()));
    PairClouds pc;
    RSX_TRY(enqueue_pair(h, loop_idx, curr_idx, T, p, rsx::icp::stream_of(h->icp.get()), &pc));
    RSX_TRY(rsx::icp::align_device_counts_locked(h->icp.get(), pc.d_cloud[0], pc.np[0], pc.d_cnt[0], 16, pc.d_cloud[1], pc.np[1], pc.d_cnt[1], 16,
                                                 &p.icp, nullptr, &ir, &ns, &nt));
  }
  out->n_source = ns;
  out->n_target = nt;
  out->converged = ir.converged;
  out->iterations = ir.iterations;
  out->state = ir.state;
  out->fitness = ir.fitness;
  std::memcpy(out->transform, ir.transform, sizeof(out->transform));
  out->accepted = !(ir.converged == 0 || ir.fitness > p.fitness_threshold);  // PGO.cpp:385
  // pcl::getTranslationAndEulerAngles (PGO.cpp:400-403), float
  const float *t = ir.transform;
  out->x = t[3];
  out->y = t[7];
  out->z = t[11];
  out->roll = std::atan2(t[9], t[10]);
  out->pitch = std::asin(-t[8]);
  out->yaw = std::atan2(t[4], t[0]);
  // poseFrom = Pose3(Rot3::RzRyRx(roll, pitch, yaw), Point3(x, y, z)); poseFrom.between(identity) = poseFrom^-1 (PGO.cpp:404-407)
  const double cx = std::cos((double)out->roll), sx = std::sin((double)out->roll), cy = std::cos((double)out->pitch),
               sy = std::sin((double)out->pitch), cz = std::cos((double)out->yaw), sz = std::sin((double)out->yaw);
  const double R[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx,
                       -sy,     cy * sx,                cy * cx};
  const double tr[3] = {(double)out->x, (double)out->y, (double)out->z};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) out->relative[4 * i + j] = R[3 * j + i];
    out->relative[4 * i + 3] = -(R[0 * 3 + i] * tr[0] + R[1 * 3 + i] * tr[1] + R[2 * 3 + i] * tr[2]);
  }
  out->relative[12] = out->relative[13] = out->relative[14] = 0.0;
  out->relative[15] = 1.0;
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_loop_verify_clouds(rsx_kfstore *h, int32_t loop_idx, int32_t curr_idx, const double *root_pose6, const rsx_loop_verify_params *params,
                           float *out_src, int64_t max_src, int64_t *n_src, float *out_tgt, int64_t max_tgt, int64_t *n_tgt) try {
  if (!h || !root_pose6 || !n_src || !n_tgt || (!out_src && max_src > 0) || (!out_tgt && max_tgt > 0)) return fail(RSX_ERR_BAD_ARG, "null arg");
  *n_src = *n_tgt = 0;
  rsx_loop_verify_params p;
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_TRY(verify_args(h, loop_idx, curr_idx, params, &p));
  RSX_HIP(hipSetDevice(h->device));
  const Mat34 T = pose_matrix(root_pose6);
  // the launch of rsx_loop_verify, on the stream it uses, then the two clouds instead of the ICP
  std::lock_guard<std::mutex> lks(rsx::vg::mutex_of(h->vg_s.get()));
  std::lock_guard<std::mutex> lkt(rsx::vg::mutex_of(h->vg_t.get()));
  std::lock_guard<std::mutex> lki(rsx::icp::mutex_of(h->icp.get()));
  hipStream_t s = rsx::icp::stream_of(h->icp.get());
  PairClouds pc;
  RSX_TRY(enqueue_pair(h, loop_idx, curr_idx, T, p, s, &pc));
  long long cnt[2] = {0, 0};
  for (int c = 0; c < 2; c++)
    if (pc.d_cnt[c]) RSX_HIP(hipMemcpyAsync(&cnt[c], pc.d_cnt[c], sizeof(cnt[c]), hipMemcpyDeviceToHost, s));
  RSX_HIP(hipStreamSynchronize(s));
  if (cnt[0] < 0 || cnt[1] < 0) return fail(RSX_ERR_HIP, "a grid barrier of the cooperative VoxelGrid kernel gave up after 5 s: its workgroups were not all resident");
  float *outs[2] = {out_src, out_tgt};
  const int64_t maxs[2] = {max_src, max_tgt};
  for (int c = 0; c < 2; c++) {
    const int64_t w = cnt[c] < maxs[c] ? cnt[c] : maxs[c];
    if (w > 0) RSX_HIP(hipMemcpyAsync(outs[c], pc.d_cloud[c], (size_t)w * 16, hipMemcpyDeviceToHost, s));
  }
  RSX_HIP(hipStreamSynchronize(s));
  *n_src = cnt[0];
  *n_tgt = cnt[1];
  return RSX_OK;
} RSX_CATCH_ALL

int rsx_kfstore_build_map(rsx_kfstore *h, const double *poses6, int64_t n_poses, int32_t skip_frames, float leaf, float *out_xyzi,
                          int64_t max_out, int64_t *out_count) try {
  if (!h || !out_count || (!poses6 && n_poses > 0) || (!out_xyzi && max_out > 0)) return fail(RSX_ERR_BAD_ARG, "null arg");
  if (skip_frames < 1 || !(leaf > 0.0f)) return fail(RSX_ERR_BAD_ARG, "skip_frames must be >= 1 and leaf positive");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_HIP(hipSetDevice(h->device));
  *out_count = 0;
  int64_t nkf = (int64_t)h->off.size() - 1;
  if (n_poses < nkf) nkf = n_poses;  // keyframePosesUpdated.size() bounds the loop (PGO.cpp:640)
  if (nkf <= 0) return RSX_OK;
  const int64_t n = h->off[nkf];
  if (n <= 0) return RSX_OK;
  hipStream_t s = h->stream;
  std::vector<KfMap> km((size_t)nkf);
  int64_t total = 0;
  for (int64_t k = 0; k < nkf; k++) {
    KfMap &e = km[(size_t)k];
    e.src_first = h->off[k];
    if (k % skip_frames == 0) {  // counter % SKIP_FRAMES == 0 (PGO.cpp:641)
      e.T = pose_matrix(poses6 + 6 * k);
      e.dst_first = total;
      total += h->off[k + 1] - h->off[k];
    } else {
      std::memset(&e.T, 0, sizeof(e.T));
      e.dst_first = -1;
    }
  }
  if (total <= 0) return RSX_OK;
  RSX_TRY(h->tf.reserve((size_t)nkf * sizeof(KfMap), s, false));
  RSX_TRY(h->work_t.reserve((size_t)total * 16, s, false));
  RSX_HIP(hipMemcpyAsync(h->tf.p, km.data(), (size_t)nkf * sizeof(KfMap), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(lv_transform_each, dim3(blocks_of(n)), dim3(256), 0, s, h->clouds.as<float4>(), h->kf_of.as<int32_t>(), n,
                     h->tf.as<KfMap>(), h->work_t.as<float4>());
  RSX_HIP(hipGetLastError());
  const float *d = nullptr;
  int64_t m = 0;
  {
    std::lock_guard<std::mutex> lkv(rsx::vg::mutex_of(h->vg_t.get()));
    RSX_TRY(rsx::vg::filter_device(h->vg_t.get(), h->work_t.p, total, 16, 12, leaf, total, &d, &m, s));  // (syncs s: km is free to go)
    *out_count = m;
    const int64_t w = m < max_out ? m : max_out;
    if (w > 0) {
      RSX_HIP(hipMemcpyAsync(out_xyzi, d, (size_t)w * 16, hipMemcpyDeviceToHost, s));
      RSX_HIP(hipStreamSynchronize(s));
    }
  }
  return RSX_OK;
} RSX_CATCH_ALL

}  // extern "C"
