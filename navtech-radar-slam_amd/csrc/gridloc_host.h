// gridloc_host.h -- the host code that the grid-map localisers share (gridmatch.hip, gridsearch.hip, gridrefine.hip, gridtrack.hip): the
// scaffold of the six rsx_gridmap_{match,search,refine}_batch[_device] entries, and the window's rules, the refinement's rules and the
// geometry that the kernels of the window matchers, the refinement and the tracker take.  A stage describes its call as data (LocCall);
// nothing here knows which stage calls it.
#pragma once
#include <cmath>
#include <functional>
#include <mutex>

#include "gridmap.h"
#include "gridmatch_dev.h"
#include "gridrefine_dev.h"
#include "ragged_host.h"

namespace rsx {
namespace gridloc {

constexpr size_t SIDE_STAGE = (size_t)64 << 20;  // a host entry: the bytes of side output staged per sub-batch

// n jobs on the device: job i owns points [off[i], off[i + 1]) of xy (rows `stride` floats apart) and priors[6 i .. 6 i + 5]
struct LocJobs {
  const float *xy;
  const int64_t *off;
  int64_t stride;
  int32_t n;
  const double *priors;
};

// what a stage says about a ragged localisation call
struct LocCall {
  std::function<int(const rsx_gridmap *)> ready;  // what only the handle can judge (the caller holds h->mu)
  size_t side_words;                              // uint32 words of side output per job (a score volume, the bounds; 0: none)
  DevBuf rsx_gridmap::*side;                      // the handle's buffer for them (null: none)
  size_t result_bytes;                            // of one record
  // launches the jobs: records to d_results, side output to d_side (the caller holds h->mu and has entered s)
  std::function<int(rsx_gridmap *, const LocJobs &, void *d_results, uint32_t *d_side, hipStream_t s)> launch;
};

// The argument rules, judged before the handle is looked at (they need no device); a host entry's stride is 2.  An entry calls
// them itself: the rules of its own params come between them and the rules of the offsets
inline int check_args(const void *xy, const void *offsets, const void *priors, const void *results, int32_t n_jobs, int32_t point_stride) {
  if (!xy || !offsets || !priors || !results || n_jobs < 0) return fail(RSX_ERR_BAD_ARG, "bad arg");
  if (point_stride < 2) return fail(RSX_ERR_BAD_ARG, "point_stride %d below 2", point_stride);
  return RSX_OK;
}

// the device entry behind its argument rules: asynchronous on `stream` (null: the handle's own); side output that the caller gave
// no room for goes to the handle's buffer
inline int run_device(rsx_gridmap *h, const LocCall &c, const LocJobs &j, void *d_results, uint32_t *d_side, void *stream) {
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_TRY(c.ready(h));
  if (j.n == 0) return RSX_OK;
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
  RSX_TRY(h->order.enter(s));
  if (!d_side && c.side) {
    RSX_TRY((h->*c.side).reserve((size_t)j.n * c.side_words * sizeof(uint32_t), s, false));
    d_side = (h->*c.side).as<uint32_t>();
  }
  return c.launch(h, j, d_results, d_side, s);
}

// the host entry behind its argument rules (`what` names it): up through the handle's one staging set, the launches, down, and a
// synchronise, so that the set is free again when it returns
inline int run_host(rsx_gridmap *h, const LocCall &c, const char *what, const float *xy, const int64_t *offsets, int32_t n_jobs, const double *priors,
                    void *out_results, uint32_t *out_side) {
  if (n_jobs > 0) {
    RSX_TRY(check_offsets(offsets, n_jobs, what));
    for (int32_t i = 0; i < n_jobs; i++)
      if (offsets[i + 1] - offsets[i] > RSX_GRIDMAP_MATCH_MAX_POINTS)
        return fail(RSX_ERR_BAD_ARG, "job %d has %lld points, more than %d", i, (long long)(offsets[i + 1] - offsets[i]), RSX_GRIDMAP_MATCH_MAX_POINTS);
  }
  if (!h) return fail(RSX_ERR_BAD_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  RSX_TRY(c.ready(h));  // (before the success of a call with no jobs: a handle that is not ready refuses that one too)
  if (n_jobs == 0) return RSX_OK;
  RSX_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  RSX_TRY(h->order.enter(s));
  const size_t n = (size_t)n_jobs, side_bytes = c.side_words * sizeof(uint32_t);
  RSX_TRY(stage_up(h->m_xy, xy, (size_t)offsets[n_jobs] * 8, s));
  RSX_TRY(stage_up(h->m_off, offsets, (n + 1) * 8, s));
  RSX_TRY(stage_up(h->m_tf, priors, n * 48, s));
  RSX_TRY(stage_room(h->m_res, n * c.result_bytes, s));
  // sub-batches bound the staged side output; a job's bytes do not depend on the cut.  A call without any is one cut
  const size_t per = side_bytes ? SIDE_STAGE / side_bytes : n, sub = per < n ? per : n;
  if (c.side) RSX_TRY(stage_room(h->*c.side, sub * side_bytes, s));
  for (size_t b0 = 0; b0 < n; b0 += sub) {
    const size_t nb = n - b0 < sub ? n - b0 : sub;
    RSX_TRY(c.launch(h, {h->m_xy.as<float>(), h->m_off.as<int64_t>() + b0, 2, (int32_t)nb, h->m_tf.as<double>() + 6 * b0},
                     h->m_res.as<char>() + b0 * c.result_bytes, c.side ? (h->*c.side).as<uint32_t>() : nullptr, s));
    if (out_side) RSX_TRY(stage_down(out_side + b0 * c.side_words, h->*c.side, nb * side_bytes, s));
  }
  RSX_TRY(stage_down(out_results, h->m_res, n * c.result_bytes, s));
  RSX_HIP(hipStreamSynchronize(s));
  return RSX_OK;
}

// the readiness that asks for the likelihood plane and nothing else
inline int have_likelihood(const rsx_gridmap *h) { return h->have_like ? RSX_OK : no_likelihood(); }

// the window of a params struct (angle_steps, angle_step, x_cells, y_cells) against the caps of its stage
template <typename P>
int check_window_params(const P &p, int max_k, int max_uv) {
  if (p.angle_steps < 0 || p.angle_steps > max_k) return fail(RSX_ERR_BAD_ARG, "angle_steps %d outside 0 .. %d", p.angle_steps, max_k);
  if (p.angle_steps > 0 && (!(p.angle_step > 0.0) || !std::isfinite(p.angle_step)))
    return fail(RSX_ERR_BAD_ARG, "angle_step must be positive and finite when angle_steps > 0");
  if (p.x_cells < 0 || p.x_cells > max_uv) return fail(RSX_ERR_BAD_ARG, "x_cells %d outside 0 .. %d", p.x_cells, max_uv);
  if (p.y_cells < 0 || p.y_cells > max_uv) return fail(RSX_ERR_BAD_ARG, "y_cells %d outside 0 .. %d", p.y_cells, max_uv);
  return RSX_OK;
}

// the map of the handle, the window K, U, V and the pitch of the framed plane that the kernels read
inline gridmatch_dev::MatchGeo match_geo(const rsx_gridmap *h, int K, int U, int V, unsigned pitch) {
  gridmatch_dev::MatchGeo g{};
  g.ox = h->p.origin_x, g.oy = h->p.origin_y, g.res = h->p.resolution, g.inv_res = 1.0 / h->p.resolution;
  g.W = h->p.width, g.H = h->p.height, g.K = K, g.U = U, g.V = V;
  g.pitch = pitch;
  return g;
}

// the rules of rsx_gridmap_refine_params
inline int check_refine_params(const rsx_gridmap_refine_params &p) {
  if (!(p.damping > 0.0) || !std::isfinite(p.damping)) return fail(RSX_ERR_BAD_ARG, "damping must be positive and finite");
  if (!(p.max_shift_step > 0.0 && p.max_shift_step <= 8.0)) return fail(RSX_ERR_BAD_ARG, "max_shift_step outside (0, 8]");
  if (!(p.max_rotation_step > 0.0 && p.max_rotation_step <= rsx::mocomp::TH_MAX)) return fail(RSX_ERR_BAD_ARG, "max_rotation_step outside (0, 0.5]");
  if (!(p.shift_tolerance >= 0.0) || !std::isfinite(p.shift_tolerance)) return fail(RSX_ERR_BAD_ARG, "shift_tolerance must be finite and not negative");
  if (!(p.rotation_tolerance >= 0.0) || !std::isfinite(p.rotation_tolerance))
    return fail(RSX_ERR_BAD_ARG, "rotation_tolerance must be finite and not negative");
  if (p.max_evaluations < 1 || p.max_evaluations > 64) return fail(RSX_ERR_BAD_ARG, "max_evaluations %d outside 1 .. 64", p.max_evaluations);
  if (p.reserved != 0) return fail(RSX_ERR_BAD_ARG, "reserved must be 0");
  return RSX_OK;
}

// the map of the handle as the refinement's evaluation reads it
inline gridrefine_dev::RefineGeo refine_geo(const rsx_gridmap *h) {
  gridrefine_dev::RefineGeo g{};
  g.ox = h->p.origin_x, g.oy = h->p.origin_y, g.res = h->p.resolution, g.inv_res = 1.0 / h->p.resolution;
  g.w = (double)h->p.width, g.h = (double)h->p.height;
  g.x_hi = (double)(h->p.width + gridmatch_dev::PLACE), g.y_hi = (double)(h->p.height + gridmatch_dev::PLACE);
  g.pitch = h->like_pitch();
  return g;
}

}  // namespace gridloc
}  // namespace rsx
