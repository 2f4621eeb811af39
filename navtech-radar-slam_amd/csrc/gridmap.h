// gridmap.h -- the handle of the radar grid map, shared by gridmap.hip (the planes: accumulate, read, render) and gridmatch.hip (the
// likelihood plane and the correlative matching that reads it), gridsearch.hip (the wide-window search over a snapshot of it) and
// gridrefine.hip (the sub-cell refinement that interpolates the likelihood plane) and gridfield.hip (the distance transform that turns
// the likelihood plane into a likelihood field) and gridtrack.hip (the tracker, whose handle borrows this one's plane, mutex, stream and
// stream order); and the rules that more than one of them judges
// (the render mode, a window of the map, the missing likelihood plane).  What the three localisers share beyond the handle is in
// gridloc_host.h (the scaffold of their entries) and gridmatch_dev.h (their device code).
#pragma once
#include <cstdint>
#include <mutex>
#include <vector>

#include "rsx_common.h"

namespace rsx {

struct GridmapGeometry {
  double res, ox, oy, rr;
  double e_hi;    // (cols rr)^2: d2 at or above it lies in bin `cols` or beyond
  double max2;    // max_range^2 (+inf: none)
  double reach2;  // tile test: no cell farther than this (squared, with margin) is observed
  double hole2;   // tile test: no cell nearer than this (squared, with margin) is observed
  float inv_rr, rows_per_rad;
  int W, H, rows, cols, lo_bin, hw, thr;
};

// the likelihood plane sits in a zeroed frame of this many cells on every side, so that a shifted cell of a placed point (64 cells
// outside the map at the most, shifted by 32 at the most, read four bytes at a time) is always a byte of the buffer: a cell outside
// the map reads 0 and the matching kernel tests no bound
constexpr int GRIDMAP_LIKE_MARGIN = 128;

}  // namespace rsx

struct rsx_gridmap {
  int device = 0, rows = 0, cols = 0;
  rsx_gridmap_params p{};
  rsx::GridmapGeometry g{};
  std::mutex mu;
  rsx::Stream stream;
  rsx::DevBuf planes;           // sum, cnt, hit: three [height][width] uint32 planes, one behind the other
  rsx::DevBuf table;            // float2[rows]
  rsx::DevBuf img, tf, out;     // staging of the host entries: images, transforms, a rendered window
  rsx::StreamOrder order;
  size_t plane_bytes() const { return (size_t)p.width * p.height * sizeof(unsigned); }
  unsigned *plane(int k) const { return planes.as<unsigned>() + (size_t)k * p.width * p.height; }
  // ---- gridmatch.hip: nothing below is allocated before the first rsx_gridmap_likelihood_* / rsx_gridmap_match_* call ----
  rsx::DevBuf like;             // uint8 [height + 2 margin][width + 2 margin]: the likelihood plane in its zeroed frame
  bool have_like = false;       // an update or a set has filled it
  rsx::DevBuf volume;           // the score volumes of a call that asked for none (uint32, n_jobs x candidates)
  // staging of the host entries of match, search and refine (gridloc_host.h): points, offsets, priors, results.  One set: every
  // one of them synchronises before it returns
  rsx::DevBuf m_xy, m_off, m_tf, m_res;
  int64_t like_pitch() const { return (int64_t)p.width + 2 * rsx::GRIDMAP_LIKE_MARGIN; }
  size_t like_bytes() const { return (size_t)like_pitch() * ((size_t)p.height + 2 * rsx::GRIDMAP_LIKE_MARGIN); }
  // ---- gridsearch.hip: nothing below is allocated before the first rsx_gridmap_search_prepare ----
  int s_cells = -1;             // the max_cells of the last prepare (-1: none yet)
  int s_margin = 0, s_cw = 0, s_ch = 0;  // the frame of that prepare: cells on every side (a multiple of 8), coarse columns and rows
  rsx::DevBuf s_frame;          // uint8 [8 s_ch][8 s_cw]: a copy of the likelihood plane in a zeroed frame of s_margin cells
  rsx::DevBuf s_pool;           // uint8 [8][8][s_ch][s_cw]: the 8 x 8 pooled plane, de-interleaved by phase
  rsx::DevBuf s_bounds, s_aux;  // workspace of a search: the bounds of a call that asked for none; seeds, prior scores, keys, counts
  // ---- gridfield.hip: nothing below is allocated before the first rsx_gridmap_likelihood_field that finds a likelihood ----
  rsx::DevBuf f_bits;           // uint64 [height][width / 64]: the seeds, a bit per cell
  rsx::DevBuf f_table;          // uint8 [radius^2 + 1]: the table of the last call, which f_table_host mirrors
  std::vector<uint8_t> f_table_host;
  uint8_t *like_origin() const { return like.as<uint8_t>() + (size_t)rsx::GRIDMAP_LIKE_MARGIN * like_pitch() + rsx::GRIDMAP_LIKE_MARGIN; }  // cell (0, 0)
};

namespace rsx {

inline int check_window(const rsx_gridmap *h, int32_t x, int32_t y, int32_t w, int32_t hgt) {
  if (x < 0 || y < 0 || w < 1 || hgt < 1 || x > h->p.width - w || y > h->p.height - hgt)
    return fail(RSX_ERR_BAD_ARG, "window %d x %d at (%d, %d) outside the %d x %d map", w, hgt, x, y, h->p.width, h->p.height);
  return RSX_OK;
}

inline int check_render(int32_t mode, int32_t min_observations) {
  if (mode != RSX_GRIDMAP_MEAN && mode != RSX_GRIDMAP_HITS) return fail(RSX_ERR_BAD_ARG, "unknown render mode %d", mode);
  if (min_observations < 1) return fail(RSX_ERR_BAD_ARG, "min_observations %d < 1", min_observations);
  return RSX_OK;
}

inline int no_likelihood() { return fail(RSX_ERR_BAD_ARG, "no likelihood plane yet: rsx_gridmap_likelihood_update or rsx_gridmap_likelihood_set first"); }

}  // namespace rsx
