// phasecorr.h -- the handle of the rsx_phasecorr entries (csrc/phasecorr.hip).
#pragma once
#include <mutex>

#include "rsx_common.h"

struct rsx_phasecorr {
  int device = 0;
  std::mutex mu;
  rsx::Stream stream;
  rsx::StreamOrder order;  // the workspace and the staging buffers are shared by every call
  rsx_phasecorr_params p{};
  int rows = 0, cols = 0;
  rsx::DevBuf tables;      // map | cos / sin | directions | Hann | high-pass cosines, made by rsx_phasecorr_create
  rsx::DevBuf work;        // the slots of the scans and the pairs of the call in flight (include/rsx.h states its size)
  int last_images = 0, last_pairs = -1;  // the layout of `work` as the last call left it (rsx_phasecorr_correlation)
  rsx::DevBuf imgs, pairs, res, cart;    // staging of the host-buffer entry
};
