// coral.h -- the handle of the rsx_coral entries (csrc/coral.hip).
#pragma once
#include <mutex>

#include "rsx_common.h"

struct rsx_coral {
  int device = 0;
  std::mutex mu;
  rsx::Stream stream;
  rsx::StreamOrder order;  // the workspace and the staging buffers are shared by every call
  rsx::DevBuf work;        // the joint clouds of the jobs in flight: 128 KiB per workgroup, min(n_jobs, 256) workgroups
  rsx::DevBuf a, b, a_off, b_off, tf, res, pts;  // staging of the host-buffer entries
};
