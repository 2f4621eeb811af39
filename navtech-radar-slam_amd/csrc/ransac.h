// ransac.h -- what csrc/odometry.hip shares with csrc/ransac.hip beside the public entries of include/rsx.h.
#pragma once
#include "rsx_common.h"

namespace rsx {

// the parameter rules of rsx_ransac_estimate_batch{,_device} (RSX_ERR_BAD_ARG + message, or RSX_OK)
int ransac_check_params(const rsx_ransac_params &p);

}  // namespace rsx
