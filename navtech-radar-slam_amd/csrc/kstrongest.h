// kstrongest.h -- what other translation units of librsx need of csrc/kstrongest.hip (the odometry handle validates its
// k-strongest settings before it creates the extraction handles).
#pragma once
#include "rsx.h"

namespace rsx {
// RSX_OK, or RSX_ERR_BAD_ARG with the message set: k in [1, 128], z_min in [0, 255], min_range >= 0, max_range >= 0,
// min_separation in [0, 32]
int kstrongest_check_params(const rsx_kstrongest_params &p);
}  // namespace rsx
