// cfar.h -- what other translation units of librsx need of csrc/cfar.hip (the odometry handle validates its CFAR settings
// before it creates the extraction handles).
#pragma once
#include "rsx.h"

namespace rsx {
// RSX_OK, or RSX_ERR_BAD_ARG with the message set: k in [1, 128], train in [1, 64], guard in [0, 16], scale_q8 in [0, 65535],
// offset in [0, 255], mode in [0, 2], min_range >= 0, max_range >= 0, min_separation in [0, 32], reserved == 0
int cfar_check_params(const rsx_cfar_params &p);
}  // namespace rsx
