// cen2018.h -- what other translation units of librsx need of csrc/cen2018.hip (the odometry handle validates its
// cen2018 settings before it creates the extraction handles).
#pragma once
#include "rsx.h"

namespace rsx {
// RSX_OK, or RSX_ERR_BAD_ARG with the message set: sigma_gauss odd in [1, 85], min_range >= 0, zq finite
int cen2018_check_params(const rsx_cen2018_params &p);
}  // namespace rsx
