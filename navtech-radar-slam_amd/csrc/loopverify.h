// loopverify.h -- internal interface of the keyframe-cloud store (loopverify.hip) for sc_api.cpp.
#pragma once
#include <cstdint>
#include <mutex>

#include "rsx.h"

namespace rsx {
namespace kf {

std::mutex &mutex_of(rsx_kfstore *h);
int device_of(rsx_kfstore *h);
// keyframeLaserClouds.push_back: n packed float4 {x, y, z, intensity} that are complete in this device's memory; the caller
// holds the store's mutex.  Returns once the copy is done (the source may be overwritten).
int append_device_locked(rsx_kfstore *h, const void *d_xyzi, int64_t n, int32_t *out_index);
// keyframe `index` where it lies in the store: *d_xyzi = its first packed float4, *n = its points (RSX_ERR_BAD_ARG for an index
// that is not stored); the caller holds the store's mutex for as long as it reads there (csrc/coral.hip)
int keyframe_device_locked(rsx_kfstore *h, int32_t index, const float **d_xyzi, int64_t *n);

}  // namespace kf
}  // namespace rsx
