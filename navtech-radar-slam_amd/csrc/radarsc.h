// radarsc.h -- internal interface of the radar scan-context builder (radarsc.hip) for sc_api.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "rsx.h"

namespace rsx {
namespace rc {

std::mutex &mutex_of(rsx_radarsc *h);
int device_of(rsx_radarsc *h);
// The callers hold the handle's mutex.  n_images device images -> n_images descriptors in the handle's scratch, enqueued on s
// (one launch, nothing read on the host); *d_descs stays valid until the handle's next call, which the handle orders behind s
int build_scratch_device(rsx_radarsc *h, const uint8_t *d_imgs, int32_t n_images, int64_t image_stride_bytes, int32_t row_stride,
                         int32_t col_offset, const float *d_azimuths, int32_t azimuths_per_image, hipStream_t s, const float **d_descs);
// the same for ONE host image and its grid (rows floats), uploaded on s first
int upload_and_build(rsx_radarsc *h, const uint8_t *img, int32_t row_stride, int32_t col_offset, const float *azimuths, hipStream_t s,
                     const float **d_descs);

}  // namespace rc
}  // namespace rsx
