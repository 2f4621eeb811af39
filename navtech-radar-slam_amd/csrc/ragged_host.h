// ragged_host.h -- what the host-buffer entries of a ragged batch share (rsx_orora_register_batch, rsx_orora_max_clique_batch,
// rsx_ransac_estimate_batch, rsx_mocomp_points_batch, rsx_mocomp_matches_batch): per-match arrays, offsets[n + 1] and per-group
// arrays go up, per-match and per-group results come down.  The one check of the offsets, and the staging of one array.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rsx_common.h"

namespace rsx {

// group i owns elements [offsets[i], offsets[i + 1]): offsets[0] == 0 and no entry below the one before it (so none is negative).
// Only a host entry can look: a kernel trusts the offsets it is given
inline int check_offsets(const int64_t *offsets, int32_t n, const char *what) {
  if (offsets[0] != 0) return fail(RSX_ERR_BAD_ARG, "%s: offsets must start at 0 (entry 0 is %lld)", what, (long long)offsets[0]);
  for (int32_t i = 1; i <= n; i++)
    if (offsets[i] < offsets[i - 1])
      return fail(RSX_ERR_BAD_ARG, "%s: offsets must not decrease (entry %d is %lld after %lld)", what, i, (long long)offsets[i],
                  (long long)offsets[i - 1]);
  return RSX_OK;
}

// The zero-length rule lives here: an array of no bytes still gets a buffer (a kernel is never handed a null pointer) and is
// not copied.  b holds at least `bytes` afterwards
inline int stage_room(DevBuf &b, size_t bytes, hipStream_t s) { return b.reserve(bytes ? bytes : 1, s, false); }

// room, then host -> b
inline int stage_up(DevBuf &b, const void *host, size_t bytes, hipStream_t s) {
  RSX_TRY(stage_room(b, bytes, s));
  if (bytes) RSX_HIP(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, s));
  return RSX_OK;
}

// b -> host; a null host pointer is an output the caller did not ask for
inline int stage_down(void *host, const DevBuf &b, size_t bytes, hipStream_t s) {
  if (host && bytes) RSX_HIP(hipMemcpyAsync(host, b.p, bytes, hipMemcpyDeviceToHost, s));
  return RSX_OK;
}

}  // namespace rsx
