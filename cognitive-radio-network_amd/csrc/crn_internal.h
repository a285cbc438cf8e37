// crn_internal.h — error plumbing and internal calls shared by the host translation units of libcrnsense.
#ifndef CRN_INTERNAL_H
#define CRN_INTERNAL_H
#include <string>

#include "../../include/crn_sense.h"

namespace crn {
// Records the thread-local message returned by crn_last_error() and returns `code`.
int fail(int code, const std::string &msg);
}  // namespace crn

// Calls between the library's own translation units (hidden: no CRN_API), defined in crn_api.cpp: the configuration a handle holds, a ring
// attaching (+1) or detaching (-1), an empty launch that wakes an idle stream, and a launch on either sample format (4 or 8 bytes)
extern "C" {
int crn_sense_cfg_of(crn_handle *h, crn_cfg *out);
int crn_sense_ring_count(crn_handle *h, int delta);
int crn_sense_warm_stream(crn_handle *h, void *stream);
int crn_sense_run_device_any(crn_handle *h, const void *d_iq, int32_t bytes_per_sample, int64_t n_epochs, int32_t samples_per_frame,
                             int64_t epoch_stride, const crn_out *d_out, void *stream);
}

// A HIP call that must succeed: otherwise the enclosing function returns CRN_ERR_DEVICE with the call's text and HIP's message.
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return crn::fail(CRN_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));     \
  } while (0)
#endif
