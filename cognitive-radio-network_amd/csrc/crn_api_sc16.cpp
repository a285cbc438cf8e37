// crn_api_sc16.cpp — the optional wire-format (int16) entry points on a handle: in libcrnsense_sc16.so and libcrnsense_plain.so only.
#include "../../include/crn_sense_sc16.h"
#include "crn_handle.h"
#include "crn_kernels.h"

int crn_sense_run_device_sc16(crn_handle *h, const int16_t *d_iq, int64_t n_epochs, int32_t samples_per_frame,
                              int64_t epoch_stride, const crn_out *d_out, void *stream) {
  return crn_sense_run_device_any(h, d_iq, 4, n_epochs, samples_per_frame, epoch_stride, d_out, stream);
}

int crn_sense_set_wire_full_scale(crn_handle *h, double full_scale) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  if (!(full_scale >= 1.0 && full_scale <= 65536.0)) return crn::fail(CRN_ERR_ARG, "full_scale must be in 1..65536");
  std::lock_guard<std::mutex> lk(h->tables_mu);
  h->wire_full_scale = full_scale;
  return CRN_OK;
}

int crn_pack_sc16_device(crn_handle *h, const float *d_iq, int64_t n_samples, int16_t *d_out, void *stream) {
  if (!h || !d_iq || !d_out) return crn::fail(CRN_ERR_ARG, "null handle / buffer");
  if (n_samples < 0) return crn::fail(CRN_ERR_ARG, "n_samples < 0");
  std::lock_guard<std::mutex> lk(h->tables_mu);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(crn::launch_pack_sc16(d_iq, n_samples, d_out, (float)h->wire_full_scale, static_cast<hipStream_t>(stream)));
  return CRN_OK;
}
