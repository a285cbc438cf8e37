// crn_kernels_sc16.hip — OPTIONAL (make SC16=1 -> libcrnsense_sc16.so): samples kept in HBM in the radio's wire format (int16 pairs, 4 bytes
// per complex sample).  The wire-format (kSc16) instantiations of sense_kernel, their dispatch, and the float -> int16 pack kernel.  The
// default library is built without this file: crn_kernels.hip's launch_sense refers to launch_sense_sc16 weakly.
#include "crn_sense_impl.h"

namespace crn {

// This unit's kernels: the wire-format forms (crn_forms.h: every row carries kSc16).
struct WireUnit {
  static constexpr size_t n = kNumWireForms;
  static constexpr FormKey row(size_t i) { return kWireForms.row[i]; }
};

hipError_t launch_sense_sc16(const SenseParams &p, int fft_len, bool mag, bool win, int variant, hipStream_t stream, int *deal_rounds_run) {
  return launch_selected<WireUnit>(p, make_form_query(p, fft_len, mag, win, variant, true), stream, deal_rounds_run);
}

// complex floats -> the radio's wire format (int16 pairs, full scale 32768): crn_pack_sc16_device
__global__ __launch_bounds__(256) void pack_sc16_kernel(const float2 *iq, long long n, short2 *out, float full_scale) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float2 v = iq[i];
    out[i] = make_short2((short)fminf(fmaxf(rintf(v.x * full_scale), -32768.f), 32767.f), (short)fminf(fmaxf(rintf(v.y * full_scale), -32768.f), 32767.f));
  }
}

hipError_t launch_pack_sc16(const float *iq, long long n_samples, short *out, float full_scale, hipStream_t stream) {
  if (n_samples <= 0) return hipSuccess;
  long long blocks = (n_samples + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(pack_sc16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<const float2 *>(iq), n_samples,
                     reinterpret_cast<short2 *>(out), full_scale);
  return hipGetLastError();
}

}  // namespace crn
