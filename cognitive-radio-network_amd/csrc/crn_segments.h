// crn_segments.h — what the units behind the CFAR launch (segments, tracks, channels, fusion, holes) need from the rest of the library and
// share on the host side, and nothing the sensing kernels include: a live handle's geometry, the alignment check, the launch in grids,
// and the chunking of a stream's epochs.
#ifndef CRN_SEGMENTS_H
#define CRN_SEGMENTS_H
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/crn_sense.h"

namespace crn {
// fft_len and the HIP device of a live handle (crn_api.cpp owns crn_handle's layout); h must not be null.
void handle_geometry(crn_handle *h, int *fft_len, int *device);

inline bool misaligned(const void *ptr, uintptr_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) != 0; }

// launch(first, count) over the workgroups [0, total) in grids of at most 2^30 (one launch for any batch that fits a device), as long
// as err is hipSuccess; the first error is returned
template <class F>
hipError_t in_grids(hipError_t err, int64_t total, F launch) {
  const int64_t grid = int64_t(1) << 30;
  for (int64_t first = 0; err == hipSuccess && first < total; first += grid) err = launch(first, (unsigned)(total - first < grid ? total - first : grid));
  return err;
}

constexpr int MAX_N = 4096;   // the largest fft_len: what a bin count is held to where no handle says more
constexpr int CHUNK = 64;     // epochs of a stream that one workgroup of the time-parallel kernels takes
inline int64_t chunks_per_stream(int epochs_per_stream) { return (int64_t(epochs_per_stream) + CHUNK - 1) / CHUNK; }   // 64-bit: close to 2^31

#ifdef __HIPCC__
// chunk `chunk` of all streams', `chunks` to a stream of eps epochs: the stream and the chunk's epochs t0 .. t0 + n - 1 of it, n in 1..64
struct ChunkSpan {
  long long stream;
  int t0, n;
};
__device__ __forceinline__ ChunkSpan chunk_span(long long chunk, int chunks, int eps) {
  ChunkSpan s;
  s.stream = chunk / chunks;
  s.t0 = (int)(chunk - s.stream * chunks) * CHUNK;
  s.n = eps - s.t0 < CHUNK ? eps - s.t0 : CHUNK;
  return s;
}
#endif
}  // namespace crn
#endif
