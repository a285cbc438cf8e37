// crn_segments.h — emitter segments from the CFAR bin mask and their tracks (crn_segments_device, crn_tracks_device,
// include/crn_sense.h): what crn_segments.hip and crn_tracks.hip need from the rest of the library, and nothing the sensing kernels include.
#ifndef CRN_SEGMENTS_H
#define CRN_SEGMENTS_H
#include "../../include/crn_sense.h"

namespace crn {
// fft_len and the HIP device of a live handle (crn_api.cpp owns crn_handle's layout); h must not be null.
void handle_geometry(crn_handle *h, int *fft_len, int *device);
}  // namespace crn
#endif
