// crn_segments.hip — the CFAR detector's back end (crn_segments_device, include/crn_sense.h): the bit mask and the `spectrum` rows a
// CFAR launch wrote become, per epoch, an ordered list of segments (contiguous detected spans, small gaps closed, slivers dropped)
// with position, width, peak, power and power centroid, plus a noise estimate from the bins outside every segment.
//
// Mapping: one wave per epoch (a 64-thread workgroup) at every size, lane l owns the B = N / 64 contiguous bins [l B, (l + 1) B) and
// its piece of the mask in one 64-bit register.
//   1. the row is read once with coalesced float4 loads into LDS (padded by 4 floats per lane piece), the mask once from HBM;
//   2. closing is bit arithmetic on the piece (dilate by merge_gap, erode by merge_gap); the two zero runs that touch the piece's
//      edges are decided with the neighbouring non-empty lanes' trailing / leading zero counts, found with one __ballot and one __shfl;
//   3. the number of segments that END in each lane and survive min_width comes from the bits alone, so an add scan over the wave gives
//      every segment its slot before any power is summed; the segment that crosses the wrap ends first and is stored last (run_plan<B>);
//   4. each lane walks its B bins once (LDS reads), emitting the segments that start and end inside it and keeping the run that
//      touches its low edge (head) and the one that leaves through its high edge (tail);
//   5. a segmented circular scan over lanes joins tail + whole lanes (join_spanning); the lane where a spanning segment ends adds its head.
// The mapping of 1, the bit helpers, 3 and 5 are in crn_mask_runs.h: the spectrum holes (crn_holes.hip) run them over an accumulator of
// their own, the channel statistics (crn_channels.hip) use the mapping.
// Sums are fp64 and offsets are relative to the segment's own lo at every join (no cancellation), rounded to fp32 once.
// A lane never walks more than its own B <= 64 bins, whatever the mask holds; no atomics, no scratch, plain vector stores.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_mask_runs.h"
#include "crn_segments.h"

namespace crn {
namespace {

struct SegParams {
  const uint32_t *mask;       // [n_epochs][N / 32]
  const float *spectrum;      // [n_epochs][N]
  crn_segment_epoch *epochs;  // [n_epochs]
  crn_segment *segments;      // [n_epochs][max_segments] or null
  long long first;            // epoch of workgroup 0
  int merge_gap, min_width, max_segments;
};

// what a run of bins has accumulated; offsets (arg, s1) count from the run's own first bin
struct Acc {
  int w, nd, arg;   // bins, set bits of the raw mask, offset of the largest P
  float mx;         // that P (-1: none yet; P >= 0)
  double s0, s1;    // sum P, sum offset * P
};

__device__ __forceinline__ Acc acc_zero() { return Acc{0, 0, 0, -1.0f, 0.0, 0.0}; }

// a, then b right behind it
__device__ __forceinline__ Acc acc_join(const Acc &a, const Acc &b) {
  Acc r;
  r.s1 = a.s1 + b.s1 + (double)a.w * b.s0;
  r.s0 = a.s0 + b.s0;
  r.nd = a.nd + b.nd;
  const bool later = b.mx > a.mx;   // ties stay with the earlier bin
  r.mx = later ? b.mx : a.mx;
  r.arg = later ? a.w + b.arg : a.arg;
  r.w = a.w + b.w;
  return r;
}

__device__ __forceinline__ Acc acc_from(const Acc &a, int lane) {
  Acc r;
  r.w = __shfl(a.w, lane, 64);
  r.nd = __shfl(a.nd, lane, 64);
  r.arg = __shfl(a.arg, lane, 64);
  r.mx = __shfl(a.mx, lane, 64);
  r.s0 = __shfl(a.s0, lane, 64);
  r.s1 = __shfl(a.s1, lane, 64);
  return r;
}

template <int B>
__global__ __launch_bounds__(64) void segments_kernel(const SegParams p) {
  constexpr int N = 64 * B;
  constexpr uint64_t PM = piece_bits(B);
  __shared__ float4 row4[padded_words(B) / 4];
  float *row = reinterpret_cast<float *>(row4);
  const int l = threadIdx.x;
  const long long e = p.first + blockIdx.x;

  // 1. the row: coalesced from HBM, to the lane that owns the bins through LDS; the lane's piece of the mask
  load_row<B>(row, p.spectrum + e * N, l);
  const uint64_t d = mask_piece<B>(p.mask + e * (N / 32), l);

  // 2. closing
  const int g = p.merge_gap;
  const uint64_t nz = __ballot(d != 0);
  uint64_t c = d;
  if (nz != 0 && g > 0) {
    const int lowz = d ? ctz64(d) : B, highz = d ? clz64(d) - (64 - B) : B;
    // the nearest non-empty lane on each side (circular; the lane itself when it is the only one)
    const int dist_p = clz64(rotl64(nz, (64 - l) & 63)), dist_n = ctz64(rotr64(nz, (l + 1) & 63));
    const int prev_gap = dist_p * B + __shfl(highz, (l - 1 - dist_p) & 63, 64);
    const int next_gap = dist_n * B + __shfl(lowz, (l + 1 + dist_n) & 63, 64);
    if (d == 0) {
      c = prev_gap + B + next_gap <= g ? PM : 0;
    } else {
      const int gi = g < 63 ? g : 63;   // a zero run between two ones of one piece is at most 62 long
      const uint64_t dil = or_up(d, gi) & PM;
      const uint64_t inner = ~or_down(~dil & PM, gi) & PM;   // beyond the piece counts as ones here: the edge runs are decided below
      const uint64_t lowm = low_bits(lowz), highm = PM & ~low_bits(B - highz);
      c = (inner & ~lowm & ~highm) | d;
      if (prev_gap + lowz <= g) c |= lowm;
      if (highz + next_gap <= g) c |= highm;
    }
  }

  // 3. run structure from the bits
  const RunPlan plan = run_plan<B>(c, l, p.min_width, p.max_segments);
  crn_segment *segs = p.segments ? p.segments + e * p.max_segments : nullptr;

  auto emit = [&](const Acc &s, int lo, int rank) {
    const int slot = plan.slot(rank);
    if (segs == nullptr || slot >= p.max_segments) return;
    crn_segment o;
    o.lo = lo;
    o.width = s.w;
    o.peak_bin = (lo + s.arg) & (N - 1);
    o.n_detected = s.nd;
    o.power = (float)s.s0;
    o.peak_power = s.mx;
    o.centroid = s.s0 > 0.0 ? (float)(s.s1 / s.s0) : 0.0f;
    o.reserved = 0.0f;
    segs[slot] = o;
  };

  // 4. one walk over the lane's bins
  __syncthreads();
  Acc a = acc_zero(), head = acc_zero();
  double nsum = 0.0;
  int rank = plan.incl - plan.cnt + (plan.head_kept ? 1 : 0);
  bool in_head = plan.cont_in;
  auto close_run = [&](int end) {
    if (in_head) {
      head = a;
    } else if (a.w >= p.min_width) {
      emit(a, l * B + end - a.w, rank);
      rank++;
    }
    a = acc_zero();
    in_head = false;
  };
  const float *mine = own_piece<B>(row, l);
#pragma unroll 1
  for (int i4 = 0; i4 < B; i4 += 4) {
    const float4 q = *reinterpret_cast<const float4 *>(mine + i4);
    const float pv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = i4 + j;
      const float P = pv[j];
      if ((c >> i) & 1) {
        if (P > a.mx) {
          a.mx = P;
          a.arg = a.w;
        }
        a.s1 += (double)a.w * (double)P;
        a.s0 += (double)P;
        a.w++;
        a.nd += (int)((d >> i) & 1);
      } else {
        nsum += (double)P;
        if (a.w) close_run(i);
      }
    }
  }
  if (a.w && !plan.cont_out) close_run(B);

  // 5. spanning segments: what leaves this lane through its high edge is joined back to the lane where the segment started
  const Acc carry = join_spanning(plan.cont_out ? a : acc_zero(), plan.pass, l);
  if (plan.head_kept) emit(acc_join(carry, head), plan.head_lo < 0 ? plan.head_lo + N : plan.head_lo, plan.incl - plan.cnt);

  // the epoch's header, and zeros in the slots nobody filled
  int nbins = B - __popcll(c);
#pragma unroll
  for (int s = 32; s > 0; s /= 2) {
    nbins += __shfl_xor(nbins, s, 64);
    nsum += __shfl_xor(nsum, s, 64);
  }
  if (l == 0) {
    crn_segment_epoch h;
    h.n_found = plan.n_found;
    h.n_stored = plan.n_stored;
    h.noise_bins = nbins;
    h.noise_mean = nbins ? (float)(nsum / (double)nbins) : 0.0f;
    p.epochs[e] = h;
  }
  if (segs != nullptr) {
    crn_segment z{};
    for (int s = plan.n_stored + l; s < p.max_segments; s += 64) segs[s] = z;
  }
}

template <int B>
hipError_t launch(const SegParams &p, unsigned n, hipStream_t stream) {
  hipLaunchKernelGGL(segments_kernel<B>, dim3(n), dim3(64), 0, stream, p);
  return hipGetLastError();
}

}  // namespace
}  // namespace crn

int crn_segments_device(crn_handle *h, const uint32_t *d_bin_mask, const float *d_spectrum, int64_t n_epochs,
                        const crn_segment_params *params, crn_segment_epoch *d_epochs, crn_segment *d_segments, void *stream) {
  static_assert(sizeof(crn_segment_params) == 16 && sizeof(crn_segment) == 32 && sizeof(crn_segment_epoch) == 16, "include/crn_sense.h");
  if (!h || !params || !d_bin_mask || !d_spectrum || !d_epochs)
    return crn::fail(CRN_ERR_ARG, "crn_segments_device: null handle / params / mask / spectrum / epochs");
  if (n_epochs < 0) return crn::fail(CRN_ERR_ARG, "crn_segments_device: n_epochs < 0");
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  if (params->merge_gap < 0 || params->merge_gap >= n) return crn::fail(CRN_ERR_ARG, "crn_segments_device: merge_gap must be in 0..fft_len - 1");
  if (params->min_width < 1) return crn::fail(CRN_ERR_ARG, "crn_segments_device: min_width < 1");
  if (params->max_segments < 1 || params->max_segments > 256) return crn::fail(CRN_ERR_ARG, "crn_segments_device: max_segments must be in 1..256");
  if (params->reserved != 0) return crn::fail(CRN_ERR_ARG, "crn_segments_device: reserved must be 0");
  if ((reinterpret_cast<uintptr_t>(d_spectrum) & 15) || (reinterpret_cast<uintptr_t>(d_bin_mask) & 7))
    return crn::fail(CRN_ERR_ARG, "crn_segments_device: d_spectrum must be 16-byte and d_bin_mask 8-byte aligned");
  if (n_epochs == 0) return CRN_OK;
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  crn::SegParams p{d_bin_mask, d_spectrum, d_epochs, d_segments, 0, params->merge_gap, params->min_width, params->max_segments};
  err = crn::in_grids(err, n_epochs, [&](int64_t first, unsigned cnt) {
    p.first = first;
    return n == 512 ? crn::launch<8>(p, cnt, st) : n == 1024 ? crn::launch<16>(p, cnt, st) : n == 2048 ? crn::launch<32>(p, cnt, st) : crn::launch<64>(p, cnt, st);
  });
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_segments_device: ") + hipGetErrorString(err));
  return CRN_OK;
}
