// crn_segments.hip — the CFAR detector's back end (crn_segments_device, include/crn_sense.h): the bit mask and the `spectrum` rows a
// CFAR launch wrote become, per epoch, an ordered list of segments (contiguous detected spans, small gaps closed, slivers dropped)
// with position, width, peak, power and power centroid, plus a noise estimate from the bins outside every segment.
//
// Mapping: one wave per epoch (a 64-thread workgroup) at every size, lane l owns the B = N / 64 contiguous bins [l B, (l + 1) B) and
// its piece of the mask in one 64-bit register.
//   1. the row is read once with coalesced float4 loads into LDS (padded by 4 floats per lane piece), the mask once from HBM;
//   2. closing is bit arithmetic on the piece (dilate by merge_gap, erode by merge_gap); the two zero runs that touch the piece's
//      edges are decided with the neighbouring non-empty lanes' trailing / leading zero counts, found with one __ballot and one __shfl;
//   3. the number of segments that END in each lane and survive min_width comes from the bits alone (an erosion by min_width - 1 and a
//      popcount of run starts), so an inclusive add scan over the wave gives every segment its slot before any power is summed.
//      Segments are disjoint, so ascending end equals ascending lo except for the one segment that crosses the wrap: it ends first and
//      is stored last;
//   4. each lane walks its B bins once (LDS reads), emitting the segments that start and end inside it and keeping the run that
//      touches its low edge (head) and the one that leaves through its high edge (tail);
//   5. a segmented scan over lanes (6 steps, circular) joins tail + whole lanes, and the lane where a spanning segment ends adds its
//      head and emits it.
// Sums are fp64 and offsets are relative to the segment's own lo at every join (no cancellation), rounded to fp32 once.
// A lane never walks more than its own B <= 64 bins, whatever the mask holds; no atomics, no scratch, plain vector stores.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "crn_internal.h"
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

__device__ __forceinline__ int ctz64(uint64_t x) { return x ? __builtin_ctzll(x) : 64; }
__device__ __forceinline__ int clz64(uint64_t x) { return x ? __builtin_clzll(x) : 64; }
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return r ? (x << r) | (x >> (64 - r)) : x; }
__device__ __forceinline__ uint64_t rotr64(uint64_t x, int r) { return r ? (x >> r) | (x << (64 - r)) : x; }
__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// bit x of the result = OR (AND) of bits x - i (x + i) of the argument, 0 <= i <= g <= 63; zeros come in at the ends
__device__ __forceinline__ uint64_t or_up(uint64_t x, int g) {
  int c = 1;
  for (; 2 * c <= g + 1; c *= 2) x |= x << c;
  return x | (x << (g + 1 - c));
}
__device__ __forceinline__ uint64_t or_down(uint64_t x, int g) {
  int c = 1;
  for (; 2 * c <= g + 1; c *= 2) x |= x >> c;
  return x | (x >> (g + 1 - c));
}
__device__ __forceinline__ uint64_t and_down(uint64_t x, int g) {
  int c = 1;
  for (; 2 * c <= g + 1; c *= 2) x &= x >> c;
  return x & (x >> (g + 1 - c));
}

template <int B>
__global__ __launch_bounds__(64) void segments_kernel(const SegParams p) {
  constexpr int N = 64 * B;
  constexpr int PAD = 4;                     // floats between lane pieces in LDS: a lane's float4 reads then spread over the banks
  constexpr uint64_t PM = B == 64 ? ~0ull : (1ull << (B % 64)) - 1;
  __shared__ float4 row4[(N + 64 * PAD) / 4];
  float *row = reinterpret_cast<float *>(row4);
  const int l = threadIdx.x;
  const long long e = p.first + blockIdx.x;

  // 1. the row: coalesced from HBM, to the lane that owns the bins through LDS
  const float4 *src = reinterpret_cast<const float4 *>(p.spectrum + e * N);
#pragma unroll
  for (int j = 0; j < B / 4; j++) {
    const int k = 4 * (j * 64 + l);
    *reinterpret_cast<float4 *>(row + k + (k / B) * PAD) = src[j * 64 + l];
  }
  const uint32_t *mw = p.mask + e * (N / 32);
  uint64_t d;
  if (B == 64) {
    const uint2 w = reinterpret_cast<const uint2 *>(mw)[l];
    d = (uint64_t)w.x | ((uint64_t)w.y << 32);
  } else if (B == 32) {
    d = mw[l];
  } else {
    d = (mw[l / (32 / B)] >> ((l % (32 / B)) * B)) & PM;
  }

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

  // 3. run structure from the bits.  An all-ones circle is cut between lane 63 and lane 0: one segment, lo = 0, width = N.
  const bool all_ones = __ballot(c == PM) == ~0ull;
  const uint64_t tops = __ballot((c >> (B - 1)) & 1), lows = __ballot(c & 1);
  const bool cont_in = (c & 1) && ((tops >> ((l - 1) & 63)) & 1) && !(all_ones && l == 0);
  const bool cont_out = ((c >> (B - 1)) & 1) && ((lows >> ((l + 1) & 63)) & 1) && !(all_ones && l == 63);
  const bool pass = c == PM && cont_in && cont_out;          // a lane in the middle of a segment
  const int headlen = cont_in ? ctz64(~c & PM) < B ? ctz64(~c & PM) : B : 0;
  const int taillen = cont_out ? (clz64(~(c << (64 - B))) < B ? clz64(~(c << (64 - B))) : B) : 0;
  // the bins a segment has gathered before it enters this lane: whole lanes back to the nearest lane that is not `pass`, and its tail
  const uint64_t pt = __ballot(pass);
  const int dist_s = clz64(rotl64(~pt, (64 - l) & 63));
  const int carry_w = dist_s * B + __shfl(taillen, (l - 1 - dist_s) & 63, 64);
  const bool head_final = cont_in && !pass;                  // a segment from an earlier lane ends here
  const int head_w = carry_w + headlen;
  const int head_lo = l * B + headlen - head_w;              // < 0: it crosses the wrap
  const bool head_kept = head_final && head_w >= p.min_width;
  const uint64_t own = c & ~low_bits(headlen) & low_bits(B - taillen);   // runs that start and end in this lane
  const uint64_t er = p.min_width - 1 >= B ? 0 : and_down(own, p.min_width - 1);
  const int cnt = __popcll(er & ~(er << 1)) + (head_kept ? 1 : 0);
  int incl = cnt;
#pragma unroll
  for (int s = 1; s < 64; s *= 2) {
    const int y = __shfl_up(incl, s, 64);
    if (l >= s) incl += y;
  }
  const int n_found = __shfl(incl, 63, 64);
  const int n_stored = n_found < p.max_segments ? n_found : p.max_segments;
  const bool wrap_kept = __ballot(head_kept && head_lo < 0) != 0;   // that segment ends first (rank 0) and is stored last
  crn_segment *segs = p.segments ? p.segments + e * p.max_segments : nullptr;

  auto emit = [&](const Acc &s, int lo, int rank) {
    const int slot = wrap_kept ? (rank == 0 ? n_found - 1 : rank - 1) : rank;
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
  int rank = incl - cnt + (head_kept ? 1 : 0);
  bool in_head = cont_in;
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
  const float *mine = row + l * (B + PAD);
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
  if (a.w && !cont_out) close_run(B);

  // 5. spanning segments: v = what leaves this lane through its high edge, joined back to the lane where the segment started
  Acc v = cont_out ? a : acc_zero();
  bool done = !pass;
#pragma unroll
  for (int s = 1; s < 64; s *= 2) {
    const Acc o = acc_from(v, (l - s) & 63);
    const bool o_done = __shfl((int)done, (l - s) & 63, 64) != 0;
    if (!done) {
      v = acc_join(o, v);
      done = o_done;
    }
  }
  const Acc carry = acc_from(v, (l - 1) & 63);
  if (head_kept) emit(acc_join(carry, head), head_lo < 0 ? head_lo + N : head_lo, incl - cnt);

  // the epoch's header, and zeros in the slots nobody filled
  int nbins = B - __popcll(c);
#pragma unroll
  for (int s = 32; s > 0; s /= 2) {
    nbins += __shfl_xor(nbins, s, 64);
    nsum += __shfl_xor(nsum, s, 64);
  }
  if (l == 0) {
    crn_segment_epoch h;
    h.n_found = n_found;
    h.n_stored = n_stored;
    h.noise_bins = nbins;
    h.noise_mean = nbins ? (float)(nsum / (double)nbins) : 0.0f;
    p.epochs[e] = h;
  }
  if (segs != nullptr) {
    crn_segment z{};
    for (int s = n_stored + l; s < p.max_segments; s += 64) segs[s] = z;
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
  const int64_t chunk = int64_t(1) << 30;   // workgroups per grid: one launch for any batch that fits a device
  for (int64_t first = 0; err == hipSuccess && first < n_epochs; first += chunk) {
    p.first = first;
    const unsigned cnt = (unsigned)(n_epochs - first < chunk ? n_epochs - first : chunk);
    err = n == 512 ? crn::launch<8>(p, cnt, st) : n == 1024 ? crn::launch<16>(p, cnt, st) : n == 2048 ? crn::launch<32>(p, cnt, st) : crn::launch<64>(p, cnt, st);
  }
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_segments_device: ") + hipGetErrorString(err));
  return CRN_OK;
}
