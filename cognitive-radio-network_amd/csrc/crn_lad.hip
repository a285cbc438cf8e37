// crn_lad.hip — wideband detection against an excised noise floor (crn_lad_device, include/crn_sense.h): a `spectrum` row becomes the
// FCME floor of each of its blocks, the lower and upper threshold masks against it, and the union of the lower clusters that hold an
// upper bin, OR-ed with an optional mask (the CFAR mask of the same launch), plus a 32-byte header and the floors.  One launch, the
// mapping of segments_kernel<B> (crn_mask_runs.h): one wave per row of N = 64 B bins, lane l keeps its B bins in registers and its piece
// of every mask in one 64-bit register; a block of the row is a group of 64 / n_blocks lanes, and a block reduction is a butterfly
// over the group.  No sort:
//
//   1. select  the n0 smallest values of a block by bisection on the bit pattern (non-negative floats order as integers), between the
//              block's smallest and largest: a pass counts the values <= the pivot; a block is done when the count is n0, or when the
//              interval is one pattern wide and the ties at the pivot are taken by count.  At most 32 passes whatever the row holds;
//              noise in eight blocks of 512 bins takes 12 on average.
//   2. floor   the fixed point that equals the forward search: take every value with x n <= t_cme C, count and sum (fp64)
//              them, until the set stops growing.  Each pass either ends a block or adds a bin to it: no cap is needed.
//   3. masks   lower and upper.  Here as in 1 and 2 a comparison (double)x n > lim of the definition is made once per pass in fp64, to
//              find the float pattern that parts the bins (cut()); a bin then costs a subtraction whose sign is the answer: no
//              condition code goes through a scalar register, and the signs shift into the mask word directly.
//   4. clusters  inside a lane a run is flooded from its upper bits with one add (the carry runs up a run of ones; the same on the
//              reversed word for the way down).  Across lanes "an upper bin somewhere before / after this lane in the run that crosses
//              the edge" is a carry chain over the 64 lanes: generate = the edge run holds an upper bin, propagate = the lane is all
//              ones, solved on ballots with a circular Kogge-Stone scan (scalar instructions only), once upwards and once downwards.
// The values are never used as an index or a trip count, so a row of NaNs or negative values costs time inside its own outputs only.
// No scratch memory, no global atomics, plain vector stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_mask_runs.h"
#include "crn_segments.h"

namespace crn {
namespace {

struct LadParams {
  const float *spectrum;     // [n_epochs][N]
  const uint32_t *or_mask;   // [n_epochs][N / 32] or null
  uint32_t *mask;            // [n_epochs][N / 32] or null
  crn_lad_row *rows;         // [n_epochs] or null
  float *floor;              // [n_epochs][n_blocks] or null
  long long first;           // row of workgroup 0
  int n_blocks, n0;          // n0: the bins of a block taken as surely noise
  float t_cme, t_lower, t_upper;
};

// One step of a butterfly over a group of lanes: the value of the lane that holds the other half of the 2 S lanes this one lies in.
// Inside a row of 16 lanes it is a DPP move (no trip through the LDS crossbar, whose latency a wave with one partner on its SIMD cannot
// hide): the quad permutations for S = 1 and 2, and for S = 4 and 8 the mirror of the half row and of the row, i -> 7 - i and
// i -> 15 - i, which name a lane of the other half: that serves a reduction that takes its steps in ascending order, since after the
// steps below S all lanes of a half hold the same value.  Beyond a row it is __shfl_xor.
template <int S>
__device__ __forceinline__ int partner(int v) {
  if constexpr (S == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);          // quad_perm [1, 0, 3, 2]
  else if constexpr (S == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);     // quad_perm [2, 3, 0, 1]
  else if constexpr (S == 4) return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);    // row_half_mirror
  else if constexpr (S == 8) return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);    // row_mirror
  else return __shfl_xor(v, S, 64);
}
template <int S>
__device__ __forceinline__ double partner(double v) {
  return __hiloint2double(partner<S>(__double2hiint(v)), partner<S>(__double2loint(v)));
}

// f over the group of g lanes (8, 16, 32 or 64) the lane lies in, in every lane of it
template <class T, class F>
__device__ __forceinline__ T group_reduce(T v, int g, F f) {
  v = f(v, partner<1>(v));
  v = f(v, partner<2>(v));
  v = f(v, partner<4>(v));
  if (g > 8) v = f(v, partner<8>(v));
  if (g > 16) v = f(v, partner<16>(v));
  if (g > 32) v = f(v, partner<32>(v));
  return v;
}
__device__ __forceinline__ int group_sum(int v, int g) { return group_reduce(v, g, [](int a, int b) { return a + b; }); }
__device__ __forceinline__ double group_sum(double v, int g) { return group_reduce(v, g, [](double a, double b) { return a + b; }); }

// The bit pattern of the largest non-negative float f with (double)f n <= lim, so that for a non-negative x
//   (double)x n > lim  <=>  pattern(x) > cut(lim, n):
// one integer compare per bin instead of a conversion, an fp64 product and an fp64 compare.  The quotient lim / n is within 2^-53 of the
// true one and floats lie 2^-24 apart, so the float next to its rounding is tried on either side; f n is exact in fp64 (24 + 12 bits).
__device__ __forceinline__ uint32_t cut(double lim, double n) {
  uint32_t b = __float_as_uint((float)(lim / n));
  if ((double)__uint_as_float(b) * n > lim) {
    if (b != 0) b--;
  } else if (!((double)__uint_as_float(b + 1) * n > lim)) {
    b++;
  }
  return b;
}

// the runs of ones of m that hold a bit of s (s inside m), from that bit upwards: the carry of m + s runs to the top of the run
__device__ __forceinline__ uint64_t flood_up(uint64_t m, uint64_t s) { return (((m + s) ^ m) & m) | s; }

// carry[l] = gen[l] | prop[l] & carry[l - 1] around the circle of 64 lanes (UP), or with l + 1 (!UP)
template <bool UP>
__device__ __forceinline__ uint64_t carry_chain(uint64_t gen, uint64_t prop) {
#pragma unroll
  for (int d = 1; d < 64; d *= 2) {
    gen |= prop & (UP ? rotl64(gen, d) : rotr64(gen, d));
    prop &= UP ? rotl64(prop, d) : rotr64(prop, d);
  }
  return gen;
}

// the circular runs of ones in the wave's mask that start in this lane; prev_top: the last bit of the lane before
template <int B>
__device__ __forceinline__ int run_starts(uint64_t m, bool prev_top) {
  return __popcll(m & ~((m << 1) | (prev_top ? 1ull : 0ull)) & piece_bits(B));
}

template <int B>
__global__ __launch_bounds__(64) void lad_kernel(const LadParams p) {
  constexpr int N = 64 * B;
  constexpr uint64_t PM = piece_bits(B);
  __shared__ float4 row4[padded_words(B) / 4];
  float *row = reinterpret_cast<float *>(row4);
  const int l = threadIdx.x;
  const long long e = p.first + blockIdx.x;
  const int G = 64 / p.n_blocks, M = G * B;      // lanes and bins of a block

  // the row: coalesced from HBM, to the lane that owns the bins through LDS; the lane's piece of the mask to OR in
  load_row<B>(row, p.spectrum + e * N, l);
  const uint64_t om = p.or_mask != nullptr ? mask_piece<B>(p.or_mask + e * (N / 32), l) : 0;
  __syncthreads();
  float x[B];
  {
    const float *mine = own_piece<B>(row, l);
#pragma unroll
    for (int i4 = 0; i4 < B; i4 += 4) {
      const float4 q = *reinterpret_cast<const float4 *>(mine + i4);
      x[i4] = q.x;
      x[i4 + 1] = q.y;
      x[i4 + 2] = q.z;
      x[i4 + 3] = q.w;
    }
  }

  // 1. the pivot, from the block's smallest and largest pattern: count(pattern < lo) <= n0 <= count(pattern <= hi) throughout; the n0
  //    smallest are the values below lo and, by count, values equal to it
  uint32_t lo = __float_as_uint(x[0]), hi = lo;
#pragma unroll
  for (int i = 1; i < B; i++) {
    lo = min(lo, __float_as_uint(x[i]));
    hi = max(hi, __float_as_uint(x[i]));
  }
  lo = (uint32_t)group_reduce((int)lo, G, [](int a, int b) { return (int)min((uint32_t)a, (uint32_t)b); });
  hi = (uint32_t)group_reduce((int)hi, G, [](int a, int b) { return (int)max((uint32_t)a, (uint32_t)b); });
  while (__ballot(lo < hi) != 0) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    // the sign of mid - pattern is "above the pivot": 32 of them are gathered in a word with one shift-in each, then counted
    uint32_t above[(B + 31) / 32] = {};
#pragma unroll
    for (int i = 0; i < B; i++) above[i / 32] = __builtin_amdgcn_alignbit(above[i / 32], mid - __float_as_uint(x[i]), 31);
    int c = B;
#pragma unroll
    for (int w = 0; w < (B + 31) / 32; w++) c -= __popc(above[w]);
    c = group_sum(c, G);
    if (lo < hi) {
      if (c == p.n0) lo = hi = mid + 1;
      else if (c > p.n0) hi = mid;
      else lo = mid + 1;
    }
  }
  int n = p.n0;
  double C;
  {
    int c = 0;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < B; i++) {
      const int below = (int)(__float_as_uint(x[i]) - lo) >> 31;      // all ones where the pattern is below lo
      c -= below;
      s[i & 3] += (double)__uint_as_float(__float_as_uint(x[i]) & (uint32_t)below);
    }
    c = group_sum(c, G);
    C = group_sum((s[0] + s[1]) + (s[2] + s[3]), G);
    if (c < n) C += (double)(n - c) * (double)__uint_as_float(lo);
  }

  // 2. the floor: n bins with the sum C so far; every value with x n <= t_cme C is taken, until none is added
  const double t_cme = (double)p.t_cme;
  bool open = n < M;
  while (__ballot(open) != 0) {
    const uint32_t top = cut(t_cme * C, (double)n);
    int c = B;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < B; i++) {
      const int out = (int)(top - __float_as_uint(x[i])) >> 31;       // all ones where the pattern is above top
      c += out;
      s[i & 3] += (double)__uint_as_float(__float_as_uint(x[i]) & ~(uint32_t)out);
    }
    c = group_sum(c, G);
    const double sum = group_sum((s[0] + s[1]) + (s[2] + s[3]), G);
    if (open) {
      if (c > n) {
        n = c;
        C = sum;
        open = n < M;
      } else {
        open = false;
      }
    }
  }
  const float floor_b = (float)(C / (double)n);

  // 3. the two masks
  uint64_t lw = 0, up = 0;
  {
    const uint32_t cut_l = cut((double)p.t_lower * C, (double)n), cut_u = cut((double)p.t_upper * C, (double)n);
    // the sign of cut - pattern is the mask bit; from the last bin down, 32 bins to a word, one shift-in each
    uint32_t lw_w[2] = {0, 0}, up_w[2] = {0, 0};
#pragma unroll
    for (int i = B - 1; i >= 0; i--) {
      lw_w[i / 32] = __builtin_amdgcn_alignbit(lw_w[i / 32], cut_l - __float_as_uint(x[i]), 31);
      up_w[i / 32] = __builtin_amdgcn_alignbit(up_w[i / 32], cut_u - __float_as_uint(x[i]), 31);
    }
    lw = (uint64_t)lw_w[0] | ((uint64_t)lw_w[1] << 32);
    up = ((uint64_t)up_w[0] | ((uint64_t)up_w[1] << 32)) & lw;
  }

  // 4. clusters.  The run at the lane's low edge (head) and the one at its high edge (tail); a lane of ones is both at once.
  const uint64_t tops = __ballot((lw >> (B - 1)) & 1), lows = __ballot(lw & 1), full = __ballot(lw == PM);
  const uint64_t link = tops & rotr64(lows, 1);          // bit l: a run goes on from lane l into lane l + 1
  const uint64_t link_in = rotl64(link, 1);              // bit l: ... from lane l - 1 into lane l
  const uint64_t head = lw & ~(lw + 1);
  const int lead = clz64(~(lw << (64 - B)));
  const uint64_t tail = PM & ~low_bits(B - (lead < B ? lead : B));
  // carried upwards out of lane l: its tail holds an upper bin, or it is all ones and passes on what came in; and downwards likewise
  const uint64_t from_below = rotl64(carry_chain<true>(link & __ballot((up & tail) != 0), link & full), 1);
  const uint64_t from_above = rotr64(carry_chain<false>(link_in & __ballot((up & head) != 0), link_in & full), 1);
  const uint64_t seeds = up | ((from_below >> l) & 1) | (((from_above >> l) & 1) << (B - 1));
  const uint64_t det = flood_up(lw, seeds) | __brevll(flood_up(__brevll(lw), __brevll(seeds)));
  const uint64_t out = det | om;

  if (p.mask != nullptr) {
    uint32_t *mw = p.mask + e * (N / 32);
    if constexpr (B == 64) {
      reinterpret_cast<uint2 *>(mw)[l] = make_uint2((uint32_t)out, (uint32_t)(out >> 32));
    } else if constexpr (B == 32) {
      mw[l] = (uint32_t)out;
    } else {
      constexpr int R = 32 / B;                          // lanes to a mask word
      uint32_t w = (uint32_t)out << ((l % R) * B);
#pragma unroll
      for (int s = 1; s < R; s *= 2) w |= __shfl_xor(w, s, 64);
      if (l % R == 0) mw[l / R] = w;
    }
  }
  const bool leader = l % G == 0;
  if (p.floor != nullptr && leader) p.floor[e * p.n_blocks + l / G] = floor_b;

  if (p.rows != nullptr) {
    const uint64_t det_tops = __ballot((det >> (B - 1)) & 1);
    int n_lower = __popcll(lw), n_upper = __popcll(up), n_out = __popcll(out), n_clean = leader ? n : 0;
    int runs = run_starts<B>(lw, (tops >> ((l - 1) & 63)) & 1), kept = run_starts<B>(det, (det_tops >> ((l - 1) & 63)) & 1);
    float fmin = floor_b, fmax = floor_b;
#pragma unroll
    for (int s = 32; s > 0; s /= 2) {
      n_lower += __shfl_xor(n_lower, s, 64);
      n_upper += __shfl_xor(n_upper, s, 64);
      n_out += __shfl_xor(n_out, s, 64);
      n_clean += __shfl_xor(n_clean, s, 64);
      runs += __shfl_xor(runs, s, 64);
      kept += __shfl_xor(kept, s, 64);
      fmin = fminf(fmin, __shfl_xor(fmin, s, 64));
      fmax = fmaxf(fmax, __shfl_xor(fmax, s, 64));
    }
    // a circle of ones has no start: it is one run
    if (runs == 0 && n_lower > 0) runs = 1;
    if (kept == 0 && n_upper > 0) kept = 1;
    if (l == 0) {
      int4 *dst = reinterpret_cast<int4 *>(p.rows + e);
      dst[0] = make_int4(n_lower, n_upper, n_out, kept);
      dst[1] = make_int4(runs - kept, n_clean, __float_as_int(fmin), __float_as_int(fmax));
    }
  }
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_lad_device: ") + why); }

template <int B>
hipError_t launch(const LadParams &p, unsigned n, hipStream_t stream) {
  hipLaunchKernelGGL(lad_kernel<B>, dim3(n), dim3(64), 0, stream, p);
  return hipGetLastError();
}

}  // namespace
}  // namespace crn

int crn_lad_device(crn_handle *h, const float *d_spectrum, int64_t n_epochs, const crn_lad_params *params, const uint32_t *d_or_mask,
                   uint32_t *d_bin_mask, crn_lad_row *d_rows, float *d_floor, void *stream) {
  static_assert(sizeof(crn_lad_params) == 32 && sizeof(crn_lad_row) == 32, "include/crn_sense.h");
  if (!h || !params || !d_spectrum) return crn::refuse("null handle / params / spectrum");
  const crn_lad_params &q = *params;
  if (!d_bin_mask && !d_rows && !d_floor) return crn::refuse("no output: d_bin_mask, d_rows and d_floor are all null");
  if (n_epochs < 0) return crn::refuse("n_epochs < 0");
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  if ((q.n_blocks != 1 && q.n_blocks != 2 && q.n_blocks != 4 && q.n_blocks != 8) || n / q.n_blocks < 256)
    return crn::refuse("n_blocks must be 1, 2, 4 or 8 with fft_len / n_blocks >= 256");
  if (q.init_percent < 1 || q.init_percent > 50) return crn::refuse("init_percent must be in 1..50");
  if (!std::isfinite(q.t_cme) || !(q.t_cme > 0.0f)) return crn::refuse("t_cme must be finite and > 0");
  if (!std::isfinite(q.t_lower) || !(q.t_lower > 0.0f) || !std::isfinite(q.t_upper) || !(q.t_upper > 0.0f))
    return crn::refuse("t_lower and t_upper must be finite and > 0");
  if (q.t_lower > q.t_upper) return crn::refuse("t_lower > t_upper");
  for (int r : q.reserved)
    if (r != 0) return crn::refuse("reserved must be 0");
  if (crn::misaligned(d_spectrum, 16) || crn::misaligned(d_rows, 16)) return crn::refuse("d_spectrum and d_rows must be 16-byte aligned");
  if (crn::misaligned(d_or_mask, 8) || crn::misaligned(d_bin_mask, 8)) return crn::refuse("d_or_mask and d_bin_mask must be 8-byte aligned");
  if (crn::misaligned(d_floor, 4)) return crn::refuse("d_floor must be 4-byte aligned");
  if (n_epochs == 0) return CRN_OK;

  const int m = n / q.n_blocks, n0 = m * q.init_percent / 100;
  crn::LadParams p{d_spectrum, d_or_mask, d_bin_mask, d_rows, d_floor, 0, q.n_blocks, n0 < 1 ? 1 : n0, q.t_cme, q.t_lower, q.t_upper};
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  err = crn::in_grids(err, n_epochs, [&](int64_t first, unsigned cnt) {
    p.first = first;
    return n == 512 ? crn::launch<8>(p, cnt, st) : n == 1024 ? crn::launch<16>(p, cnt, st) : n == 2048 ? crn::launch<32>(p, cnt, st) : crn::launch<64>(p, cnt, st);
  });
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_lad_device: ") + hipGetErrorString(err));
  return CRN_OK;
}
