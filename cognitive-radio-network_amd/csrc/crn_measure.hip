// crn_measure.hip — the segment stage's second half (crn_measure_device, include/crn_sense.h): for every stored segment of an epoch the
// occupied bandwidth (the span that leaves tail_ppm of the net power outside on each side), the x-dB bandwidth (the outermost bins above
// xdb_ratio x the net peak), how many bins lie above that line, the net power and the crest (peak over mean of the net bins).  The net
// bins are turned into integers once (q = trunc(Q 2^(30 - e)), e the binary exponent of the record's peak_power), so every sum is an
// integer sum and the result does not depend on the order of the additions.
//
// Mapping: one workgroup of four waves per epoch at every fft_len (one instantiation).
//   1. the row is read once with coalesced float4 loads into LDS, unpadded; together with it lane j of wave v loads lo, width and
//      peak_power of slot v + 4 j (its own array's slots only) and every thread the epoch's header: one wait for memory per epoch;
//   2. wave v takes the stored slots v, v + 4, ...; the record of round j is broadcast from lane j;
//   3. one pass over the segment, 64 bins at a time, lane l at offset c 64 + l (consecutive LDS words: no bank conflict): the lane keeps
//      its maximum; the bins above the x-dB line are a ballot, counted and placed in scalar registers; the chunk's integers are add
//      scanned over the wave and the total is kept by lane c (a segment has at most 64 chunks);
//   4. an add scan over the chunk totals gives S0 and, by ballot, the chunk in which the running total passes T and the one in which it
//      reaches S0 - T; only those chunks are read again and scanned for the bin, and not even those where the lanes still hold the
//      chunk's scan (a segment of up to 64 bins, the common case, is scanned once);
//   5. lane j keeps the record of round j; at the end every lane stores its slot, zeros where nothing was measured or stored.
// No lane walks a segment; the rounds of a wave are bounded by max_segments / 4 and the chunks of a round by fft_len / 64.  Every row
// index is masked with fft_len - 1, every count clamped: whatever the two input arrays hold, the kernel reads its own row and its own
// max_segments records and writes its own max_segments slots.  No scratch memory, no atomics, plain vector stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_segments.h"

namespace crn {
namespace {

constexpr int WAVES = 4;   // waves of an epoch's workgroup: they share the row and deal the slots

struct MeasureParams {
  const float *spectrum;             // [n_epochs][N]
  const crn_segment_epoch *epochs;   // [n_epochs]
  const crn_segment *segments;       // [n_epochs][max_segments]
  crn_measure *measures;             // [n_epochs][max_segments]
  long long first;                   // epoch of workgroup 0
  int N, max_segments, tail_ppm, subtract;
  float ratio;
};

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int s = 32; s > 0; s /= 2) {
    const int u = __shfl_xor(v, s, 64);
    v = u > v ? u : v;
  }
  return v;
}
// inclusive add scan over the lanes
__device__ __forceinline__ long long wave_scan(long long v, int l) {
#pragma unroll
  for (int s = 1; s < 64; s *= 2) {
    const long long u = __shfl_up(v, s, 64);
    if (l >= s) v += u;
  }
  return v;
}

// one segment as a wave sees it
struct Span {
  const float *row;
  int mask, lo, w;   // N - 1; the record's lo and width, both checked
  float nm;
  double scale;      // 2^(30 - e)
  // Q of offset i, 0 beyond the segment (which is neither counted nor above any line)
  __device__ __forceinline__ float net(int i) const { return i < w ? __fsub_rn(row[(lo + i) & mask], nm) : 0.0f; }
  // the integer of a net bin: 0 unless Q > 0 (NaN included), at most 2^31 - 1; the product is exact in fp64
  __device__ __forceinline__ int quant(float Q) const {
    const double v = (double)Q * scale;
    return !(Q > 0.0f) ? 0 : v >= 2147483647.0 ? 0x7fffffff : (int)v;
  }
};

__global__ __launch_bounds__(64 * WAVES) void measure_kernel(const MeasureParams p) {
  __shared__ float4 row4[MAX_N / 4];
  const float *row = reinterpret_cast<const float *>(row4);
  const int tid = threadIdx.x, l = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, max_segments = p.max_segments;
  const long long e = p.first + blockIdx.x;

  // 1. every load of the epoch is issued before the first use
  constexpr int PASSES = MAX_N / 4 / (64 * WAVES);
  const float4 *src = reinterpret_cast<const float4 *>(p.spectrum + e * N);
  float4 part[PASSES];
#pragma unroll
  for (int i = 0; i < PASSES; i++) {
    const int k = tid + i * 64 * WAVES;
    part[i] = k < N / 4 ? src[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  const crn_segment_epoch head = p.epochs[e];
  const int slot = wv + WAVES * l;
  int my_lo = 0, my_width = 0;
  float my_peak = 0.0f;
  if (slot < max_segments) {
    const int4 *rec = reinterpret_cast<const int4 *>(p.segments + e * max_segments + slot);
    const int4 a = rec[0], b = rec[1];
    my_lo = a.x;
    my_width = a.y;
    my_peak = __int_as_float(b.y);
  }
#pragma unroll
  for (int i = 0; i < PASSES; i++) {
    const int k = tid + i * 64 * WAVES;
    if (k < N / 4) row4[k] = part[i];
  }
  __syncthreads();

  const int n_stored = head.n_stored < 0 ? 0 : head.n_stored > max_segments ? max_segments : head.n_stored;
  const float nm = p.subtract && finite_bits(head.noise_mean) && head.noise_mean > 0.0f ? head.noise_mean : 0.0f;
  const int rounds = n_stored > wv ? (n_stored - wv + WAVES - 1) / WAVES : 0;   // at most 64
  int4 out_a = make_int4(0, 0, 0, 0), out_b = make_int4(0, 0, 0, 0);

  // 2. the wave's slots
  for (int j = 0; j < rounds; j++) {
    Span g;
    g.row = row;
    g.mask = N - 1;
    g.nm = nm;
    g.lo = __builtin_amdgcn_readlane(my_lo, j);
    g.w = __builtin_amdgcn_readlane(my_width, j);
    const float peak = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_peak), j));
    const float pq = __fsub_rn(peak, nm);
    if (g.lo < 0 || g.lo >= N || g.w < 1 || g.w > N || !finite_bits(peak) || !(peak > 0.0f) || !(pq > 0.0f)) continue;
    // 2^ex <= peak < 2^(ex + 1): -149 .. 127
    const uint32_t pb = __float_as_uint(peak);
    const int ex = (pb >> 23) != 0 ? (int)(pb >> 23) - 127 : (31 - __clz((int)pb)) - 149;
    g.scale = __longlong_as_double((long long)(1023 + 30 - ex) << 52);
    const float thr = __fmul_rn(p.ratio, pq);

    // 3. one pass; the bins above the line are a ballot, counted and placed in scalar registers
    const int chunks = (g.w + 63) >> 6;   // at most 64
    long long my_total = 0, total = 0, incl = 0;
    int q = 0, mx = 0, n_above = 0, xdb_lo = 0, xdb_last = -1;
    for (int c = 0; c < chunks; c++) {
      const float Q = g.net(c * 64 + l);
      q = g.quant(Q);
      mx = q > mx ? q : mx;
      const unsigned long long above = __ballot(Q > thr);
      if (above != 0) {
        if (n_above == 0) xdb_lo = c * 64 + __builtin_ctzll(above);
        xdb_last = c * 64 + 63 - __builtin_clzll(above);
        n_above += __popcll(above);
      }
      incl = wave_scan((long long)q, l);
      total = __shfl(incl, 63, 64);
      if (l == c) my_total = total;
    }
    int at = chunks - 1;                  // the chunk whose q and scan the lanes hold

    // 4. the crossings; a segment of one chunk, the common case, is done with the scan it has
    const long long run = chunks > 1 ? wave_scan(my_total, l) : total;   // the running total behind chunk l
    const long long S0 = chunks > 1 ? __shfl(run, 63, 64) : total;
    if (S0 == 0) continue;
    const long long T = S0 * p.tail_ppm / 1000000, U = S0 - T;   // 0 <= T < S0 / 2
    const long long before = run - my_total;
    const int c_lo = __builtin_ctzll(__ballot(run > T));                        // run of lane 63 is S0 > T
    const int c_hi = 63 - __builtin_clzll(__ballot(before < U && l < chunks));  // lane 0: 0 < U
    auto rescan = [&](int c) {
      if (c == at) return;
      q = g.quant(g.net(c * 64 + l));
      incl = wave_scan((long long)q, l);
      at = c;
    };
    rescan(c_lo);
    // the chunk's last lane holds run of c_lo > T
    const int obw_lo = c_lo * 64 + __builtin_ctzll(__ballot(incl + __shfl(before, c_lo, 64) > T));
    rescan(c_hi);
    // the largest i with C[i - 1] < U; lane 0 of the chunk holds `before` of c_hi < U and lies inside the segment
    const int obw_last = c_hi * 64 + 63 - __builtin_clzll(__ballot(incl - q + __shfl(before, c_hi, 64) < U && c_hi * 64 + l < g.w));

    mx = wave_max(mx);
    const float net_power = (float)((double)S0 * __longlong_as_double((long long)(1023 + ex - 30) << 52));
    const float crest = (float)((double)mx * (double)g.w / (double)S0);
    // 5. lane j keeps the round's record
    if (l == j) {
      out_a = make_int4(obw_lo, obw_last - obw_lo + 1, xdb_lo, xdb_last - xdb_lo + 1);
      out_b = make_int4(n_above, __float_as_int(net_power), __float_as_int(crest), 0);
    }
  }
  if (slot < max_segments) {
    int4 *dst = reinterpret_cast<int4 *>(p.measures + e * max_segments + slot);
    dst[0] = out_a;
    dst[1] = out_b;
  }
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_measure_device: ") + why); }

}  // namespace
}  // namespace crn

int crn_measure_device(crn_handle *h, const float *d_spectrum, int64_t n_epochs, const crn_measure_params *params,
                       const crn_segment_epoch *d_epochs, const crn_segment *d_segments, crn_measure *d_measures, void *stream) {
  static_assert(sizeof(crn_measure_params) == 32 && sizeof(crn_measure) == 32 && sizeof(crn_segment) == 32 && sizeof(crn_segment_epoch) == 16,
                "include/crn_sense.h");
  static_assert(crn::MAX_N / 4 % (64 * crn::WAVES) == 0 && 64 * crn::WAVES >= 256, "the row's passes; a lane per slot of a wave");
  if (!h || !params || !d_spectrum || !d_epochs || !d_segments || !d_measures)
    return crn::refuse("null handle / params / spectrum / epochs / segments / measures");
  const crn_measure_params &q = *params;
  if (n_epochs < 0) return crn::refuse("n_epochs < 0");
  if (q.max_segments < 1 || q.max_segments > 256) return crn::refuse("max_segments must be in 1..256");
  if (q.tail_ppm < 0 || q.tail_ppm > 499999) return crn::refuse("tail_ppm must be in 0..499999");
  if (!std::isfinite(q.xdb_ratio) || !(q.xdb_ratio >= 0.0f) || !(q.xdb_ratio < 1.0f)) return crn::refuse("xdb_ratio must be finite and in [0, 1)");
  if (q.subtract_noise != 0 && q.subtract_noise != 1) return crn::refuse("subtract_noise must be 0 or 1");
  if (q.reserved[0] != 0 || q.reserved[1] != 0 || q.reserved[2] != 0 || q.reserved[3] != 0) return crn::refuse("reserved must be 0");
  if (crn::misaligned(d_spectrum, 16) || crn::misaligned(d_epochs, 16) || crn::misaligned(d_segments, 16) || crn::misaligned(d_measures, 16))
    return crn::refuse("d_spectrum, d_epochs, d_segments and d_measures must be 16-byte aligned");
  if (n_epochs == 0) return CRN_OK;
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  crn::MeasureParams p{d_spectrum, d_epochs, d_segments, d_measures, 0, n, q.max_segments, q.tail_ppm, q.subtract_noise, q.xdb_ratio};
  err = crn::in_grids(err, n_epochs, [&](int64_t first, unsigned cnt) {
    p.first = first;
    hipLaunchKernelGGL(crn::measure_kernel, dim3(cnt), dim3(64 * crn::WAVES), 0, st, p);
    return hipGetLastError();
  });
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_measure_device: ") + hipGetErrorString(err));
  return CRN_OK;
}
