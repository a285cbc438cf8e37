// crn_resample.hip — extracted streams at k samples per symbol (crn_resample_device, include/crn_sense.h): an arbitrary-ratio polyphase
// resampler with a fine mixer behind it.  Ratio and offset are per row, read from device memory; the carry is the caller's.
//
// Mapping: two launches, one instantiation per T in {8, 16, 32}, one wave per workgroup.
//   resample_kernel<T>  a workgroup takes one row and one tile of 256 consecutive outputs.  It reads the row record and the head of the
//      state, finds n and w (step 1), and stages the tile's input span into LDS once: at most 255 * 4 + T + 1 samples (rho = 4), from an
//      even sample of d_in on, 16-byte loads wherever both samples of a pair lie inside the row; samples below 0 come from the state's
//      history, through the same staging, so an output's arithmetic does not know where the call began.  A lane owns two adjacent
//      outputs, in two rounds of 128; per output it reads the two table rows of its phi through the cache (16-byte loads; the table is
//      8 KB at 16 x 128 and 33 KB at 32 x 256, and every wave on the device reads the same one), builds each coefficient as
//      fma(mu, h1 - h0, h0), and sums k = 0 .. T - 1 in that order from LDS.  The mixer factor comes from the integer phase: the quadrant
//      is exact, the remainder in +-pi / 4 goes through two short polynomials.  Stores are 16 bytes where the output row is so aligned
//      (out_cap even or the row even), 8 bytes otherwise; samples at and above w are written as zeros.
//   carry_kernel<T>     one wave per row, after the first launch has finished: step 6.  No wave of the first launch writes a state and
//      the waves of the second read and write only their own, so no word is read by one wave and written by another in one launch.
// Every index comes from the launch geometry and the arithmetic of steps 1 and 2; the LDS index of an output is clamped into the staged
// span.  No atomics, no scratch, one writer per word, nothing depends on timing.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_segments.h"

namespace crn {
namespace {

constexpr int TILE = 256;              // outputs of a workgroup
constexpr uint64_t STEP_MIN = 1ull << 30, STEP_MAX = 1ull << 34;

struct ResampleParams {
  const float2 *in;                    // [n_rows][in_len]
  const crn_resample_row *rows;        // [n_rows]
  const float *taps;                   // [P + 1][T]
  crn_resample_state *state;           // [n_rows]
  float2 *out;                         // [n_rows][out_cap]
  long long first_group;               // (row, tile) of workgroup 0
  int in_len, out_cap, tiles, shift;   // tiles to a row; shift = s = 32 - log2 P
  int first;
};

// what steps 1 and 6 need of a row: the record, and the state's head as the definition reads it
struct RowHead {
  uint64_t step, pos;
  uint32_t phase, dphi;
  bool live, empty;
};

template <int T>
__device__ __forceinline__ RowHead row_head(const ResampleParams &p, long long r) {
  RowHead hd;
  const int4 rec = *reinterpret_cast<const int4 *>(p.rows + r);
  hd.step = (uint64_t)(uint32_t)rec.x | ((uint64_t)(uint32_t)rec.y << 32);
  hd.dphi = (uint32_t)rec.z;
  hd.live = hd.step >= STEP_MIN && hd.step <= STEP_MAX;
  const int4 st = *reinterpret_cast<const int4 *>(p.state + r);
  hd.empty = p.first != 0 || st.w != T;
  hd.pos = hd.empty ? 0 : (uint64_t)(uint32_t)st.x | ((uint64_t)(uint32_t)st.y << 32);
  hd.phase = hd.empty ? 0 : (uint32_t)st.z;
  return hd;
}

// step 1: the outputs whose position falls inside in_len samples; at most 2^26
__device__ __forceinline__ uint32_t count(uint64_t pos, uint64_t step, int in_len) {
  const uint64_t L = (uint64_t)in_len << 32;
  return pos >= L ? 0u : (uint32_t)((L - 1 - pos) / step) + 1u;
}

// e^(+j 2 pi theta / 2^32): the quadrant is exact; the remainder r in [-2^29, 2^29) becomes an angle in [-pi / 4, pi / 4) with two
// roundings, and sine and cosine there are short polynomials (the coefficients of the Cephes single-precision kernels)
__device__ __forceinline__ float2 unit_turn(uint32_t theta) {
  const uint32_t q = (theta + (1u << 29)) >> 30;
  const int32_t r = (int32_t)(theta - (q << 30));
  const float a = (float)r * 1.4629180792671596e-9f;   // 2 pi / 2^32
  const float z = a * a;
  const float s = fmaf(a * z, fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), a);
  const float c = fmaf(z * z, fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f), fmaf(z, -0.5f, 1.0f));
  const float cr = q & 1 ? -s : c, ci = q & 1 ? c : s;   // quadrants: (c, s), (-s, c), (-c, -s), (s, -c)
  return make_float2(q & 2 ? -cr : cr, q & 2 ? -ci : ci);
}

template <int T>
__global__ __launch_bounds__(64) void resample_kernel(const ResampleParams p) {
  constexpr int SPAN = 4 * TILE + T;   // samples staged: 255 * 4 + 1 of the positions, T - 1 before them, one for the even start
  __shared__ float2 xs[SPAN];
  const int lane = threadIdx.x;
  const long long g = p.first_group + blockIdx.x;   // < n_rows tiles
  const long long r = g / p.tiles;
  const int u0 = (int)(g - r * p.tiles) * TILE;     // < out_cap
  const int u_end = u0 + TILE < p.out_cap ? u0 + TILE : p.out_cap;
  float2 *const row = p.out + r * p.out_cap;
  const bool wide = ((r * p.out_cap) & 1) == 0;     // row + an even u is 16-byte aligned
  const RowHead hd = row_head<T>(p, r);
  const uint32_t n = hd.live ? count(hd.pos, hd.step, p.in_len) : 0u;
  const int w = n < (uint32_t)p.out_cap ? (int)n : p.out_cap;

  if (u0 >= w) {   // the whole workgroup: nothing but zeros
    for (int u = u0 + 2 * lane; u < u_end; u += 128) {
      if (wide && u + 1 < u_end) {
        *reinterpret_cast<float4 *>(row + u) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      } else {
        row[u] = make_float2(0.0f, 0.0f);
        if (u + 1 < u_end) row[u + 1] = make_float2(0.0f, 0.0f);
      }
    }
    return;
  }

  // the span of the tile: from T - 1 samples before its first position to its last position, begun at an even sample of d_in
  const float2 *const x = p.in + r * p.in_len;
  const int u_last = (u0 + TILE < w ? u0 + TILE : w) - 1;
  const int j_first = (int)((hd.pos + (uint64_t)u0 * hd.step) >> 32);        // 0 .. in_len - 1
  const int j_last = (int)((hd.pos + (uint64_t)u_last * hd.step) >> 32);     // j_first .. in_len - 1, at most j_first + 1020
  int start = j_first - (T - 1);
  start -= (start ^ (int)(r * p.in_len)) & 1;
  const float2 *const hist = reinterpret_cast<const float2 *>(p.state[r].hist);
  for (int q = lane; q < SPAN / 2; q += 64) {
    const int i = start + 2 * q;   // (r in_len + i) is even
    if (i > j_last) break;
    float2 a = make_float2(0.0f, 0.0f), b = a;
    if (i >= 0 && i + 1 < p.in_len) {
      const float4 v = *reinterpret_cast<const float4 *>(x + i);
      a = make_float2(v.x, v.y);
      b = make_float2(v.z, v.w);
    } else {
      if (i >= 0 && i < p.in_len) a = x[i];
      else if (i >= -(T - 1) && i < 0 && !hd.empty) a = hist[T - 1 + i];
      if (i + 1 >= 0 && i + 1 < p.in_len) b = x[i + 1];
      else if (i + 1 >= -(T - 1) && i + 1 < 0 && !hd.empty) b = hist[T + i];
    }
    xs[2 * q] = a;
    xs[2 * q + 1] = b;
  }
  __syncthreads();

#pragma unroll 1
  for (int round = 0; round < 2; round++) {
    const int ua = u0 + round * 128 + 2 * lane;
    if (ua >= u_end) continue;
    float zr[2], zi[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int u = ua + e;
      zr[e] = 0.0f;
      zi[e] = 0.0f;
      if (u < w) {
        const uint64_t pp = hd.pos + (uint64_t)u * hd.step;
        const uint32_t f = (uint32_t)pp;
        const int phi = (int)(f >> p.shift);                                  // 0 .. P - 1
        const uint32_t low = f & ((1u << p.shift) - 1u);
        const float mu = p.shift > 24 ? (float)(low >> (p.shift - 24)) * 5.9604644775390625e-8f : (float)low * 5.9604644775390625e-8f;
        int jb = (int)(pp >> 32) - start;                                     // the place of x[j] in the span
        jb = jb < T - 1 ? T - 1 : (jb > SPAN - 1 ? SPAN - 1 : jb);
        const float4 *const h0 = reinterpret_cast<const float4 *>(p.taps + (long long)phi * T);
        const float4 *const h1 = h0 + T / 4;
        float yr = 0.0f, yi = 0.0f;
#pragma unroll
        for (int k4 = 0; k4 < T / 4; k4++) {
          const float4 a = h0[k4], b = h1[k4];
          const float c[4] = {fmaf(mu, b.x - a.x, a.x), fmaf(mu, b.y - a.y, a.y), fmaf(mu, b.z - a.z, a.z), fmaf(mu, b.w - a.w, a.w)};
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const float2 v = xs[jb - 4 * k4 - k];
            yr = fmaf(c[k], v.x, yr);
            yi = fmaf(c[k], v.y, yi);
          }
        }
        const float2 m = unit_turn(hd.phase + (uint32_t)u * hd.dphi);
        zr[e] = fmaf(yr, m.x, -(yi * m.y));
        zi[e] = fmaf(yr, m.y, yi * m.x);
      }
    }
    if (wide && ua + 1 < u_end) {
      *reinterpret_cast<float4 *>(row + ua) = make_float4(zr[0], zi[0], zr[1], zi[1]);
    } else {
      row[ua] = make_float2(zr[0], zi[0]);
      if (ua + 1 < u_end) row[ua + 1] = make_float2(zr[1], zi[1]);
    }
  }
}

// step 6, one wave per row: everything is read before anything is written
template <int T>
__global__ __launch_bounds__(64) void carry_kernel(const ResampleParams p) {
  const int lane = threadIdx.x;
  const long long r = p.first_group + blockIdx.x;
  const RowHead hd = row_head<T>(p, r);
  crn_resample_state *const st = p.state + r;
  if (!hd.live) {
    if (lane == 0) st->last_n_out = 0;
    return;
  }
  const uint32_t n = count(hd.pos, hd.step, p.in_len);
  const uint32_t w = n < (uint32_t)p.out_cap ? n : (uint32_t)p.out_cap;
  const uint64_t L = (uint64_t)p.in_len << 32;
  float2 *const hist = reinterpret_cast<float2 *>(st->hist);
  // hist[lane] <- sample in_len - (T - 1) + lane of (history ++ row); entries from T - 1 on are 0
  float2 v = make_float2(0.0f, 0.0f);
  if (lane < T - 1) {
    const long long i = (long long)p.in_len - (T - 1) + lane;
    if (i >= 0) v = p.in[r * p.in_len + i];
    else if (!hd.empty) v = hist[T - 1 + i];
  }
  int64_t n_in = 0, n_out = 0, n_dropped = 0;
  if (!hd.empty) {
    n_in = st->n_in;
    n_out = st->n_out;
    n_dropped = st->n_dropped;
  }
  __syncthreads();
  if (lane < 32) hist[lane] = v;
  if (lane == 0) {
    st->pos = hd.pos + (uint64_t)n * hd.step - L;   // mod 2^64: right also for n = 0, where pos >= L
    st->phase = hd.phase + n * hd.dphi;
    st->taps = T;
    st->n_in = (int64_t)((uint64_t)(n_in < 0 ? 0 : n_in) + (uint64_t)p.in_len);
    st->n_out = (int64_t)((uint64_t)(n_out < 0 ? 0 : n_out) + w);
    st->n_dropped = (int64_t)((uint64_t)(n_dropped < 0 ? 0 : n_dropped) + (n - w));
    st->last_n_out = (int32_t)w;
#pragma unroll
    for (int i = 0; i < 5; i++) st->reserved[i] = 0;
  }
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_resample_device: ") + why); }

template <int T>
hipError_t launch(hipError_t err, int64_t n_rows, ResampleParams p, hipStream_t st) {
  err = in_grids(err, n_rows * p.tiles, [&](int64_t first, unsigned cnt) {
    p.first_group = first;
    hipLaunchKernelGGL(resample_kernel<T>, dim3(cnt), dim3(64), 0, st, p);
    return hipGetLastError();
  });
  if (err != hipSuccess) return err;
  p.first_group = 0;
  hipLaunchKernelGGL(carry_kernel<T>, dim3((unsigned)n_rows), dim3(64), 0, st, p);
  return hipGetLastError();
}

}  // namespace
}  // namespace crn

int64_t crn_resample_state_bytes(int64_t n_rows) { return n_rows < 0 || n_rows > 65536 ? -1 : n_rows * (int64_t)sizeof(crn_resample_state); }

int crn_resample_device(crn_handle *h, const float *d_in, int32_t n_rows, const crn_resample_params *params, const crn_resample_row *d_rows,
                        const float *d_taps, crn_resample_state *d_state, float *d_out, void *stream) {
  static_assert(sizeof(crn_resample_params) == 32 && sizeof(crn_resample_row) == 16 && sizeof(crn_resample_state) == 320, "include/crn_sense.h");
  static_assert(offsetof(crn_resample_state, taps) == 12 && offsetof(crn_resample_state, hist) == 64, "include/crn_sense.h");
  if (!h || !params || !d_in || !d_rows || !d_taps || !d_state || !d_out) return crn::refuse("null handle / params / in / rows / taps / state / out");
  const crn_resample_params &q = *params;
  if (q.taps != 8 && q.taps != 16 && q.taps != 32) return crn::refuse("taps must be 8, 16 or 32");
  if (q.phases != 32 && q.phases != 64 && q.phases != 128 && q.phases != 256) return crn::refuse("phases must be 32, 64, 128 or 256");
  if (q.in_len < 1 || q.in_len > (1 << 24)) return crn::refuse("in_len must be in 1..2^24");
  if (q.out_cap < 1 || q.out_cap > (1 << 26)) return crn::refuse("out_cap must be in 1..2^26");
  if (n_rows < 0 || n_rows > 65536) return crn::refuse("n_rows must be in 0..65536");
  for (int i = 0; i < 3; i++)
    if (q.reserved[i] != 0) return crn::refuse("reserved must be 0");
  if (crn::misaligned(d_in, 16) || crn::misaligned(d_rows, 16) || crn::misaligned(d_taps, 16) || crn::misaligned(d_state, 16) || crn::misaligned(d_out, 16))
    return crn::refuse("d_in, d_rows, d_taps, d_state and d_out must be 16-byte aligned");
  if (n_rows == 0) return CRN_OK;
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int log2p = 5;
  while ((1 << log2p) < q.phases) log2p++;
  const crn::ResampleParams p{reinterpret_cast<const float2 *>(d_in), d_rows, d_taps, d_state, reinterpret_cast<float2 *>(d_out), 0,
                              q.in_len, q.out_cap, (q.out_cap + crn::TILE - 1) / crn::TILE, 32 - log2p, q.first};
  switch (q.taps) {
    case 8: err = crn::launch<8>(err, n_rows, p, st); break;
    case 16: err = crn::launch<16>(err, n_rows, p, st); break;
    default: err = crn::launch<32>(err, n_rows, p, st); break;
  }
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_resample_device: ") + hipGetErrorString(err));
  return CRN_OK;
}
