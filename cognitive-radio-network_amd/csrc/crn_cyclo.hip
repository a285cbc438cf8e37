// crn_cyclo.hip — what a segment is, second part (crn_cyclo_device, include/crn_sense.h): for every stored segment of an epoch the
// spectral coherence S(a, q) between the components a bins apart, over the F frames of the epoch, for n_a separations a and the F
// fractional offsets q; the strongest cell and its two neighbours in a give the symbol rate of a digitally modulated carrier.
//
// Mapping: one workgroup of four waves per (epoch, slot), one instantiation per F in {8, 16, 32, 64}; an empty slot, or one whose
// segment is too narrow for any cell, zero-fills its record and its profile and leaves.
//   1. a lane owns a separation: lane l of chunk c has a = a_lo + 64 c + l (n_a <= 128: at most two chunks, taken in turn) and keeps the
//      F sums of its (a, q) cells in fp64 registers.  The pairs are walked in tiles of T offsets i; the four waves deal a tile's offsets.
//   2. a tile is staged once in LDS as [F][columns] complex: T + 2 columns from the first component's side (bin lo' + i, the same for
//      every lane: a broadcast read) and T + 66 from the second's (bin lo' + i + a: consecutive lanes, consecutive 8-byte words, no bank
//      conflict).  Both windows start on an even bin, so the frame rows are read with 16-byte loads, all issued before the first LDS
//      store; a window is taken modulo N and may run past the span (those columns are read and never used).  Every staged column is
//      divided by the root of its power P[k], once per tile.
//   3. per pair a lane forms the F products X_f[k'] conj(X_f[k]) from LDS, transforms them in registers (radix 2, decimation in
//      frequency, every index and twiddle factor a compile-time constant: no scratch), and adds rho = |C|^2 of the normalised columns to its F sums.
//   4. the sums of waves 1, 2, 3 are added to wave 0's in that order through the staging area; wave 0 forms S and z, writes the profile
//      rows, and picks the chunk's best cell by a wave reduction whose order is (z, then a, then q): nothing depends on timing.
//      The neighbours in a come from the adjacent lanes, across the chunk border from two rows kept in LDS.
// Every row index is masked with N - 1 and every count clamped, so whatever the two record arrays hold, a workgroup reads its own
// epoch's frames and its own record and writes its own slot.  No atomics, plain vector stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_segments.h"

namespace crn {
namespace {

constexpr int WAVES = 4;    // waves of a workgroup: they deal the offsets of a tile
constexpr int LANES = 64;   // separations of a chunk, one to a lane

struct CycloParams {
  const float *frames;               // [n_epochs][F][N] complex
  const crn_segment_epoch *epochs;   // [n_epochs]
  const crn_segment *segments;       // [n_epochs][max_segments]
  crn_cyclo *out;                    // [n_epochs][max_segments]
  float *profile;                    // [n_epochs][max_segments][n_a][F] or null
  long long first;                   // (epoch, slot) of workgroup 0
  int N, max_segments, a_lo, n_a, max_width, min_pairs;
  float z_min;
};

// the staging of one tile: T offsets, TL columns on the first component's side, TR on the second's (one more on either side so that a
// window can start on the even bin below, and TR a multiple of two)
template <int F>
struct Tile {
  static constexpr int T = F == 64 ? 16 : 32;
  static constexpr int TL = T + 2, TR = T + LANES + 2;
  static constexpr int PAIRS = (TL + TR) / 2;                                  // 16-byte loads per frame row
  static constexpr int PASSES = (F * PAIRS + 64 * WAVES - 1) / (64 * WAVES);   // ... per thread
  static_assert(F * LANES * 8 <= F * (TL + TR) * 8, "the waves' sums pass through the staging area");
};

// W_64^k = cos - j sin, k = 0 .. 31
__device__ constexpr float COS64[32] = {
    1.0f, 0.9951847195625305f, 0.9807852506637573f, 0.9569403529167175f, 0.9238795042037964f, 0.8819212913513184f, 0.8314695954322815f, 0.7730104327201843f,
    0.7071067690849304f, 0.6343932747840881f, 0.5555702447891235f, 0.4713967442512512f, 0.3826834261417389f, 0.290284663438797f, 0.19509032368659973f, 0.0980171412229538f,
    0.0f, -0.0980171412229538f, -0.19509032368659973f, -0.290284663438797f, -0.3826834261417389f, -0.4713967442512512f, -0.5555702447891235f, -0.6343932747840881f,
    -0.7071067690849304f, -0.7730104327201843f, -0.8314695954322815f, -0.8819212913513184f, -0.9238795042037964f, -0.9569403529167175f, -0.9807852506637573f, -0.9951847195625305f};
__device__ constexpr float SIN64[32] = {
    0.0f, 0.0980171412229538f, 0.19509032368659973f, 0.290284663438797f, 0.3826834261417389f, 0.4713967442512512f, 0.5555702447891235f, 0.6343932747840881f,
    0.7071067690849304f, 0.7730104327201843f, 0.8314695954322815f, 0.8819212913513184f, 0.9238795042037964f, 0.9569403529167175f, 0.9807852506637573f, 0.9951847195625305f,
    1.0f, 0.9951847195625305f, 0.9807852506637573f, 0.9569403529167175f, 0.9238795042037964f, 0.8819212913513184f, 0.8314695954322815f, 0.7730104327201843f,
    0.7071067690849304f, 0.6343932747840881f, 0.5555702447891235f, 0.4713967442512512f, 0.3826834261417389f, 0.290284663438797f, 0.19509032368659973f, 0.0980171412229538f};

// position p of the transform's output holds the coefficient of this index (F a power of two)
template <int F>
__device__ constexpr int bit_reversed(int p) {
  int q = 0;
  for (int b = 1; b < F; b *= 2, p /= 2) q = q * 2 + (p & 1);
  return q;
}

// the forward DFT of F values in place, output in bit-reversed order; every loop unrolls, every index is a constant
template <int F>
__device__ __forceinline__ void dft(float (&re)[F], float (&im)[F]) {
#pragma unroll
  for (int h = F / 2; h >= 1; h /= 2) {
#pragma unroll
    for (int b = 0; b < F; b += 2 * h) {
#pragma unroll
      for (int j = 0; j < h; j++) {
        const int k = j * (32 / h);   // W_(2h)^j = W_64^k
        const float ur = re[b + j], ui = im[b + j], tr = re[b + j + h], ti = im[b + j + h];
        re[b + j] = ur + tr;
        im[b + j] = ui + ti;
        const float dr = ur - tr, di = ui - ti;
        if (k == 0) {
          re[b + j + h] = dr;
          im[b + j + h] = di;
        } else if (k == 16) {   // -j
          re[b + j + h] = di;
          im[b + j + h] = -dr;
        } else {
          re[b + j + h] = dr * COS64[k] + di * SIN64[k];
          im[b + j + h] = di * COS64[k] - dr * SIN64[k];
        }
      }
    }
  }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// a chunk's best cell as the wave agrees on it: the largest z, then the smallest key = (a - a_lo) F + q
struct Best {
  float z;
  int key, have;
};
__device__ __forceinline__ Best wave_best(Best m) {
#pragma unroll
  for (int s = 32; s > 0; s /= 2) {
    const float oz = __shfl_xor(m.z, s, 64);
    const int okey = __shfl_xor(m.key, s, 64), ohave = __shfl_xor(m.have, s, 64);
    const bool take = ohave && (!m.have || oz > m.z || (oz == m.z && okey < m.key));
    m.z = take ? oz : m.z;
    m.key = take ? okey : m.key;
    m.have = take ? ohave : m.have;
  }
  return m;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int s = 32; s > 0; s /= 2) v += __shfl_xor(v, s, 64);
  return v;
}

template <int F>
__global__ __launch_bounds__(64 * WAVES) void cyclo_kernel(const CycloParams p) {
  using G = Tile<F>;
  constexpr int T = G::T, TL = G::TL, TR = G::TR;
  __shared__ float4 stage4[F * (TL + TR) / 2];   // [F][TL] then [F][TR] complex
  __shared__ float edge[2][2][F];                // S of the first and of the last lane of either chunk
  float2 *const colL = reinterpret_cast<float2 *>(stage4), *const colR = colL + F * TL;
  double *const pass = reinterpret_cast<double *>(stage4);   // [F][64], between the tiles and the pick

  const int tid = threadIdx.x, l = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = p.N, mask = N - 1, n_a = p.n_a, max_segments = p.max_segments;
  const long long g = p.first + blockIdx.x;   // < n_epochs max_segments
  const long long e = g / max_segments;
  const int slot = (int)(g - e * max_segments);

  // the record, clamped
  const int n_stored = clampi(p.epochs[e].n_stored, 0, max_segments);
  int w = 0, lo2 = 0;
  if (slot < n_stored) {
    const int4 rec = *reinterpret_cast<const int4 *>(p.segments + g);
    const int width = clampi(rec.y, 0, N);
    w = width < p.max_width ? width : p.max_width;
    lo2 = ((rec.x & mask) + (width - w) / 2) & mask;
  }
  // separations a_lo .. a_lo + n_t - 1 are tested: w - a >= min_pairs
  const int n_t = clampi(w - p.min_pairs - p.a_lo + 1, 0, n_a);
  int4 *const dst = reinterpret_cast<int4 *>(p.out + g);
  float4 *const prof4 = p.profile ? reinterpret_cast<float4 *>(p.profile + g * n_a * F) : nullptr;
  if (n_t == 0) {   // the whole workgroup
    if (tid < 2) dst[tid] = make_int4(0, 0, 0, 0);
    if (prof4)
      for (int i = tid; i < n_a * F / 4; i += 64 * WAVES) prof4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }

  const float2 *const rows = reinterpret_cast<const float2 *>(p.frames) + e * F * N;
  const int n_chunks = (n_a + LANES - 1) / LANES;
  // wave 0's running result
  Best best = {0.0f, 0, 0};
  int n_over = 0, best_pairs = 0;
  float stat = 0.0f, stat_lo = 0.0f, stat_hi = 0.0f;

  for (int c = 0; c < n_chunks; c++) {
    const int a0 = p.a_lo + c * LANES, idx = c * LANES + l, a = a0 + l;
    const bool tested = idx < n_t;
    const int np = w - a;             // pairs of this lane's separation; >= min_pairs >= 1 where tested
    const int mp = w - a0;            // ... of the chunk's first, the most
    const bool live = c * LANES < n_t;   // the chunk has a tested separation
    double acc[F];
#pragma unroll
    for (int q = 0; q < F; q++) acc[q] = 0.0;

    for (int i0 = 0; live && i0 < mp; i0 += T) {
      // 2. stage the tile: both windows start on the even bin at or below their first column
      const int sL = (lo2 + i0) & mask, sR = (lo2 + i0 + a0) & mask;
      const int offL = sL & 1, offR = sR & 1;
      float4 part[G::PASSES];
#pragma unroll
      for (int ps = 0; ps < G::PASSES; ps++) {
        const int it = tid + ps * 64 * WAVES;
        const int f = it / G::PAIRS, c2 = it - f * G::PAIRS;
        const int bin = c2 < TL / 2 ? (sL - offL + 2 * c2) & mask : (sR - offR + 2 * (c2 - TL / 2)) & mask;   // even, bin + 1 < N
        part[ps] = f < F ? *reinterpret_cast<const float4 *>(rows + (long long)f * N + bin) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
      __syncthreads();   // the tile before is read
#pragma unroll
      for (int ps = 0; ps < G::PASSES; ps++) {
        const int it = tid + ps * 64 * WAVES;
        const int f = it / G::PAIRS, c2 = it - f * G::PAIRS;
        if (f < F) stage4[c2 < TL / 2 ? (f * TL) / 2 + c2 : (F * TL + f * TR) / 2 + (c2 - TL / 2)] = part[ps];
      }
      __syncthreads();
      // every staged column is divided by sqrt(P) of that column, once: rho is then |sum of the products|^2 as it stands, and neither
      // P[k'] P[k] nor |C|^2 is formed where spectra far from 1 would take it out of the fp32 range.  A column of no power stays zero.
      if (tid < TL + TR) {
        float2 *col = tid < TL ? colL + tid : colR + (tid - TL);
        const int stride = tid < TL ? TL : TR;
        float s = 0.0f;
#pragma unroll 8
        for (int f = 0; f < F; f++) {
          const float2 x = col[f * stride];
          s += x.x * x.x + x.y * x.y;
        }
        const float sc = s > 0.0f ? 1.0f / sqrtf(s) : 0.0f;
#pragma unroll 8
        for (int f = 0; f < F; f++) {
          const float2 x = col[f * stride];
          col[f * stride] = make_float2(x.x * sc, x.y * sc);
        }
      }
      __syncthreads();

      // 3. the wave's offsets of the tile
      for (int t = wv; t < T && i0 + t < mp; t += WAVES) {
        const bool valid = tested && i0 + t < np;
        float re[F], im[F];
#pragma unroll
        for (int f = 0; f < F; f++) {
          const float2 x = colL[f * TL + offL + t], y = colR[f * TR + offR + t + l];
          re[f] = y.x * x.x + y.y * x.y;
          im[f] = y.y * x.x - y.x * x.y;
        }
        dft<F>(re, im);
#pragma unroll
        for (int pz = 0; pz < F; pz++) {
          const float rho = re[pz] * re[pz] + im[pz] * im[pz];
          acc[bit_reversed<F>(pz)] += valid ? (double)(rho < 1.0f ? rho : 1.0f) : 0.0;
        }
      }
    }

    // 4. waves 1, 2, 3 into wave 0, in that order
    for (int r = 1; live && r < WAVES; r++) {
      __syncthreads();
      if (wv == r) {
#pragma unroll
        for (int q = 0; q < F; q++) pass[q * LANES + l] = acc[q];
      }
      __syncthreads();
      if (wv == 0) {
#pragma unroll
        for (int q = 0; q < F; q++) acc[q] += pass[q * LANES + l];
      }
    }

    if (wv == 0) {
      const double scale = sqrt((double)(tested ? np : 1) * (double)(F + 1) / (double)(F - 1));
      float S[F];
      Best mine = {-INFINITY, idx * F, tested ? 1 : 0};
      int over = 0;
#pragma unroll
      for (int q = 0; q < F; q++) {
        S[q] = tested ? (float)(acc[q] / (double)np) : 0.0f;
        const float z = (float)(((double)F * (double)S[q] - 1.0) * scale);
        over += tested && z >= p.z_min ? 1 : 0;
        if (z > mine.z) {
          mine.z = z;
          mine.key = idx * F + q;
        }
      }
      if (prof4 && idx < n_a) {
#pragma unroll
        for (int q = 0; q < F; q += 4) prof4[(idx * F + q) / 4] = make_float4(S[q], S[q + 1], S[q + 2], S[q + 3]);
      }
      if (l == 0 || l == LANES - 1) {
#pragma unroll
        for (int q = 0; q < F; q++) edge[c][l == 0 ? 0 : 1][q] = S[q];
      }
      n_over += wave_sum(over);
      const Best cb = wave_best(mine);
      if (cb.have && (!best.have || cb.z > best.z)) {   // chunks come in rising a: a tie stays with the earlier
        best = cb;
        const int bl = cb.key / F - c * LANES, bq = cb.key % F;
        float sel = 0.0f;
#pragma unroll
        for (int q = 0; q < F; q++) sel = q == bq ? S[q] : sel;
        stat = __shfl(sel, bl, 64);
        stat_lo = __shfl(sel, bl > 0 ? bl - 1 : 0, 64);
        stat_hi = __shfl(sel, bl < LANES - 1 ? bl + 1 : LANES - 1, 64);
        best_pairs = w - (a0 + bl);
      }
    }
  }
  __syncthreads();   // edge[] is complete
  if (tid == 0) {
    const int bi = best.key / F, bq = best.key % F, bl = bi % LANES, bc = bi / LANES;
    if (bl == 0) stat_lo = bc > 0 ? edge[bc - 1][1][bq] : 0.0f;
    if (bl == LANES - 1) stat_hi = bc + 1 < n_chunks ? edge[bc + 1][0][bq] : 0.0f;
    dst[0] = make_int4(p.a_lo + bi, bq, best_pairs, n_over);
    dst[1] = make_int4(__float_as_int(stat), __float_as_int(stat_lo), __float_as_int(stat_hi), __float_as_int(best.z));
  }
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_cyclo_device: ") + why); }

template <int F>
hipError_t launch(hipError_t err, int64_t groups, CycloParams p, hipStream_t st) {
  return in_grids(err, groups, [&](int64_t first, unsigned cnt) {
    p.first = first;
    hipLaunchKernelGGL(cyclo_kernel<F>, dim3(cnt), dim3(64 * WAVES), 0, st, p);
    return hipGetLastError();
  });
}

}  // namespace
}  // namespace crn

int crn_cyclo_device(crn_handle *h, const float *d_frames, int64_t n_epochs, const crn_cyclo_params *params, const crn_segment_epoch *d_epochs,
                     const crn_segment *d_segments, crn_cyclo *d_cyclo, float *d_profile, void *stream) {
  static_assert(sizeof(crn_cyclo_params) == 36 && sizeof(crn_cyclo) == 32 && sizeof(crn_segment) == 32 && sizeof(crn_segment_epoch) == 16,
                "include/crn_sense.h");
  if (!h || !params || !d_frames || !d_epochs || !d_segments || !d_cyclo) return crn::refuse("null handle / params / frames / epochs / segments / cyclo");
  const crn_cyclo_params &q = *params;
  if (n_epochs < 0) return crn::refuse("n_epochs < 0");
  if (q.max_segments < 1 || q.max_segments > 256) return crn::refuse("max_segments must be in 1..256");
  if (q.frames != 8 && q.frames != 16 && q.frames != 32 && q.frames != 64) return crn::refuse("frames must be 8, 16, 32 or 64");
  if (q.a_lo < 1) return crn::refuse("a_lo must be >= 1");
  if (q.n_a < 1 || q.n_a > 128) return crn::refuse("n_a must be in 1..128");
  if (q.max_width < 2 || q.max_width > 1024) return crn::refuse("max_width must be in 2..1024");
  if (q.min_pairs < 1 || q.min_pairs > q.max_width) return crn::refuse("min_pairs must be in 1..max_width");
  if (!std::isfinite(q.z_min)) return crn::refuse("z_min must be finite");
  if (q.reserved[0] != 0 || q.reserved[1] != 0) return crn::refuse("reserved must be 0");
  if (crn::misaligned(d_frames, 16) || crn::misaligned(d_epochs, 16) || crn::misaligned(d_segments, 16) || crn::misaligned(d_cyclo, 16) ||
      crn::misaligned(d_profile, 16))
    return crn::refuse("d_frames, d_epochs, d_segments, d_cyclo and d_profile must be 16-byte aligned");
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  if ((int64_t)q.a_lo + q.n_a - 1 > n / 2) return crn::refuse("a_lo + n_a - 1 must be <= fft_len / 2");
  if (n_epochs == 0) return CRN_OK;
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const crn::CycloParams p{d_frames, d_epochs, d_segments, d_cyclo, d_profile, 0, n, q.max_segments, q.a_lo, q.n_a, q.max_width, q.min_pairs, q.z_min};
  const int64_t groups = n_epochs * q.max_segments;
  switch (q.frames) {
    case 8: err = crn::launch<8>(err, groups, p, st); break;
    case 16: err = crn::launch<16>(err, groups, p, st); break;
    case 32: err = crn::launch<32>(err, groups, p, st); break;
    default: err = crn::launch<64>(err, groups, p, st); break;
  }
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_cyclo_device: ") + hipGetErrorString(err));
  return CRN_OK;
}
