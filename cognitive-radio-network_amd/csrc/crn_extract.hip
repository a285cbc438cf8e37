// crn_extract.hip — detected emitters as baseband sample streams (crn_extract_device, include/crn_sense.h): the overlap-save channelizer
// on the per-frame spectra of half-overlapped frames.  Per channel and frame the M bins around the centre are tapered and taken back
// by an M-point inverse DFT; the middle half of the block is kept and its sign set by the parity of centre x frame index.
//
// Mapping: one wave per workgroup, one instantiation per M in {16, 32, 64, 128, 256}.  A (channel, frame) pair is one transform, held by
// L = M / 16 lanes of 16 values each, so a wave takes 64 / L consecutive frames of one channel at a time and PASSES such groups in turn;
// the taper and the twiddle factors of a lane are the same for all of them and stay in registers.
//   1. lane l of a transform reads Z[j] for j = L a + l, a = 0 .. 15 (for each a the L lanes read 8 L consecutive bytes of the frame's row,
//      8-byte loads, any centre; every bin index is masked with N - 1), multiplies by the taper, and transforms over a in registers:
//      radix 2, decimation in frequency, every index and twiddle factor a compile-time constant, no scratch.  With j' = j - M / 2 the
//      definition's e^(+j 2 pi j' n / M) is (-1)^n e^(+j 2 pi j n / M): the sign goes into the final scale.
//   2. output n1 of lane l is turned by e^(+j 2 pi l n1 / M) and handed over through LDS, [n1][lane] with rows of 65 (writes and reads
//      then fall on different banks).
//   3. lane r takes n1 = r C .. r C + C - 1 (C = 16 / L), transforms the L values of each over l, and keeps n = n1 + 16 n2 inside the middle
//      half: n2 = L / 4 .. 3 L / 4 - 1 (at L = 2 the one n2 that puts n there; at L = 1 there is no second pass and n1 = 4 .. 11).  What
//      the compiler sees of the L-point transform is only what those outputs need.  A lane's 8 samples go out as 16-byte stores (8-byte at
//      L = 16, where consecutive samples lie in consecutive lanes); the frames of a wave are consecutive, so it writes 4096 contiguous bytes.
// A channel whose stream is outside the batch gets zeros.  Whatever the records hold, a workgroup reads rows of its own stream's frames and
// the taper, and writes its own channel's row.  No atomics, no scratch, nothing depends on timing.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_segments.h"

namespace crn {
namespace {

constexpr int PASSES = 4;   // groups of 64 / L frames that one wave takes in turn
constexpr int ROW = 65;     // complex words of an LDS row: 64 lanes and one of padding

struct ExtractParams {
  const float2 *spectra;                  // [S][F][N] complex
  const crn_extract_channel *channels;    // [n_chan]
  const float *taper;                     // [M]
  float2 *out;                            // [n_chan][F M / 2] complex
  long long first;                        // (channel, chunk) of workgroup 0
  long long S;                            // streams of the batch
  int N, F, t0, chunks;                   // chunks: workgroups to a channel
  float scale;                            // 1 / N
};

// cos(2 pi k / 256), k = 0 .. 64, rounded to fp32 from fp64; the other three quadrants follow by symmetry
__device__ constexpr float QCOS[65] = {
    1.0f, 0.99969881772995f, 0.9987954497337341f, 0.9972904324531555f, 0.9951847195625305f, 0.9924795627593994f, 0.9891765117645264f, 0.9852776527404785f,
    0.9807852506637573f, 0.9757021069526672f, 0.9700312614440918f, 0.9637760519981384f, 0.9569403529167175f, 0.949528157711029f, 0.9415440559387207f, 0.9329928159713745f,
    0.9238795042037964f, 0.91420978307724f, 0.903989315032959f, 0.89322429895401f, 0.8819212913513184f, 0.8700869679450989f, 0.8577286005020142f, 0.8448535799980164f,
    0.8314695954322815f, 0.8175848126411438f, 0.803207516670227f, 0.7883464097976685f, 0.7730104327201843f, 0.7572088241577148f, 0.7409511208534241f, 0.7242470979690552f,
    0.7071067690849304f, 0.6895405650138855f, 0.6715589761734009f, 0.6531728506088257f, 0.6343932747840881f, 0.6152315735816956f, 0.5956993103027344f, 0.5758081674575806f,
    0.5555702447891235f, 0.5349976420402527f, 0.5141027569770813f, 0.49289819598197937f, 0.4713967442512512f, 0.4496113359928131f, 0.4275550842285156f, 0.40524131059646606f,
    0.3826834261417389f, 0.3598950505256653f, 0.3368898630142212f, 0.3136817514896393f, 0.290284663438797f, 0.2667127549648285f, 0.24298018217086792f, 0.21910123527050018f,
    0.19509032368659973f, 0.1709618866443634f, 0.1467304676771164f, 0.12241067737340927f, 0.0980171412229538f, 0.0735645666718483f, 0.049067676067352295f, 0.024541229009628296f,
    0.0f};

// e^(+j 2 pi k / 256), k = 0 .. 255 (scalar selects: with the four quadrants chosen as whole float2 values this toolchain's code gave the
// fourth quadrant wrongly on the device, which the comparison with the twin at M = 128 and 256 showed)
__device__ __forceinline__ float2 unit256(int k) {
  const int q = k >> 6, r = k & 63;   // quadrant q: (a, b), (-b, a), (-a, -b), (b, -a) with a = cos, b = sin of the remainder
  const float a = QCOS[r], b = QCOS[64 - r];
  const float c = q & 1 ? b : a, s = q & 1 ? a : b;
  return make_float2(q == 1 || q == 2 ? -c : c, q >= 2 ? -s : s);
}

// position p of a transform's output holds the coefficient of this index (P a power of two)
template <int P>
__device__ constexpr int bit_reversed(int p) {
  int q = 0;
  for (int b = 1; b < P; b *= 2, p /= 2) q = q * 2 + (p & 1);
  return q;
}

// the inverse DFT of P <= 16 values in place, sum of x[a] e^(+j 2 pi a n / P), unscaled, output in bit-reversed order; every loop unrolls
template <int P>
__device__ __forceinline__ void idft(float (&re)[P], float (&im)[P]) {
#pragma unroll
  for (int h = P / 2; h >= 1; h /= 2) {
#pragma unroll
    for (int b = 0; b < P; b += 2 * h) {
#pragma unroll
      for (int j = 0; j < h; j++) {
        const int k = j * (128 / h);   // the factor e^(+j 2 pi j / (2 h)) = e^(+j 2 pi k / 256), k < 128
        const float ur = re[b + j], ui = im[b + j], tr = re[b + j + h], ti = im[b + j + h];
        re[b + j] = ur + tr;
        im[b + j] = ui + ti;
        const float dr = ur - tr, di = ui - ti;
        if (k == 0) {
          re[b + j + h] = dr;
          im[b + j + h] = di;
        } else if (k == 64) {   // +j
          re[b + j + h] = -di;
          im[b + j + h] = dr;
        } else {
          const float c = k < 64 ? QCOS[k] : -QCOS[128 - k], s = k < 64 ? QCOS[64 - k] : QCOS[k - 64];
          re[b + j + h] = dr * c - di * s;
          im[b + j + h] = di * c + dr * s;
        }
      }
    }
  }
}

template <int M>
__global__ __launch_bounds__(64) void extract_kernel(const ExtractParams p) {
  constexpr int L = M / 16, G = 64 / L, C = 16 / L, H = M / 2;   // lanes of a transform, transforms of a wave, n1 of a lane, samples of a frame
  __shared__ float2 ex[L > 1 ? 16 * ROW : 1];
  const int lane = threadIdx.x, l = lane % L, fl = lane / L;
  const long long g = p.first + blockIdx.x;   // < n_chan chunks
  const long long c = g / p.chunks;
  const long long t_first = (g - c * p.chunks) * (G * PASSES);   // 64-bit: F may be close to 2^31
  const long long t_end = t_first + G * PASSES < p.F ? t_first + G * PASSES : p.F;   // the workgroup's frames of the channel's row
  const int4 rec = *reinterpret_cast<const int4 *>(p.channels + c);
  const int mask = p.N - 1, kappa = rec.y & mask;
  float2 *const row = p.out + c * p.F * H;

  if (rec.x < 0 || rec.x >= p.S) {   // the whole workgroup: no such stream, zeros
    float4 *const dst = reinterpret_cast<float4 *>(row);
    for (long long i = t_first * (H / 2) + lane; i < t_end * (H / 2); i += 64) dst[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }

  // what a lane keeps over its frames: its 16 taper values and, position by position of pass 1's output, e^(+j 2 pi l n1 / M)
  float hw[16];
#pragma unroll
  for (int a = 0; a < 16; a++) hw[a] = p.taper[L * a + l];
  float twr[16], twi[16];
  if constexpr (L > 1) {
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const float2 w = unit256(l * bit_reversed<16>(q) * (256 / M));   // l n1 < L 16 = M: below 256
      twr[q] = w.x;
      twi[q] = w.y;
    }
  }

  const float2 *const frames = p.spectra + rec.x * (long long)p.F * p.N;
  const int b0 = kappa - M / 2 + l;
  for (int ps = 0; ps < PASSES; ps++) {
    const long long tb = t_first + ps * G;   // the same for the whole workgroup
    if (tb >= p.F) break;
    const long long t = tb + fl;
    const bool live = t < p.F;
    const float2 *const x = frames + (live ? t : p.F - 1) * p.N;
    float re[16], im[16];
#pragma unroll
    for (int a = 0; a < 16; a++) {
      const float2 v = x[(b0 + L * a) & mask];
      re[a] = v.x * hw[a];
      im[a] = v.y * hw[a];
    }
    idft<16>(re, im);
    // 1 / N, the turn of the mixer between frames, and below (-1)^n
    const float s = (kappa & (p.t0 ^ (int)t) & 1) ? -p.scale : p.scale;
    float2 *const dst = row + t * H;

    if constexpr (L == 1) {
      if (live) {
#pragma unroll
        for (int n = 4; n < 12; n += 2) {
          const int q0 = bit_reversed<16>(n), q1 = bit_reversed<16>(n + 1);
          *reinterpret_cast<float4 *>(dst + (n - 4)) = make_float4(re[q0] * s, im[q0] * s, re[q1] * -s, im[q1] * -s);
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < 16; q++) ex[bit_reversed<16>(q) * ROW + lane] = make_float2(re[q] * twr[q] - im[q] * twi[q], im[q] * twr[q] + re[q] * twi[q]);
      __syncthreads();
      if constexpr (L == 2) {
        // n = n1 + 16 n2 in 8 .. 23: lane 0 (n1 = 0 .. 7) keeps n2 = 1, lane 1 (n1 = 8 .. 15) keeps n2 = 0
        const float sg = l ? 1.0f : -1.0f;
        float yr[8], yi[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const float2 v0 = ex[(l * 8 + j) * ROW + fl * 2], v1 = ex[(l * 8 + j) * ROW + fl * 2 + 1];
          const float sj = j & 1 ? -s : s;
          yr[j] = (v0.x + sg * v1.x) * sj;
          yi[j] = (v0.y + sg * v1.y) * sj;
        }
        if (live) {
#pragma unroll
          for (int j = 0; j < 8; j += 2) *reinterpret_cast<float4 *>(dst + (l ? 0 : 8) + j) = make_float4(yr[j], yi[j], yr[j + 1], yi[j + 1]);
        }
      } else {
        float yr[L / 2][C], yi[L / 2][C];
#pragma unroll
        for (int j = 0; j < C; j++) {
          const int n1 = l * C + j;
          float vr[L], vi[L];
#pragma unroll
          for (int l2 = 0; l2 < L; l2++) {
            const float2 v = ex[n1 * ROW + fl * L + l2];
            vr[l2] = v.x;
            vi[l2] = v.y;
          }
          idft<L>(vr, vi);
          const float sj = (C == 1 ? l : j) & 1 ? -s : s;   // (-1)^n1, n1 = l C + j
#pragma unroll
          for (int m = 0; m < L / 2; m++) {
            const int q = bit_reversed<L>(L / 4 + m);
            yr[m][j] = vr[q] * sj;
            yi[m][j] = vi[q] * sj;
          }
        }
        if (live) {
#pragma unroll
          for (int m = 0; m < L / 2; m++) {
            float2 *const d = dst + 16 * m + l * C;   // u = n1 + 16 n2 - M / 4 with n2 = L / 4 + m
            if constexpr (C == 1) {
              d[0] = make_float2(yr[m][0], yi[m][0]);
            } else {
#pragma unroll
              for (int j = 0; j < C; j += 2) *reinterpret_cast<float4 *>(d + j) = make_float4(yr[m][j], yi[m][j], yr[m][j + 1], yi[m][j + 1]);
            }
          }
        }
      }
      __syncthreads();   // the rows are read before the next group writes them
    }
  }
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_extract_device: ") + why); }

template <int M>
hipError_t launch(hipError_t err, int64_t n_chan, ExtractParams p, hipStream_t st) {
  const int per = (64 / (M / 16)) * PASSES;   // frames of a workgroup
  p.chunks = (int)(((int64_t)p.F + per - 1) / per);
  return in_grids(err, n_chan * p.chunks, [&](int64_t first, unsigned cnt) {
    p.first = first;
    hipLaunchKernelGGL(extract_kernel<M>, dim3(cnt), dim3(64), 0, st, p);
    return hipGetLastError();
  });
}

}  // namespace
}  // namespace crn

int crn_extract_device(crn_handle *h, const float *d_spectra, int64_t n_frames, const crn_extract_params *params, const crn_extract_channel *d_channels,
                       int32_t n_chan, const float *d_taper, float *d_out, void *stream) {
  static_assert(sizeof(crn_extract_params) == 32 && sizeof(crn_extract_channel) == 16, "include/crn_sense.h");
  if (!h || !params || !d_spectra || !d_channels || !d_taper || !d_out) return crn::refuse("null handle / params / spectra / channels / taper / out");
  const crn_extract_params &q = *params;
  const int m = q.out_len;
  if (m != 16 && m != 32 && m != 64 && m != 128 && m != 256) return crn::refuse("out_len must be 16, 32, 64, 128 or 256");
  if (n_frames < 0) return crn::refuse("n_frames < 0");
  if (q.frames_per_stream < 1 || n_frames % q.frames_per_stream != 0) return crn::refuse("frames_per_stream must be >= 1 and divide n_frames");
  if (q.t0 < 0) return crn::refuse("t0 < 0");
  if (n_chan < 0 || n_chan > 65536) return crn::refuse("n_chan must be in 0..65536");
  for (int i = 0; i < 5; i++)
    if (q.reserved[i] != 0) return crn::refuse("reserved must be 0");
  if (crn::misaligned(d_spectra, 16) || crn::misaligned(d_channels, 16) || crn::misaligned(d_taper, 16) || crn::misaligned(d_out, 16))
    return crn::refuse("d_spectra, d_channels, d_taper and d_out must be 16-byte aligned");
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  if (m > n / 2) return crn::refuse("out_len must be <= fft_len / 2");
  if (n_frames == 0 || n_chan == 0) return CRN_OK;
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const crn::ExtractParams p{reinterpret_cast<const float2 *>(d_spectra), d_channels, d_taper, reinterpret_cast<float2 *>(d_out), 0,
                             n_frames / q.frames_per_stream, n, q.frames_per_stream, q.t0, 1, 1.0f / (float)n};
  switch (m) {
    case 16: err = crn::launch<16>(err, n_chan, p, st); break;
    case 32: err = crn::launch<32>(err, n_chan, p, st); break;
    case 64: err = crn::launch<64>(err, n_chan, p, st); break;
    case 128: err = crn::launch<128>(err, n_chan, p, st); break;
    default: err = crn::launch<256>(err, n_chan, p, st); break;
  }
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_extract_device: ") + hipGetErrorString(err));
  return CRN_OK;
}
