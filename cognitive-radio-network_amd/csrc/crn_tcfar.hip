// crn_tcfar.hip — ordered-statistic CFAR along time, per bin (crn_tcfar_device, include/crn_sense.h): a bin of a `spectrum` row is tested
// against its own D rows before the guard epochs, fl32(alpha c) < P counted against `rank`, the rows before the batch coming from the
// caller's history ring.  Every (epoch, bin) decision is independent given the rows, so the stage is parallel along time and along bins.
// Three launches on the caller's stream:
//
//   1. open    tcfar_open_kernel: d_seen[s] = seen + T, seen = first ? 0 : clamp(d_seen[s]), so that the launches behind it read one
//              normalised value (seen = d_seen[s] - T) and nobody reads d_seen while it changes; the headers are zeroed.
//   2. tiles   tcfar_kernel, one workgroup of eight waves per tile of one stream: a strip of 64 bins x a run of R epochs.  The tile's rows
//              and the H rows before them are staged in LDS once, as fl32(alpha c): from the batch, or from d_hist by slot where they
//              precede it; rows of epochs never seen are not read.  With the H rows in front, the cells of the tile's epoch e are the
//              staged rows e .. e + D - 1.  A lane owns a bin and a wave four consecutive epochs at a time: the D + 3 rows their windows
//              cover are read from LDS once each and held against four test values in registers.  The mask words of an (epoch, strip)
//              are a ballot.  R = 256 - 7 - H rounded down to 32, evened out over the runs of a stream: the rows before a tile are read
//              again by the tile behind it, (H + R) / R of the input, 1.41 at D = 64, g = 1, 2.5 at the largest H.
//              A header sums the bits of N / 64 workgroups and the entry point has no workspace: each workgroup adds its two counts
//              with one 64-bit integer atomic (exact in any order), skipped where both are zero; n_cells is a plain store of strip 0.
//   3. history tcfar_hist_kernel, one workgroup per (stream, row): the batch's last min(T, H) rows go to their slots.  It runs behind the
//              tiles, which read the old slots.
// d_seen and d_hist are read as values: the slot n mod H is computed, never loaded.  No scratch memory, plain vector stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_segments.h"

namespace crn {
namespace {

constexpr int STRIP = 64;                  // bins of a tile: a lane each
constexpr int TILE_ROWS = 256;             // staged rows of a tile, the H before its first epoch included: 64 KB of LDS
constexpr int WAVES = 8, QUAD = 4;         // waves of a workgroup; epochs a wave decides at a time
constexpr int SLACK = 7;                   // staged rows a wave may read beyond its last window: it takes rows eight at a time
constexpr long long SEEN_MAX = 1ll << 62;

struct TcfarParams {
  const float *spectrum;     // [n_epochs][N]
  const uint32_t *or_mask;   // [n_epochs][N / 32] or null
  uint32_t *mask;            // [n_epochs][N / 32] or null
  crn_tcfar_row *rows;       // [n_epochs] or null
  float *hist;               // [n_streams][H][N]
  long long *seen;           // [n_streams]
  long long first;           // index of workgroup 0 (tiles, history rows) or of thread 0's workgroup (open)
  long long n_epochs, n_streams;
  int N, eps, runs, R;       // runs of R epochs to a stream
  int D, g, rank, fresh;
  float alpha;
};

__global__ __launch_bounds__(256) void tcfar_open_kernel(const TcfarParams p) {
  const long long i = (p.first + blockIdx.x) * 256 + threadIdx.x;
  if (p.rows != nullptr && i < p.n_epochs) reinterpret_cast<int4 *>(p.rows)[i] = make_int4(0, 0, 0, 0);
  if (i < p.n_streams) {
    long long seen = 0;
    if (!p.fresh) {
      seen = p.seen[i];
      seen = seen < 0 ? 0 : seen > SEEN_MAX ? SEEN_MAX : seen;
    }
    p.seen[i] = seen + p.eps;
  }
}

// bits lo .. hi - 1 of a word, 0 <= lo, hi <= 32; none when hi <= lo
__device__ __forceinline__ uint32_t bit_span(int lo, int hi) { return hi > lo ? (uint32_t)(((1ull << (hi - lo)) - 1) << lo) : 0u; }

__global__ __launch_bounds__(64 * WAVES) void tcfar_kernel(const TcfarParams p) {
  __shared__ float4 tile4[TILE_ROWS * STRIP / 4];
  float *tile = reinterpret_cast<float *>(tile4);
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int N = p.N, strips = N / STRIP, D = p.D, H = p.D + p.g;
  const long long idx = p.first + blockIdx.x;
  const int strip = (int)(idx % strips);
  const long long rest = idx / strips;
  const int run = (int)(rest % p.runs);
  const long long stream = rest / p.runs;
  const int t0 = run * p.R, nr = p.eps - t0 < p.R ? p.eps - t0 : p.R;      // the tile's epochs t0 .. t0 + nr - 1 of the call
  const long long seen = p.seen[stream] - p.eps;                            // tcfar_open_kernel left seen + T
  const int slot0 = (int)(seen % H);
  const float *batch = p.spectrum + stream * p.eps * N + strip * STRIP;
  const float *hist = p.hist + stream * H * N + strip * STRIP;

  // staged row j is the call's epoch t0 - H + j: 16 lanes to a row, four floats each; a thread's loads are all issued before the first
  // product is stored, so that a tile waits for memory once
  {
    constexpr int PASS = 64 * WAVES / 16, PASSES = TILE_ROWS / PASS;      // rows staged in one pass of the workgroup
    const int c4 = (tid & 15) * 4;
    float4 c[PASSES];
#pragma unroll
    for (int i = 0; i < PASSES; i++) {
      const int j = (tid >> 4) + i * PASS, t = t0 - H + j;                  // t >= -H
      // an epoch never seen is not read, and no decision uses it
      const bool there = j < H + nr && seen + t >= 0;
      const float *src = t >= 0 ? batch + (long long)t * N : hist + (long long)((slot0 + t + H) % H) * N;
      c[i] = there ? *reinterpret_cast<const float4 *>(src + c4) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int i = 0; i < PASSES; i++) {
      const int j = (tid >> 4) + i * PASS;
      if (j < H + nr)
        *reinterpret_cast<float4 *>(tile + j * STRIP + c4) = make_float4(p.alpha * c[i].x, p.alpha * c[i].y, p.alpha * c[i].z, p.alpha * c[i].w);
    }
  }
  __syncthreads();

  // the test values of a quad are loaded while the quad before it is counted
  float next[QUAD];
#pragma unroll
  for (int q = 0; q < QUAD; q++) next[q] = w * QUAD + q < nr ? batch[(long long)(t0 + w * QUAD + q) * N + l] : 0.0f;
  for (int e0 = w * QUAD; e0 < nr; e0 += WAVES * QUAD) {
    uint32_t P[QUAD];
#pragma unroll
    for (int q = 0; q < QUAD; q++) {
      const int e = e0 + WAVES * QUAD + q;
      P[q] = __float_as_uint(next[q]);
      next[q] = e < nr ? batch[(long long)(t0 + e) * N + l] : 0.0f;
    }
    // The window of epoch e0 + q is the staged rows e0 + q .. e0 + q + D - 1: the quad's windows cover D + 3 rows.  Non-negative floats
    // order as their bit patterns and the difference of two patterns cannot overflow, so the sign of pattern(fl32(alpha c)) - pattern(P)
    // is "the cell is below the test value", exactly, ties and denormals included.  Every row is read once and its four signs are
    // shifted into a word per epoch, one subtraction and one shift-in per cell and no condition code through a scalar register; every
    // 32 rows the words are counted under the mask of the rows that lie in the epoch's window.  The rows are taken eight at a time, up
    // to seven beyond the last window (SLACK), which the masks drop.
    int cnt[QUAD] = {0, 0, 0, 0};
    const float *col = tile + e0 * STRIP + l;
    const int J = (D + QUAD - 1 + SLACK) & ~SLACK;
    for (int j0 = 0; j0 < J; j0 += 32) {
      const int n = J - j0 < 32 ? J - j0 : 32;
      uint32_t below[QUAD] = {0, 0, 0, 0};
      for (int j = j0; j < j0 + n; j += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const uint32_t v = __float_as_uint(col[(j + u) * STRIP]);
#pragma unroll
          for (int q = 0; q < QUAD; q++) below[q] = __builtin_amdgcn_alignbit(below[q], v - P[q], 31);
        }
      }
      // row j0 + i of the block ended up in bit n - 1 - i
#pragma unroll
      for (int q = 0; q < QUAD; q++) {
        const int first = (q > j0 ? q : j0) - j0, last = (q + D < j0 + n ? q + D : j0 + n) - j0;
        cnt[q] += __popc(below[q] & bit_span(n - last, n - first));
      }
    }
    // rows beyond the tile's last epoch were never staged: what was counted on them belongs to epochs beyond nr, which nobody writes
    uint64_t det = 0;
#pragma unroll
    for (int q = 0; q < QUAD; q++) {
      const uint64_t b = __ballot(cnt[q] >= p.rank);
      if (l == q) det = b;
    }
    // lane q finishes epoch e0 + q
    const int e = e0 + l;
    if (l < QUAD && e < nr) {
      const long long row = stream * p.eps + t0 + e;
      const bool past = seen + t0 + e >= H;
      if (!past) det = 0;                                             // the warm-up: no cells
      uint64_t om = 0;
      if (p.or_mask != nullptr) {
        const uint2 o = reinterpret_cast<const uint2 *>(p.or_mask + row * (N / 32))[strip];
        om = (uint64_t)o.x | ((uint64_t)o.y << 32);
      }
      const uint64_t out = det | om;
      if (p.mask != nullptr) reinterpret_cast<uint2 *>(p.mask + row * (N / 32))[strip] = make_uint2((uint32_t)out, (uint32_t)(out >> 32));
      if (p.rows != nullptr) {
        // n_detected and n_new are neighbours: one 64-bit add, no carry between them (each sum is at most N)
        const unsigned long long both = (unsigned long long)__popcll(out) | ((unsigned long long)__popcll(det & ~om) << 32);
        if (both != 0) atomicAdd(reinterpret_cast<unsigned long long *>(p.rows + row), both);
        if (strip == 0 && past) p.rows[row].n_cells = D;
      }
    }
  }
}

__global__ __launch_bounds__(256) void tcfar_hist_kernel(const TcfarParams p) {
  const int N = p.N, H = p.D + p.g, m = p.eps < H ? p.eps : H;             // the batch's last m rows
  const long long idx = p.first + blockIdx.x;
  const long long stream = idx / m;
  const int t = p.eps - m + (int)(idx % m);
  const long long seen = p.seen[stream] - p.eps;
  const int slot = (int)((seen + t) % H);
  const float4 *src = reinterpret_cast<const float4 *>(p.spectrum + (stream * p.eps + t) * N);
  float4 *dst = reinterpret_cast<float4 *>(p.hist + (stream * H + slot) * N);
  for (int i = threadIdx.x; i < N / 4; i += 256) dst[i] = src[i];
}

// Why q cannot serve, as the text that follows the entry point's name, or null when it can
const char *tcfar_params_refusal(const crn_tcfar_params &q) {
  if (q.epochs_per_stream < 1) return "epochs_per_stream < 1";
  if (q.cells < 2 || q.cells > 128 || q.cells % 2 != 0) return "cells must be even and in 2..128";
  if (q.guard_epochs < 0 || q.guard_epochs > 16) return "guard_epochs must be in 0..16";
  if (q.rank < 1 || q.rank > q.cells) return "rank must be in 1..cells";
  if (!std::isfinite(q.alpha) || !(q.alpha > 0.0f)) return "alpha must be finite and > 0";
  if (q.reserved[0] != 0 || q.reserved[1] != 0) return "reserved must be 0";
  return nullptr;
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_tcfar_device: ") + why); }

template <class K>
hipError_t launch(K kernel, int threads, const TcfarParams &p, unsigned n, hipStream_t stream) {
  hipLaunchKernelGGL(kernel, dim3(n), dim3(threads), 0, stream, p);
  return hipGetLastError();
}

}  // namespace
}  // namespace crn

int64_t crn_tcfar_hist_bytes(int64_t n_streams, int32_t fft_len, const crn_tcfar_params *params) {
  if (!params || n_streams < 1 || crn::tcfar_params_refusal(*params)) return -1;
  if (fft_len != 512 && fft_len != 1024 && fft_len != 2048 && fft_len != 4096) return -1;
  return n_streams * (params->cells + params->guard_epochs) * fft_len * (int64_t)sizeof(float);
}

int crn_tcfar_device(crn_handle *h, const float *d_spectrum, int64_t n_epochs, const crn_tcfar_params *params, const uint32_t *d_or_mask,
                     uint32_t *d_bin_mask, crn_tcfar_row *d_rows, float *d_hist, int64_t *d_seen, void *stream) {
  static_assert(sizeof(crn_tcfar_params) == 32 && sizeof(crn_tcfar_row) == 16, "include/crn_sense.h");
  static_assert(crn::TILE_ROWS * crn::STRIP * sizeof(float) == 65536 && crn::TILE_ROWS - crn::SLACK - (128 + 16) >= crn::WAVES * crn::QUAD, "the tile and its smallest run");
  if (!h || !params || !d_spectrum || !d_hist || !d_seen) return crn::refuse("null handle / params / spectrum / hist / seen");
  const crn_tcfar_params &q = *params;
  if (n_epochs < 0) return crn::refuse("n_epochs < 0");
  if (const char *why = crn::tcfar_params_refusal(q)) return crn::refuse(why);
  if (n_epochs % q.epochs_per_stream != 0) return crn::refuse("epochs_per_stream must divide n_epochs");
  if (crn::misaligned(d_spectrum, 16) || crn::misaligned(d_rows, 16) || crn::misaligned(d_hist, 16))
    return crn::refuse("d_spectrum, d_rows and d_hist must be 16-byte aligned");
  if (crn::misaligned(d_or_mask, 8) || crn::misaligned(d_bin_mask, 8) || crn::misaligned(d_seen, 8))
    return crn::refuse("d_or_mask, d_bin_mask and d_seen must be 8-byte aligned");
  if (n_epochs == 0) return CRN_OK;

  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  const int T = q.epochs_per_stream, H = q.cells + q.guard_epochs;
  const int64_t n_streams = n_epochs / T;
  // runs of at most TILE_ROWS - SLACK - H epochs, a multiple of what the waves decide at a time, evened out over the stream
  const int most = (crn::TILE_ROWS - crn::SLACK - H) / (crn::WAVES * crn::QUAD) * (crn::WAVES * crn::QUAD);
  const int runs = (int)((int64_t(T) + most - 1) / most);
  const int per = (int)((int64_t(T) + runs - 1) / runs);
  const int R = (per + crn::WAVES * crn::QUAD - 1) / (crn::WAVES * crn::QUAD) * (crn::WAVES * crn::QUAD);
  crn::TcfarParams p{d_spectrum, d_or_mask, d_bin_mask, d_rows, d_hist, reinterpret_cast<long long *>(d_seen), 0, (long long)n_epochs,
                     (long long)n_streams, n, T, (int)((int64_t(T) + R - 1) / R), R, q.cells, q.guard_epochs, q.rank, q.first != 0, q.alpha};
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t opened = d_rows != nullptr && n_epochs > n_streams ? n_epochs : n_streams;
  err = crn::in_grids(err, (opened + 255) / 256, [&](int64_t first, unsigned cnt) {
    p.first = first;
    return crn::launch(crn::tcfar_open_kernel, 256, p, cnt, st);
  });
  if (d_bin_mask != nullptr || d_rows != nullptr)
    err = crn::in_grids(err, n_streams * p.runs * (n / crn::STRIP), [&](int64_t first, unsigned cnt) {
      p.first = first;
      return crn::launch(crn::tcfar_kernel, 64 * crn::WAVES, p, cnt, st);
    });
  err = crn::in_grids(err, n_streams * (T < H ? T : H), [&](int64_t first, unsigned cnt) {
    p.first = first;
    return crn::launch(crn::tcfar_hist_kernel, 256, p, cnt, st);
  });
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_tcfar_device: ") + hipGetErrorString(err));
  return CRN_OK;
}
