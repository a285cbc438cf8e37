// crn_channels.hip — per-channel occupancy statistics over time (crn_channels_device, crn_channel_forecast, include/crn_sense.h): the
// CFAR bit mask and, optionally, the `spectrum` rows of a batch become one record per stream and channel that the caller carries from
// call to call.  Three small launches on the caller's stream, all scratch in the caller's workspace:
//
//   1. epoch  channels_epoch_kernel<B>, one wave per epoch, the lane-owns-B-bins mapping of segments_kernel<B> (crn_mask_runs.h): the
//             row is read once with coalesced float4 loads into LDS (padded by 4 floats per lane piece), the mask piece sits in a
//             register.  Lane l sums its own B bins once (fp64) and leaves that sum and its mask piece in LDS.  Then lane c owns
//             channel c: it walks the pieces the span touches, at most two of them partly (bin by bin, only bins inside the span) and
//             the others whole (the owning lane's sum and popcount).  A channel-by-channel loop with a wave reduction each would leave
//             one lane at work in the 64-band plan, where every span is one lane piece; here the 64 channels go side by side and a span
//             of any width costs at most 2 (B - 1) bin reads and 62 piece sums.  Every sum is direct and in a fixed order: no bin outside
//             a span enters it (no difference of prefix sums: a +90 dB neighbour leaves nothing behind), and an epoch gives the same
//             bytes in any batch.  One busy word and n_channels fp32 powers per epoch, to the caller's arrays or to the workspace.
//   2. time   channels_time_kernel, one wave per 64 consecutive epochs of a stream, lane c = channel c: 64 busy words become the lane's
//             64-bit time word by ballots; transitions, head and tail run and the counts come from bit arithmetic, the runs inside from
//             one walk over them (lengths <= 62: their histogram is six 8-bit fields of one word), the two power sums from one
//             coalesced read per epoch.  One summary (TimeSum) per chunk and channel.
//   3. join   channels_join_kernel, one workgroup per stream, lane c = channel c in each of up to 8 waves: every wave folds a contiguous
//             share of the stream's chunk summaries with the associative sum_join (a, then b right behind it: the manner of acc_join in
//             crn_segments.hip), the waves' results are folded through LDS, and the carried record, the leftmost operand, takes the
//             total.  A stream of T epochs is T / 64 / 8 + 8 dependent steps, not T.  The histogram is integer adds in LDS.
// Integer results do not depend on the order work ran in; power[] is an fp64 sum of the fp32 powers in the order of the joins.
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

constexpr int JOIN_WAVES = 8;    // (a time summary is over CHUNK = 64 epochs: one bit each of a lane's time word)

struct ChanParams {
  const uint32_t *mask;     // [n_epochs][N / 32]
  const float *spectrum;    // [n_epochs][N] or null
  uint64_t *busy;           // [n_epochs]
  float *power;             // [n_epochs][nch], null without spectrum
  long long first;          // epoch of workgroup 0
  int nch, min_bins;
  crn_channel_span span[CRN_MAX_CHANNELS];
};

template <int B>
__global__ __launch_bounds__(64) void channels_epoch_kernel(const ChanParams p) {
  constexpr int N = 64 * B;
  __shared__ float4 row4[padded_words(B) / 4];
  __shared__ double piece_sum[64];
  __shared__ uint64_t piece_mask[64];
  float *row = reinterpret_cast<float *>(row4);
  const int l = threadIdx.x;
  const long long e = p.first + blockIdx.x;
  const bool spec = p.spectrum != nullptr;

  if (spec) load_row<B>(row, p.spectrum + e * N, l);
  piece_mask[l] = mask_piece<B>(p.mask + e * (N / 32), l);
  __syncthreads();

  // the lane's own bins, once
  if (spec) {
    const float *mine = own_piece<B>(row, l);
    double w = 0.0;
#pragma unroll
    for (int i4 = 0; i4 < B; i4 += 4) {
      const float4 q = *reinterpret_cast<const float4 *>(mine + i4);
      w += (double)q.x;
      w += (double)q.y;
      w += (double)q.z;
      w += (double)q.w;
    }
    piece_sum[l] = w;
  }
  __syncthreads();

  // lane c owns channel c: positions count from bin 0 without wrapping (lo + width <= 2 N - 1), piece q covers [q B, (q + 1) B)
  int nd = 0;
  double s = 0.0;
  if (l < p.nch) {
    const crn_channel_span sp = p.span[l];
    int pos = sp.lo;
    const int end = sp.lo + sp.width;
    while (pos < end) {
      const int q = pos / B, r = q & 63;
      const int pe = end < (q + 1) * B ? end : (q + 1) * B;
      if (pe - pos == B) {
        nd += __popcll(piece_mask[r]);
        if (spec) s += piece_sum[r];
      } else {
        nd += __popcll(piece_mask[r] & low_bits(pe - q * B) & ~low_bits(pos - q * B));
        if (spec) {
          const float *theirs = own_piece<B>(row, r) - q * B;
          for (int k = pos; k < pe; k++) s += (double)theirs[k];
        }
      }
      pos = pe;
    }
  }
  const uint64_t word = __ballot(l < p.nch && nd >= p.min_bins);
  if (l == 0) p.busy[e] = word;
  if (p.power != nullptr && l < p.nch) p.power[e * p.nch + l] = (float)s;
}

// What a stretch of one channel's epochs comes to.  head: the run that touches its first epoch, tail: the one that touches its last; a
// stretch of one run has head = tail = n and nothing completed.  Completed: the runs that begin and end inside.
struct TimeSum {
  int n, nb;                 // epochs, busy epochs
  int first, last;           // states of the first and last epoch
  int head, tail;
  int t01, t10, t11;         // transitions inside (t00 is the rest of n - 1)
  int nr0, nr1, rs0, rs1, rm0, rm1;   // completed runs: count, summed length, longest; idle and busy
  double pw0, pw1;           // power over idle / busy epochs
};
constexpr int SUM_WORDS = 21;   // 4-byte words of a stored summary: the 15 ints, the two sums, the packed histogram

__device__ __forceinline__ TimeSum sum_empty() { return TimeSum{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0}; }

__device__ __forceinline__ int hist_bin(long long len) {
  const int b = len > 0 ? 63 - __builtin_clzll((unsigned long long)len) : 0;
  return b > 15 ? 15 : b;
}

// a run of `len` epochs in state `st` is complete; an idle one goes to the histogram hist[bin * stride]
__device__ __forceinline__ void sum_complete(TimeSum &r, int st, int len, int *hist, int stride) {
  if (st) {
    r.nr1++;
    r.rs1 += len;
    r.rm1 = len > r.rm1 ? len : r.rm1;
  } else {
    r.nr0++;
    r.rs0 += len;
    r.rm0 = len > r.rm0 ? len : r.rm0;
    atomicAdd(hist + hist_bin(len) * stride, 1);
  }
}

// a, then b right behind it.  Associative; runs that the seam completes are counted here.
__device__ __forceinline__ TimeSum sum_join(const TimeSum &a, const TimeSum &b, int *hist, int stride) {
  if (a.n == 0) return b;
  if (b.n == 0) return a;
  TimeSum r = a;
  r.n = a.n + b.n;
  r.nb = a.nb + b.nb;
  r.last = b.last;
  r.t01 = a.t01 + b.t01 + (a.last == 0 && b.first == 1);
  r.t10 = a.t10 + b.t10 + (a.last == 1 && b.first == 0);
  r.t11 = a.t11 + b.t11 + (a.last == 1 && b.first == 1);
  r.nr0 += b.nr0;
  r.nr1 += b.nr1;
  r.rs0 += b.rs0;
  r.rs1 += b.rs1;
  r.rm0 = b.rm0 > r.rm0 ? b.rm0 : r.rm0;
  r.rm1 = b.rm1 > r.rm1 ? b.rm1 : r.rm1;
  r.pw0 = a.pw0 + b.pw0;
  r.pw1 = a.pw1 + b.pw1;
  const bool a_whole = a.head == a.n, b_whole = b.head == b.n;
  if (a.last == b.first) {                      // a's tail and b's head are one run
    if (a_whole && b_whole) {
      r.head = r.tail = r.n;
    } else if (a_whole) {
      r.head = a.n + b.head;
      r.tail = b.tail;
    } else if (b_whole) {
      r.tail = a.tail + b.n;
    } else {
      sum_complete(r, a.last, a.tail + b.head, hist, stride);
      r.tail = b.tail;
    }
  } else {
    if (!a_whole) sum_complete(r, a.last, a.tail, hist, stride);
    if (b_whole) {
      r.tail = b.n;
    } else {
      sum_complete(r, b.first, b.head, hist, stride);
      r.tail = b.tail;
    }
  }
  return r;
}

struct TimeParams {
  const uint64_t *busy;     // [n_epochs]
  const float *power;       // [n_epochs][nch] or null
  int *sums;                // [n_streams * chunks][SUM_WORDS][nch]
  crn_channel_stats *stats; // [n_streams][nch]
  long long first;          // chunk (time) or stream (join) of workgroup 0
  int nch, eps, chunks, fresh;
};

__device__ __forceinline__ void sum_store(int *at, int nch, const TimeSum &t, uint64_t hist6) {
  const int v[15] = {t.n, t.nb, t.first, t.last, t.head, t.tail, t.t01, t.t10, t.t11, t.nr0, t.nr1, t.rs0, t.rs1, t.rm0, t.rm1};
#pragma unroll
  for (int f = 0; f < 15; f++) at[f * nch] = v[f];
  const long long a = __double_as_longlong(t.pw0), b = __double_as_longlong(t.pw1);
  at[15 * nch] = (int)a;
  at[16 * nch] = (int)(a >> 32);
  at[17 * nch] = (int)b;
  at[18 * nch] = (int)(b >> 32);
  at[19 * nch] = (int)hist6;
  at[20 * nch] = (int)(hist6 >> 32);
}

__device__ __forceinline__ double two_words(int lo, int hi) { return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo)); }

__device__ __forceinline__ TimeSum sum_load(const int *at, int nch, uint64_t *hist6) {
  TimeSum t;
  t.n = at[0];
  t.nb = at[nch];
  t.first = at[2 * nch];
  t.last = at[3 * nch];
  t.head = at[4 * nch];
  t.tail = at[5 * nch];
  t.t01 = at[6 * nch];
  t.t10 = at[7 * nch];
  t.t11 = at[8 * nch];
  t.nr0 = at[9 * nch];
  t.nr1 = at[10 * nch];
  t.rs0 = at[11 * nch];
  t.rs1 = at[12 * nch];
  t.rm0 = at[13 * nch];
  t.rm1 = at[14 * nch];
  t.pw0 = two_words(at[15 * nch], at[16 * nch]);
  t.pw1 = two_words(at[17 * nch], at[18 * nch]);
  *hist6 = ((uint64_t)(uint32_t)at[20 * nch] << 32) | (uint32_t)at[19 * nch];
  return t;
}

__global__ __launch_bounds__(64) void channels_time_kernel(const TimeParams p) {
  const int l = threadIdx.x;
  const long long chunk = p.first + blockIdx.x;
  const ChunkSpan cs = chunk_span(chunk, p.chunks, p.eps);
  const int n = cs.n;
  const long long e0 = cs.stream * p.eps + cs.t0;
  const uint64_t w = l < n ? p.busy[e0 + l] : 0;
  uint64_t x = 0;                                                  // bit i: this lane's channel busy in epoch e0 + i
  for (int c = 0; c < p.nch; c++) {
    const uint64_t col = __ballot((w >> c) & 1);
    if (l == c) x = col;
  }
  if (l >= p.nch) return;

  TimeSum t = sum_empty();
  const uint64_t pairs = low_bits(n - 1);
  t.n = n;
  t.nb = __popcll(x);
  t.first = (int)(x & 1);
  t.last = (int)((x >> (n - 1)) & 1);
  t.t01 = __popcll(~x & (x >> 1) & pairs);
  t.t10 = __popcll(x & ~(x >> 1) & pairs);
  t.t11 = __popcll(x & (x >> 1) & pairs);
  const uint64_t flips = (x ^ (x >> 1)) & pairs;                   // bit i: epochs i and i + 1 differ
  uint64_t hist6 = 0;
  if (flips == 0) {
    t.head = t.tail = n;
  } else {
    t.head = __builtin_ctzll(flips) + 1;
    const int last_flip = 63 - __builtin_clzll(flips);
    t.tail = n - 1 - last_flip;
    // the runs between the first and the last flip
    uint64_t rest = flips & (flips - 1);
    int start = t.head, st = t.first ^ 1;
    while (rest) {
      const int nxt = __builtin_ctzll(rest) + 1;
      const int len = nxt - start;
      if (st) {
        t.nr1++;
        t.rs1 += len;
        t.rm1 = len > t.rm1 ? len : t.rm1;
      } else {
        t.nr0++;
        t.rs0 += len;
        t.rm0 = len > t.rm0 ? len : t.rm0;
        hist6 += 1ull << (8 * (31 - __builtin_clz((unsigned)len)));   // len <= 62: bins 0..5, at most 31 runs each
      }
      start = nxt;
      st ^= 1;
      rest &= rest - 1;
    }
  }
  if (p.power != nullptr) {
    const float *pw = p.power + e0 * p.nch + l;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
    for (int i = 0; i < n; i++) {
      const double v = (double)pw[(long long)i * p.nch];
      if ((x >> i) & 1) s1 += v; else s0 += v;
    }
    t.pw0 = s0;
    t.pw1 = s1;
  }
  sum_store(p.sums + chunk * SUM_WORDS * p.nch + l, p.nch, t, hist6);
}

// a completed run of the record itself: lengths are 64-bit here
__device__ __forceinline__ void stats_complete(crn_channel_stats &R, int st, long long len, int *hist, int stride) {
  if (st) {
    R.n_runs[1]++;
    R.run_sum[1] += len;
    R.run_max[1] = len > R.run_max[1] ? len : R.run_max[1];
  } else {
    R.n_runs[0]++;
    R.run_sum[0] += len;
    R.run_max[0] = len > R.run_max[0] ? len : R.run_max[0];
    atomicAdd(hist + hist_bin(len) * stride, 1);
  }
}

__global__ __launch_bounds__(64 * JOIN_WAVES) void channels_join_kernel(const TimeParams p) {
  __shared__ int hist[16][64];                       // completed idle runs of this call, per channel
  __shared__ int part[JOIN_WAVES][15][64];           // the waves' summaries: the 15 ints, and the two sums
  __shared__ double part_pw[JOIN_WAVES][2][64];
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const long long stream = p.first + blockIdx.x;
  for (int i = threadIdx.x; i < 16 * 64; i += blockDim.x) (&hist[0][0])[i] = 0;
  __syncthreads();

  // this wave's share of the stream's chunks, folded left to right
  TimeSum t = sum_empty();
  if (l < p.nch) {
    const int per = (p.chunks + nw - 1) / nw;
    const int c0 = wv * per, c1 = c0 + per < p.chunks ? c0 + per : p.chunks;
    for (int c = c0; c < c1; c++) {
      uint64_t hist6;
      const TimeSum b = sum_load(p.sums + (stream * p.chunks + c) * SUM_WORDS * p.nch + l, p.nch, &hist6);
#pragma unroll
      for (int k = 0; k < 6; k++) {
        const int cnt = (int)((hist6 >> (8 * k)) & 255);
        if (cnt) atomicAdd(&hist[k][l], cnt);
      }
      t = sum_join(t, b, &hist[0][l], 64);
    }
  }
  {
    const int v[15] = {t.n, t.nb, t.first, t.last, t.head, t.tail, t.t01, t.t10, t.t11, t.nr0, t.nr1, t.rs0, t.rs1, t.rm0, t.rm1};
#pragma unroll
    for (int f = 0; f < 15; f++) part[wv][f][l] = v[f];
    part_pw[wv][0][l] = t.pw0;
    part_pw[wv][1][l] = t.pw1;
  }
  __syncthreads();
  if (wv != 0 || l >= p.nch) return;
  // (only wave 0 goes on: its LDS adds below follow every other wave's, which the barrier ordered)
  for (int k = 1; k < nw; k++) {
    TimeSum b;
    b.n = part[k][0][l];
    b.nb = part[k][1][l];
    b.first = part[k][2][l];
    b.last = part[k][3][l];
    b.head = part[k][4][l];
    b.tail = part[k][5][l];
    b.t01 = part[k][6][l];
    b.t10 = part[k][7][l];
    b.t11 = part[k][8][l];
    b.nr0 = part[k][9][l];
    b.nr1 = part[k][10][l];
    b.rs0 = part[k][11][l];
    b.rs1 = part[k][12][l];
    b.rm0 = part[k][13][l];
    b.rm1 = part[k][14][l];
    b.pw0 = part_pw[k][0][l];
    b.pw1 = part_pw[k][1][l];
    t = sum_join(t, b, &hist[0][l], 64);
  }

  // the carried record is the leftmost operand
  crn_channel_stats *at = p.stats + stream * p.nch + l;
  crn_channel_stats R;
  if (p.fresh) {
    R = crn_channel_stats{};
  } else {
    R = *at;
  }
  const bool t_whole = t.head == t.n;
  if (R.n_epochs > 0) {
    const int a = R.state & 1;
    if (a == t.first) {
      if (a) R.n_trans[1][1]++; else R.n_trans[0][0]++;
      if (t_whole) {
        R.run += t.n;
      } else {
        stats_complete(R, a, R.run + t.head, &hist[0][l], 64);
        R.run = t.tail;
      }
    } else {
      if (a) R.n_trans[1][0]++; else R.n_trans[0][1]++;
      stats_complete(R, a, R.run, &hist[0][l], 64);
      if (t_whole) {
        R.run = t.n;
      } else {
        stats_complete(R, t.first, t.head, &hist[0][l], 64);
        R.run = t.tail;
      }
    }
  } else if (t_whole) {
    R.run += t.n;
  } else {
    stats_complete(R, t.first, R.run + t.head, &hist[0][l], 64);
    R.run = t.tail;
  }
  R.n_trans[0][0] += t.n - 1 - t.t01 - t.t10 - t.t11;
  R.n_trans[0][1] += t.t01;
  R.n_trans[1][0] += t.t10;
  R.n_trans[1][1] += t.t11;
  R.n_runs[0] += t.nr0;
  R.n_runs[1] += t.nr1;
  R.run_sum[0] += t.rs0;
  R.run_sum[1] += t.rs1;
  R.run_max[0] = t.rm0 > R.run_max[0] ? t.rm0 : R.run_max[0];
  R.run_max[1] = t.rm1 > R.run_max[1] ? t.rm1 : R.run_max[1];
  R.state = t.last;
  R.n_epochs += t.n;
  R.n_busy += t.nb;
  R.power[0] += t.pw0;
  R.power[1] += t.pw1;
#pragma unroll
  for (int k = 0; k < 16; k++) R.idle_hist[k] += hist[k][l];
  *at = R;
}

// Why q cannot serve n_epochs epochs, as the text that follows the entry point's name, or null when it can.  fft_len 0: not known (the
// size function has no handle), and a span is then held to the largest fft_len.
const char *channel_params_refusal(const crn_channel_params &q, int64_t n_epochs, int fft_len = 0) {
  const int n = fft_len > 0 ? fft_len : MAX_N;
  if (n_epochs < 0) return "n_epochs < 0";
  if (q.n_channels < 1 || q.n_channels > CRN_MAX_CHANNELS) return "n_channels must be in 1..64";
  if (q.epochs_per_stream < 1 || n_epochs % q.epochs_per_stream != 0) return "epochs_per_stream must be >= 1 and divide n_epochs";
  if (q.min_bins < 1) return "min_bins < 1";
  for (int r : q.reserved)
    if (r != 0) return "reserved must be 0";
  for (int c = 0; c < q.n_channels; c++)
    if (q.span[c].lo < 0 || q.span[c].lo >= n || q.span[c].width < 1 || q.span[c].width > n) return "a span needs lo in 0..fft_len - 1 and width in 1..fft_len";
  return nullptr;
}

// the workspace: busy words, powers, chunk summaries, each from an 8-byte boundary
struct Layout {
  int64_t busy, power, sums, bytes, chunks;   // offsets; chunks per stream
};
Layout layout_of(int64_t n_epochs, const crn_channel_params &q) {
  Layout y;
  y.chunks = chunks_per_stream(q.epochs_per_stream);
  const int64_t n_streams = n_epochs / q.epochs_per_stream;
  y.busy = 0;
  y.power = n_epochs * 8;
  y.sums = y.power + ((n_epochs * q.n_channels * 4 + 7) & ~int64_t(7));
  y.bytes = y.sums + n_streams * y.chunks * SUM_WORDS * q.n_channels * 4;
  if (y.bytes < 64) y.bytes = 64;
  return y;
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_channels_device: ") + why); }

template <int B>
hipError_t launch_epochs(const ChanParams &p, unsigned n, hipStream_t stream) {
  hipLaunchKernelGGL(channels_epoch_kernel<B>, dim3(n), dim3(64), 0, stream, p);
  return hipGetLastError();
}

}  // namespace
}  // namespace crn

int64_t crn_channels_workspace_bytes(int64_t n_epochs, const crn_channel_params *params) {
  if (!params || crn::channel_params_refusal(*params, n_epochs)) return -1;
  return crn::layout_of(n_epochs, *params).bytes;
}

int crn_channels_device(crn_handle *h, const uint32_t *d_bin_mask, const float *d_spectrum, int64_t n_epochs, const crn_channel_params *params,
                        crn_channel_stats *d_stats, uint64_t *d_busy, float *d_power, void *d_workspace, int64_t workspace_bytes, void *stream) {
  static_assert(sizeof(crn_channel_span) == 8 && sizeof(crn_channel_params) == 544 && sizeof(crn_channel_stats) == 192, "include/crn_sense.h");
  if (!h || !params || !d_bin_mask || !d_stats || !d_workspace) return crn::refuse("null handle / params / mask / stats / workspace");
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  if (const char *why = crn::channel_params_refusal(*params, n_epochs, n)) return crn::refuse(why);
  if (d_power && !d_spectrum) return crn::refuse("d_power needs d_spectrum");
  if (crn::misaligned(d_bin_mask, 8) || crn::misaligned(d_busy, 8) || crn::misaligned(d_workspace, 8))
    return crn::refuse("d_bin_mask, d_busy and d_workspace must be 8-byte aligned");
  if (crn::misaligned(d_spectrum, 16) || crn::misaligned(d_stats, 16) || crn::misaligned(d_power, 16))
    return crn::refuse("d_spectrum, d_stats and d_power must be 16-byte aligned");
  const crn::Layout y = crn::layout_of(n_epochs, *params);
  if (workspace_bytes < y.bytes) return crn::refuse("workspace too small (crn_channels_workspace_bytes)");
  if (n_epochs == 0) return CRN_OK;

  char *ws = static_cast<char *>(d_workspace);
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  crn::ChanParams p;
  p.mask = d_bin_mask;
  p.spectrum = d_spectrum;
  p.busy = d_busy ? d_busy : reinterpret_cast<uint64_t *>(ws + y.busy);
  p.power = !d_spectrum ? nullptr : d_power ? d_power : reinterpret_cast<float *>(ws + y.power);
  p.nch = params->n_channels;
  p.min_bins = params->min_bins;
  for (int c = 0; c < CRN_MAX_CHANNELS; c++) p.span[c] = c < p.nch ? params->span[c] : crn_channel_span{0, 1};
  err = crn::in_grids(err, n_epochs, [&](int64_t first, unsigned cnt) {
    p.first = first;
    return n == 512 ? crn::launch_epochs<8>(p, cnt, st) : n == 1024 ? crn::launch_epochs<16>(p, cnt, st)
           : n == 2048 ? crn::launch_epochs<32>(p, cnt, st) : crn::launch_epochs<64>(p, cnt, st);
  });
  const int64_t n_streams = n_epochs / params->epochs_per_stream;
  crn::TimeParams t{p.busy, p.power, reinterpret_cast<int *>(ws + y.sums), d_stats, 0, p.nch, params->epochs_per_stream, (int)y.chunks,
                    params->first != 0};
  err = crn::in_grids(err, n_streams * y.chunks, [&](int64_t first, unsigned cnt) {
    t.first = first;
    hipLaunchKernelGGL(crn::channels_time_kernel, dim3(cnt), dim3(64), 0, st, t);
    return hipGetLastError();
  });
  const int waves = y.chunks < crn::JOIN_WAVES ? (int)y.chunks : crn::JOIN_WAVES;
  err = crn::in_grids(err, n_streams, [&](int64_t first, unsigned cnt) {
    t.first = first;
    hipLaunchKernelGGL(crn::channels_join_kernel, dim3(cnt), dim3(64 * waves), 0, st, t);
    return hipGetLastError();
  });
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_channels_device: ") + hipGetErrorString(err));
  return CRN_OK;
}

int crn_channel_forecast(const crn_channel_stats *s, int32_t horizon, double prior, double *p01, double *p10, double *p_idle) {
  if (!s) return crn::fail(CRN_ERR_ARG, "crn_channel_forecast: null record");
  if (horizon < 1) return crn::fail(CRN_ERR_ARG, "crn_channel_forecast: horizon < 1");
  if (!(prior >= 0.0) || !std::isfinite(prior)) return crn::fail(CRN_ERR_ARG, "crn_channel_forecast: prior must be finite and >= 0");
  auto leave = [&](int a) {
    const double den = (double)s->n_trans[a][0] + (double)s->n_trans[a][1] + 2.0 * prior;
    return den > 0.0 ? ((double)s->n_trans[a][1 - a] + prior) / den : 0.5;
  };
  const double q01 = leave(0), q10 = leave(1);
  if (p01) *p01 = q01;
  if (p10) *p10 = q10;
  if (p_idle) *p_idle = (s->state & 1) ? q10 * std::pow(1.0 - q01, horizon - 1) : std::pow(1.0 - q01, horizon);
  return CRN_OK;
}
