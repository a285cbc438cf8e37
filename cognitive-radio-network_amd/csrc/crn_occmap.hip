// crn_occmap.hip — the occupancy map (crn_occmap_device, include/crn_sense.h): the CFAR bit mask and, optionally, the `spectrum` rows of
// a batch become one 64-byte record per stream and BIN that the caller carries from call to call: busy count, transitions, the run in
// progress and the longest completed runs, max hold and min hold, and the fp64 power sums while idle and while busy.  A reduction over
// time, one column per bin, parallel across chunks of a stream through an associative summary (the pattern of crn_channels.hip's
// TimeSum and sum_join, here for fft_len columns).  Three launches on the caller's stream, all scratch in the caller's workspace:
//
//   1. chunk   occmap_chunk_kernel<SPEC>, one wave per stream x tile of 256 adjacent bins x chunk of CHUNK = 64 epochs.  Lane l owns the
//              bins 4 l .. 4 l + 3 of the tile: a row costs the wave one coalesced 16-byte load per lane, and a column's epochs come one
//              row after the other.  ROWS = 16 rows (and their mask words, one dword per lane, 32 bytes per wave and row) are in flight
//              before the first is used.  Per bin the lane keeps a 64-bit time word (bit t: busy in the chunk's epoch t), umax and umin
//              of the bit patterns and the two fp64 sums; everything else of the summary (counts, first and last state, head and tail
//              run, rises and falls, the longest run completed inside) comes from bit arithmetic on the time word once the rows are
//              through.  A summary is 32 bytes: two packed words, umax, umin, the two sums; it leaves as two 16-byte stores into
//              [chunk][2][N], which the join reads coalesced.
//   2. join    occmap_join_kernel, one workgroup per stream and 64 adjacent bins, lane = bin in each of up to 8 waves, one per 8 chunks: every wave folds a
//              contiguous share of the stream's chunk summaries with the associative sum_join (a, then b right behind it), 8 summaries
//              loaded ahead of the fold (their addresses do not depend on it); the waves' results are folded through LDS, and the
//              carried record, the leftmost operand, takes the total.  A stream of T epochs is T / 64 / 8 / 8 + 8 dependent steps, not
//              T / 64.  The record leaves as four 16-byte stores, the usual mask as one ballot per wave, and the workgroup's share of
//              the header goes to the workspace.
//   3. header  occmap_header_kernel, one wave per stream: lane g takes the share of bins 64 g .. 64 g + 63, a wave reduction, one writer.
// Integer results do not depend on the order work ran in; power[] is an fp64 sum in the fixed order of the chunks and joins.  Every
// index is computed from the launch geometry (row indices of a short last chunk are clamped), none comes from loaded data.  No scratch
// memory, no atomics of any kind, plain vector stores.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_segments.h"

namespace crn {
namespace {

constexpr int TILE = 256;        // bins of a chunk workgroup: 64 lanes x 4
constexpr int ROWS = 16;         // rows in flight in the chunk kernel
constexpr int GROUP = 64;        // bins of a join workgroup: one per lane
constexpr int JOIN_WAVES = 8;    // shares of a stream's chunks folded side by side
constexpr int AHEAD = 8;         // summaries loaded ahead of the fold
constexpr int SUM_VECS = 2;      // 16-byte vectors of a stored summary
constexpr long long SAT = 2147483647ll;

// What a stretch of one bin's epochs comes to.  head: the run that touches its first epoch, tail: the one that touches its last; a
// stretch of one run has head = tail = n and nothing completed.  rm0, rm1: the longest idle / busy run that begins and ends inside.
struct BinSum {
  int n, nb;
  int first, last;
  int head, tail;
  int rise, fall;
  int rm0, rm1;
  uint32_t umax, umin;
  double pw0, pw1;
};

__device__ __forceinline__ BinSum sum_empty() { return BinSum{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0u, 0u, 0.0, 0.0}; }

__device__ __forceinline__ void sum_complete(BinSum &r, int st, int len) {
  if (st) r.rm1 = len > r.rm1 ? len : r.rm1;
  else r.rm0 = len > r.rm0 ? len : r.rm0;
}

// a, then b right behind it.  Associative; runs that the seam completes are counted here.  (The stretches of one call add up to at most
// 2^31 - 1 epochs: int arithmetic does not overflow.)
__device__ __forceinline__ BinSum sum_join(const BinSum &a, const BinSum &b) {
  if (a.n == 0) return b;
  if (b.n == 0) return a;
  BinSum r = a;
  r.n = a.n + b.n;
  r.nb = a.nb + b.nb;
  r.last = b.last;
  r.rise = a.rise + b.rise + (a.last == 0 && b.first == 1);
  r.fall = a.fall + b.fall + (a.last == 1 && b.first == 0);
  r.rm0 = b.rm0 > a.rm0 ? b.rm0 : a.rm0;
  r.rm1 = b.rm1 > a.rm1 ? b.rm1 : a.rm1;
  r.umax = b.umax > a.umax ? b.umax : a.umax;
  r.umin = b.umin < a.umin ? b.umin : a.umin;
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
      sum_complete(r, a.last, a.tail + b.head);
      r.tail = b.tail;
    }
  } else {
    if (!a_whole) sum_complete(r, a.last, a.tail);
    if (b_whole) {
      r.tail = b.n;
    } else {
      sum_complete(r, b.first, b.head);
      r.tail = b.tail;
    }
  }
  return r;
}

// two fp64 sums as one 16-byte vector, and a sum back from its two words
__device__ __forceinline__ uint4 two_doubles(double p, double q) {
  const unsigned long long a = (unsigned long long)__double_as_longlong(p), b = (unsigned long long)__double_as_longlong(q);
  return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
}
__device__ __forceinline__ double two_words(uint32_t lo, uint32_t hi) { return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo)); }

// a chunk's summary in 32 bytes: n, nb, head, tail <= 64 (7 bits each), first, last; rise, fall <= 32 (6 bits), rm0, rm1 <= 62 (7 bits)
__device__ __forceinline__ void sum_pack(const BinSum &t, uint4 *v0, uint4 *v1) {
  v0->x = (uint32_t)t.n | (uint32_t)t.nb << 7 | (uint32_t)t.head << 14 | (uint32_t)t.tail << 21 | (uint32_t)t.first << 28 | (uint32_t)t.last << 29;
  v0->y = (uint32_t)t.rise | (uint32_t)t.fall << 6 | (uint32_t)t.rm0 << 12 | (uint32_t)t.rm1 << 19;
  v0->z = t.umax;
  v0->w = t.umin;
  *v1 = two_doubles(t.pw0, t.pw1);
}

__device__ __forceinline__ BinSum sum_unpack(const uint4 &v0, const uint4 &v1) {
  BinSum t;
  t.n = (int)(v0.x & 127);
  t.nb = (int)(v0.x >> 7 & 127);
  t.head = (int)(v0.x >> 14 & 127);
  t.tail = (int)(v0.x >> 21 & 127);
  t.first = (int)(v0.x >> 28 & 1);
  t.last = (int)(v0.x >> 29 & 1);
  t.rise = (int)(v0.y & 63);
  t.fall = (int)(v0.y >> 6 & 63);
  t.rm0 = (int)(v0.y >> 12 & 127);
  t.rm1 = (int)(v0.y >> 19 & 127);
  t.umax = v0.z;
  t.umin = v0.w;
  t.pw0 = two_words(v1.x, v1.y);
  t.pw1 = two_words(v1.z, v1.w);
  return t;
}

// the summary of n epochs, 1 <= n <= 64, from the time word x (bit t: busy in epoch t; bits at and above n are 0)
__device__ __forceinline__ BinSum sum_of_word(uint64_t x, int n) {
  BinSum t = sum_empty();
  const uint64_t pairs = (1ull << (n - 1)) - 1;                    // bit i: the pair of epochs i, i + 1 exists
  t.n = n;
  t.nb = __popcll(x);
  t.first = (int)(x & 1);
  t.last = (int)((x >> (n - 1)) & 1);
  t.rise = __popcll(~x & (x >> 1) & pairs);
  t.fall = __popcll(x & ~(x >> 1) & pairs);
  const uint64_t flips = (x ^ (x >> 1)) & pairs;                   // bit i: epochs i and i + 1 differ
  if (flips == 0) {
    t.head = t.tail = n;
  } else {
    t.head = __builtin_ctzll(flips) + 1;
    t.tail = n - 1 - (63 - __builtin_clzll(flips));
    // the runs between the first and the last flip
    uint64_t rest = flips & (flips - 1);
    int start = t.head, st = t.first ^ 1;
    while (rest) {
      const int nxt = __builtin_ctzll(rest) + 1;
      sum_complete(t, st, nxt - start);
      start = nxt;
      st ^= 1;
      rest &= rest - 1;
    }
  }
  return t;
}

__device__ __forceinline__ int sat(long long v) { return (int)(v < SAT ? v : SAT); }

// The record as the call leaves it: the carried record (its four 16-byte vectors; all zero for a fresh start), the leftmost operand, takes
// the summary t of the call's epochs, t.n >= 1.  Sums run in 64 bits and are clamped once: sat(sat(x + a) + b) = sat(x + a + b).
struct Record {
  uint4 q[4];
};
__device__ __forceinline__ Record record_join(uint4 r0, uint4 r1, uint4 r2, uint4 r3, const BinSum &t) {
  const bool carried = (int)r0.x > 0;
  if (!carried) r0 = r1 = r2 = r3 = make_uint4(0u, 0u, 0u, 0u);   // n_epochs <= 0: taken as all zero
  long long n_epochs = (int)r0.x, n_busy = (int)r0.y, n_rise = (int)r0.z, n_fall = (int)r0.w;
  long long run = (int)r1.x > 0 ? (int)r1.x : 0;
  int rm[2] = {(int)r1.z, (int)r1.w};
  uint32_t max_hold = r2.x, min_hold = r2.y;
  const bool t_whole = t.head == t.n;
  auto complete = [&](int st, long long len) {
    const int v = sat(len);
    if (st) rm[1] = v > rm[1] ? v : rm[1];
    else rm[0] = v > rm[0] ? v : rm[0];
  };
  if (carried) {
    const int a = (int)(r1.y & 1u);
    if (a == t.first) {
      if (t_whole) {
        run += t.n;
      } else {
        complete(a, run + t.head);
        run = t.tail;
      }
    } else {
      if (a) n_fall++; else n_rise++;
      complete(a, run);
      if (t_whole) {
        run = t.n;
      } else {
        complete(t.first, t.head);
        run = t.tail;
      }
    }
    max_hold = t.umax > max_hold ? t.umax : max_hold;
    min_hold = t.umin < min_hold ? t.umin : min_hold;
  } else {
    if (t_whole) {
      run = t.n;
    } else {
      complete(t.first, t.head);
      run = t.tail;
    }
    max_hold = t.umax;
    min_hold = t.umin;
  }
  if (t.rm0 > 0) rm[0] = t.rm0 > rm[0] ? t.rm0 : rm[0];   // (0: no run completed inside, and the record's figure stays whatever it is)
  if (t.rm1 > 0) rm[1] = t.rm1 > rm[1] ? t.rm1 : rm[1];
  const int ne = sat(n_epochs + t.n), nb = sat(n_busy + t.nb);
  Record R;
  R.q[0] = make_uint4((uint32_t)ne, (uint32_t)nb, (uint32_t)sat(n_rise + t.rise), (uint32_t)sat(n_fall + t.fall));
  R.q[1] = make_uint4((uint32_t)sat(run), (uint32_t)t.last, (uint32_t)rm[0], (uint32_t)rm[1]);
  R.q[2] = make_uint4(max_hold, min_hold, 0u, 0u);
  R.q[3] = two_doubles(two_words(r3.x, r3.y) + t.pw0, two_words(r3.z, r3.w) + t.pw1);
  return R;
}

struct ChunkParams {
  const uint32_t *mask;     // [n_epochs][N / 32]
  const float *spectrum;    // [n_epochs][N] or null
  uint4 *sums;              // [n_streams * chunks][SUM_VECS][N]
  long long first;          // workgroup 0 of this grid, of (n_streams * chunks) x tiles
  int N, eps, chunks, tiles;
};

template <bool SPEC>
__global__ __launch_bounds__(64) void occmap_chunk_kernel(const ChunkParams p) {
  const int l = threadIdx.x;
  const long long wg = p.first + blockIdx.x;
  const long long chunk = wg / p.tiles;
  const int tile = (int)(wg - chunk * p.tiles);
  const ChunkSpan cs = chunk_span(chunk, p.chunks, p.eps);
  const int n = cs.n;
  const long long e0 = cs.stream * p.eps + cs.t0;
  const int bin = tile * TILE + 4 * l;
  const int words = p.N >> 5;
  const uint32_t *mrow = p.mask + e0 * words + (bin >> 5);
  const int sh = bin & 31;
  const float *srow = SPEC ? p.spectrum + e0 * p.N + bin : nullptr;

  uint64_t x[4] = {0, 0, 0, 0};
  uint32_t hi[4] = {0u, 0u, 0u, 0u}, lo[4] = {SPEC ? ~0u : 0u, SPEC ? ~0u : 0u, SPEC ? ~0u : 0u, SPEC ? ~0u : 0u};
  double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int g = 0; g < CHUNK; g += ROWS) {
    if (g < n) {                                  // (uniform over the wave)
      uint32_t w[ROWS];
      float4 v[ROWS];
      // the group's loads, all of them before the first use; a row past the chunk's end is the chunk's last row again, and not used
#pragma unroll
      for (int i = 0; i < ROWS; i++) {
        const long long t = g + i < n ? g + i : n - 1;
        w[i] = mrow[t * words];
        if (SPEC) v[i] = *reinterpret_cast<const float4 *>(srow + t * p.N);
      }
#pragma unroll
      for (int i = 0; i < ROWS; i++) {
        if (g + i < n) {
          const uint32_t nib = (w[i] >> sh) & 15u;
          const float f[4] = {SPEC ? v[i].x : 0.f, SPEC ? v[i].y : 0.f, SPEC ? v[i].z : 0.f, SPEC ? v[i].w : 0.f};
#pragma unroll
          for (int b = 0; b < 4; b++) {
            const uint32_t s = (nib >> b) & 1u;
            x[b] |= (uint64_t)s << (g + i);
            if (SPEC) {
              const uint32_t u = __float_as_uint(f[b]);
              hi[b] = u > hi[b] ? u : hi[b];
              lo[b] = u < lo[b] ? u : lo[b];
              // (the other sum takes +0.0, which changes nothing)
              s1[b] += (double)(s ? f[b] : 0.f);
              s0[b] += (double)(s ? 0.f : f[b]);
            }
          }
        }
      }
    }
  }

  uint4 *out = p.sums + chunk * SUM_VECS * p.N + bin;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    BinSum t = sum_of_word(x[b], n);
    t.umax = hi[b];
    t.umin = lo[b];
    t.pw0 = s0[b];
    t.pw1 = s1[b];
    uint4 v0, v1;
    sum_pack(t, &v0, &v1);
    out[b] = v0;
    out[p.N + b] = v1;
  }
}

struct JoinParams {
  const uint4 *sums;            // [n_streams * chunks][SUM_VECS][N]
  crn_occmap_bin *bins;         // [n_streams][N]
  uint32_t *usual;              // [n_streams][N / 32] or null
  uint4 *parts;                 // [n_streams][groups][2]: the join workgroups' shares of the headers
  crn_occmap_stream *streams;   // [n_streams]
  long long first;              // workgroup 0 of this grid
  int N, chunks, groups, fresh, duty_ppm;
};

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int s = 32; s > 0; s /= 2) v += __shfl_xor(v, s, 64);
  return v;
}

__global__ __launch_bounds__(64 * JOIN_WAVES) void occmap_join_kernel(const JoinParams p) {
  __shared__ uint4 part[JOIN_WAVES][4][GROUP];   // the waves' summaries, 64 bytes each
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const long long wg = p.first + blockIdx.x;
  const long long stream = wg / p.groups;
  const int grp = (int)(wg - stream * p.groups);
  const int bin = grp * GROUP + l;

  // this wave's share of the stream's chunks, folded left to right
  BinSum t = sum_empty();
  {
    const int per = (p.chunks + nw - 1) / nw;
    const int c0 = wv * per, c1 = c0 + per < p.chunks ? c0 + per : p.chunks;
    const uint4 *at = p.sums + stream * p.chunks * SUM_VECS * p.N + bin;
    const long long step = (long long)SUM_VECS * p.N;
    for (int c = c0; c < c1; c += AHEAD) {
      uint4 a[AHEAD], b[AHEAD];
#pragma unroll
      for (int i = 0; i < AHEAD; i++) {
        const int cc = c + i < c1 ? c + i : c1 - 1;
        a[i] = at[cc * step];
        b[i] = at[cc * step + p.N];
      }
#pragma unroll
      for (int i = 0; i < AHEAD; i++)
        if (c + i < c1) t = sum_join(t, sum_unpack(a[i], b[i]));
    }
  }
  if (nw > 1) {
    part[wv][0][l] = make_uint4((uint32_t)t.n, (uint32_t)t.nb, (uint32_t)t.head, (uint32_t)t.tail);
    part[wv][1][l] = make_uint4((uint32_t)t.rise, (uint32_t)t.fall, (uint32_t)t.rm0, (uint32_t)t.rm1);
    part[wv][2][l] = make_uint4((uint32_t)(t.first | t.last << 1), t.umax, t.umin, 0u);
    part[wv][3][l] = two_doubles(t.pw0, t.pw1);
    __syncthreads();
    if (wv != 0) return;
    for (int k = 1; k < nw; k++) {
      const uint4 q0 = part[k][0][l], q1 = part[k][1][l], q2 = part[k][2][l], q3 = part[k][3][l];
      BinSum b;
      b.n = (int)q0.x;
      b.nb = (int)q0.y;
      b.head = (int)q0.z;
      b.tail = (int)q0.w;
      b.rise = (int)q1.x;
      b.fall = (int)q1.y;
      b.rm0 = (int)q1.z;
      b.rm1 = (int)q1.w;
      b.first = (int)(q2.x & 1);
      b.last = (int)(q2.x >> 1 & 1);
      b.umax = q2.y;
      b.umin = q2.z;
      b.pw0 = two_words(q3.x, q3.y);
      b.pw1 = two_words(q3.z, q3.w);
      t = sum_join(t, b);
    }
  }

  // the carried record is the leftmost operand; t.n >= 1
  uint4 *at = reinterpret_cast<uint4 *>(p.bins + stream * p.N + bin);
  uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0, r2 = r0, r3 = r0;
  if (!p.fresh) {
    r0 = at[0];
    r1 = at[1];
    r2 = at[2];
    r3 = at[3];
  }
  const Record R = record_join(r0, r1, r2, r3, t);
  const int ne = (int)R.q[0].x, nb = (int)R.q[0].y;
  at[0] = R.q[0];
  at[1] = R.q[1];
  at[2] = R.q[2];
  at[3] = R.q[3];

  // the usual mask by ballot (ne > 0 always: the call added an epoch), and this workgroup's share of the header
  const uint64_t usual = __ballot((long long)nb * 1000000ll >= (long long)p.duty_ppm * ne);
  const uint64_t clear = __ballot(nb == 0), now = __ballot(t.last != 0);
  const long long busy_sum = wave_sum((long long)nb);
  if (l == 0) {
    if (p.usual != nullptr) *reinterpret_cast<uint64_t *>(p.usual + stream * (p.N >> 5) + grp * 2) = usual;
    uint4 *h = p.parts + (stream * p.groups + grp) * 2;
    h[0] = make_uint4((uint32_t)(unsigned long long)busy_sum, (uint32_t)((unsigned long long)busy_sum >> 32), (uint32_t)ne, (uint32_t)__popcll(usual));
    h[1] = make_uint4((uint32_t)__popcll(clear), (uint32_t)__popcll(now), 0u, 0u);
  }
}

__global__ __launch_bounds__(64) void occmap_header_kernel(const JoinParams p) {
  const int l = threadIdx.x;
  const long long stream = p.first + blockIdx.x;
  uint4 h0 = make_uint4(0u, 0u, 0u, 0u), h1 = h0;
  if (l < p.groups) {
    const uint4 *h = p.parts + (stream * p.groups + l) * 2;
    h0 = h[0];
    h1 = h[1];
  }
  const long long busy_sum = wave_sum((long long)((unsigned long long)h0.y << 32 | h0.x));
  const long long counts = wave_sum((long long)h0.w | (long long)h1.x << 20 | (long long)h1.y << 40);   // three counts <= 4096 each
  const int ne = __shfl((int)h0.z, 0, 64);                                                                // that of bin 0
  if (l == 0) {
    uint4 *at = reinterpret_cast<uint4 *>(p.streams + stream);
    at[0] = make_uint4((uint32_t)(unsigned long long)busy_sum, (uint32_t)((unsigned long long)busy_sum >> 32), (uint32_t)ne, (uint32_t)(counts & 0xfffff));
    at[1] = make_uint4((uint32_t)(counts >> 20 & 0xfffff), (uint32_t)(counts >> 40 & 0xfffff), 0u, 0u);
  }
}

// Why q cannot serve n_epochs epochs, as the text that follows the entry point's name, or null when it can.
const char *occmap_params_refusal(const crn_occmap_params &q, int64_t n_epochs) {
  if (n_epochs < 0) return "n_epochs < 0";
  if (q.epochs_per_stream < 1 || n_epochs % q.epochs_per_stream != 0) return "epochs_per_stream must be >= 1 and divide n_epochs";
  if (q.duty_ppm < 1 || q.duty_ppm > 1000000) return "duty_ppm must be in 1..1000000";
  for (int r : q.reserved)
    if (r != 0) return "reserved must be 0";
  return nullptr;
}

// the workspace: the join workgroups' shares of the headers, then the chunk summaries; both hold 16-byte vectors.  fft_len 0: not known
// (the size function has no handle), and the size is then that of the largest fft_len.
struct Layout {
  int64_t parts, sums, bytes, chunks;   // offsets; chunks per stream
};
Layout layout_of(int64_t n_epochs, const crn_occmap_params &q, int fft_len = 0) {
  const int64_t n = fft_len > 0 ? fft_len : MAX_N;
  Layout y;
  y.chunks = chunks_per_stream(q.epochs_per_stream);
  const int64_t n_streams = n_epochs / q.epochs_per_stream;
  y.parts = 0;
  y.sums = n_streams * (n / GROUP) * 2 * 16;
  y.bytes = y.sums + n_streams * y.chunks * SUM_VECS * n * 16;
  if (y.bytes < 64) y.bytes = 64;
  return y;
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_occmap_device: ") + why); }

}  // namespace
}  // namespace crn

int64_t crn_occmap_workspace_bytes(int64_t n_epochs, const crn_occmap_params *params) {
  if (!params || crn::occmap_params_refusal(*params, n_epochs)) return -1;
  return crn::layout_of(n_epochs, *params).bytes;
}

int crn_occmap_device(crn_handle *h, const uint32_t *d_bin_mask, const float *d_spectrum, int64_t n_epochs, const crn_occmap_params *params,
                      crn_occmap_bin *d_bins, crn_occmap_stream *d_streams, uint32_t *d_usual_mask, void *d_workspace, int64_t workspace_bytes,
                      void *stream) {
  static_assert(sizeof(crn_occmap_params) == 32 && sizeof(crn_occmap_bin) == 64 && sizeof(crn_occmap_stream) == 32, "include/crn_sense.h");
  if (!h || !params || !d_bin_mask || !d_bins || !d_streams || !d_workspace) return crn::refuse("null handle / params / mask / bins / streams / workspace");
  if (const char *why = crn::occmap_params_refusal(*params, n_epochs)) return crn::refuse(why);
  if (crn::misaligned(d_bin_mask, 8) || crn::misaligned(d_usual_mask, 8)) return crn::refuse("d_bin_mask and d_usual_mask must be 8-byte aligned");
  if (crn::misaligned(d_spectrum, 16) || crn::misaligned(d_bins, 16) || crn::misaligned(d_streams, 16) || crn::misaligned(d_workspace, 16))
    return crn::refuse("d_spectrum, d_bins, d_streams and d_workspace must be 16-byte aligned");
  if (workspace_bytes < crn::layout_of(n_epochs, *params).bytes) return crn::refuse("workspace too small (crn_occmap_workspace_bytes)");
  if (n_epochs == 0) return CRN_OK;

  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  const crn::Layout y = crn::layout_of(n_epochs, *params, n);   // (this fft_len's offsets: no larger than what was checked)
  char *ws = static_cast<char *>(d_workspace);
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n_streams = n_epochs / params->epochs_per_stream;
  crn::ChunkParams c{d_bin_mask, d_spectrum, reinterpret_cast<uint4 *>(ws + y.sums), 0, n, params->epochs_per_stream, (int)y.chunks, n / crn::TILE};
  err = crn::in_grids(err, n_streams * y.chunks * c.tiles, [&](int64_t first, unsigned cnt) {
    c.first = first;
    if (d_spectrum) hipLaunchKernelGGL(crn::occmap_chunk_kernel<true>, dim3(cnt), dim3(64), 0, st, c);
    else hipLaunchKernelGGL(crn::occmap_chunk_kernel<false>, dim3(cnt), dim3(64), 0, st, c);
    return hipGetLastError();
  });
  crn::JoinParams j{c.sums, d_bins, d_usual_mask, reinterpret_cast<uint4 *>(ws + y.parts), d_streams, 0, n, (int)y.chunks, n / crn::GROUP,
                    params->first != 0, params->duty_ppm};
  // (a wave has AHEAD summaries in flight: a stream of up to AHEAD chunks is one round of loads for one wave, and needs no second one)
  const int64_t rounds = (y.chunks + crn::AHEAD - 1) / crn::AHEAD;
  const int waves = rounds < crn::JOIN_WAVES ? (int)rounds : crn::JOIN_WAVES;
  err = crn::in_grids(err, n_streams * j.groups, [&](int64_t first, unsigned cnt) {
    j.first = first;
    hipLaunchKernelGGL(crn::occmap_join_kernel, dim3(cnt), dim3(64 * waves), 0, st, j);
    return hipGetLastError();
  });
  err = crn::in_grids(err, n_streams, [&](int64_t first, unsigned cnt) {
    j.first = first;
    hipLaunchKernelGGL(crn::occmap_header_kernel, dim3(cnt), dim3(64), 0, st, j);
    return hipGetLastError();
  });
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_occmap_device: ") + hipGetErrorString(err));
  return CRN_OK;
}
