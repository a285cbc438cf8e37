// crn_hops.hip — channel-to-channel transition counts over time (crn_hops_device, crn_hop_forecast, include/crn_sense.h): the busy words
// of a batch, one per epoch as crn_channels_device writes them, become one record per stream that the caller carries from call to call:
// the moves between channels (hop) and, per lag, how often channel j was busy lag epochs after channel i was (pair, with its row and
// column totals from and to).  State 63 stands for "nothing busy".  Integers only; two launches on the caller's stream, all scratch in
// the caller's workspace:
//
//   1. chunk  hops_chunk_kernel, one wave per stream x part x matrix (hop, or the pair matrix of one lag).  A part is a contiguous run of
//             the stream's chunks of CHUNK = 64 epochs.  Per chunk lane t loads word t, augments it, and 64 ballots turn the 64 words into
//             per-channel time words (lane c: bit t = channel c busy in the chunk's epoch t; the manner of channels_time_kernel).  A lane
//             keeps its channel's time word of the chunk before (at the stream's first chunk: the carried hist, bit-reversed, or nothing),
//             so the time word d epochs earlier is (cur << d) | (prev >> (64 - d)) for every lag d in 1..64 alike.  Lane j holds column j
//             of the matrix in 64 registers; row i's word comes from lane i as a broadcast (i is a compile-time constant), and the
//             increment is popcount(row_i & col_j), the column word already masked to the epochs that have an epoch d before them.
//             from and to are popcounts of the same words; for hop the row word is prev & ~cur (fall) and the column word cur & ~prev
//             (rise).  The part's matrix goes to the workspace row by row, 256 contiguous bytes a row.  The wave of matrix 0, part 0 also
//             leaves the verdict on the carried record (taken as empty or not, and its n_epochs) in the workspace: the join must not judge
//             a head that one of its own workgroups is rewriting.
//   2. join   hops_join_kernel, one workgroup of 256 per stream x matrix x quarter of the matrix's rows: every thread owns four cells, has the
//             cells of 8 parts in flight, adds the parts in ascending order to the carried count in 64 bits and stores the sum clamped to
//             2^31 - 1.  The workgroup of a
//             lag's first quarter does the same for from and to; wave 0 of the hop matrix's first quarter writes the head and shifts the
//             call's last epochs into hist (one more transposition by ballots).
// Sums of non-negative integers clamped once: the result does not depend on the order work ran in or on how a stream is cut into calls.
// Every index comes from the launch geometry (the word index of a short last chunk is clamped); none comes from loaded data.  No scratch
// memory, no atomics, one writer per word, plain vector stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "crn_internal.h"
#include "crn_segments.h"

namespace crn {
namespace {

constexpr int MAX_LAGS = 8;
constexpr int IDLE = 63;                      // the virtual channel "nothing busy"
constexpr int PART_CHUNKS = 4;                // chunks of a part, as long as a stream has no more than MAX_PARTS parts
constexpr int MAX_PARTS = 64;                 // parts of a stream: bounds the workspace of a long stream
constexpr int QUARTERS = 4;                   // join workgroups per matrix: 16 rows each
constexpr int JOIN_THREADS = 256;
constexpr int AHEAD = 8;                      // parts whose cells a join thread has in flight
constexpr int64_t HEAD_BYTES = 64, HIST_BYTES = 512, MAT_BYTES = 16384, LAG_BYTES = 512 + MAT_BYTES;
constexpr int SLOT_WORDS = 128 + 4096;        // a part's share of one matrix in the workspace: from[64], to[64], the matrix; 4-byte words
constexpr int64_t VERDICT_BYTES = 16;         // per stream: carried (0 / 1) and its n_epochs, two 8-byte words
constexpr long long SAT = 2147483647ll;

inline int64_t record_bytes_of(int n_lags) { return HEAD_BYTES + HIST_BYTES + MAT_BYTES + int64_t(n_lags) * LAG_BYTES; }

__device__ __forceinline__ uint64_t below(int n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1; }   // bits 0 .. n - 1

__device__ __forceinline__ uint64_t augment(uint64_t w, int nch) {
  const uint64_t a = w & below(nch);
  return a ? a : 1ull << IDLE;
}

// 64 words, one per lane, to 64 time words, one per lane: bit t of lane c's result is bit c of lane t's word.  Augmented words have
// bits at the channels below nch and at IDLE only.
__device__ __forceinline__ uint64_t transpose(uint64_t a, int nch, int l) {
  uint64_t x = 0;
  for (int c = 0; c < nch; c++) {
    const uint64_t col = __ballot((a >> c) & 1);
    if (l == c) x = col;
  }
  const uint64_t col = __ballot((a >> IDLE) & 1);
  if (l == IDLE) x = col;
  return x;
}

__device__ __forceinline__ uint64_t from_lane(uint64_t v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return (uint64_t)hi << 32 | lo;
}

struct HopKernelParams {
  const uint64_t *busy;     // [n_epochs]
  char *records;            // [n_streams] records of record_bytes each
  long long *verdict;       // [n_streams][2], in the workspace
  int *slots;               // [n_streams][parts][1 + n_lags][SLOT_WORDS], in the workspace
  long long record_bytes;
  long long first;          // workgroup 0 of this grid
  int nch, n_lags, eps, chunks, per, parts, fresh;
  int lag[MAX_LAGS];        // entries at and above n_lags are 0
};

// Is the carried record of this stream one of this call's kind?  Its n_epochs if so, else 0.  (Every lane reads the same 64 bytes.)
__device__ __forceinline__ long long carried_epochs(const HopKernelParams &p, const char *rec) {
  if (p.fresh) return 0;
  const int *head = reinterpret_cast<const int *>(rec);
  const long long t = *reinterpret_cast<const long long *>(rec);
  bool same = t > 0 && head[2] == p.nch && head[3] == p.n_lags;
#pragma unroll
  for (int m = 0; m < MAX_LAGS; m++) same = same && head[4 + m] == p.lag[m];
  return same ? t : 0;
}

// hist word of channel l as the rule reads it: only the epochs seen, only the channel positions
__device__ __forceinline__ uint64_t carried_hist(const HopKernelParams &p, const char *rec, long long t_before, int l) {
  if (t_before <= 0 || !(l < p.nch || l == IDLE)) return 0;
  const uint64_t h = reinterpret_cast<const uint64_t *>(rec + HEAD_BYTES)[l];
  return h & below(t_before < 64 ? (int)t_before : 64);
}

__global__ __launch_bounds__(64) void hops_chunk_kernel(const HopKernelParams p) {
  const int l = threadIdx.x;
  const int mats = p.n_lags + 1;
  const long long wg = p.first + blockIdx.x;
  const long long stream = wg / ((long long)p.parts * mats);
  const int r = (int)(wg - stream * p.parts * mats);
  const int part = r / mats, mat = r - part * mats;
  int d = 1;
#pragma unroll
  for (int m = 0; m < MAX_LAGS; m++) d = mat == m + 1 ? p.lag[m] : d;
  const char *rec = p.records + stream * p.record_bytes;
  const long long t_before = carried_epochs(p, rec);
  const int seen = t_before < 64 ? (int)t_before : 64;          // all a lag of at most 64 asks about
  if (mat == 0 && part == 0 && l == 0) {
    p.verdict[stream * 2] = t_before > 0;
    p.verdict[stream * 2 + 1] = t_before;
  }

  const int c0 = part * p.per, c1 = c0 + p.per < p.chunks ? c0 + p.per : p.chunks;
  const uint64_t *words = p.busy + stream * p.eps;
  // the chunk before this part's first: the carried history (bit k: k + 1 epochs ago) turned round, or a whole chunk of this call
  uint64_t prev;
  if (c0 == 0) prev = __brevll(carried_hist(p, rec, t_before, l));
  else prev = transpose(augment(words[(long long)(c0 - 1) * CHUNK + l], p.nch), p.nch, l);

  int acc[64];
#pragma unroll
  for (int i = 0; i < 64; i++) acc[i] = 0;
  int n_from = 0, n_to = 0;
  for (int c = c0; c < c1; c++) {
    const int t0 = c * CHUNK;                                    // (chunks * 64 < 2^31 + 64: c * 64 <= eps - 1)
    const int n = p.eps - t0 < CHUNK ? p.eps - t0 : CHUNK;
    const uint64_t w = words[(long long)t0 + (l < n ? l : n - 1)];
    const uint64_t cur = transpose(l < n ? augment(w, p.nch) : 0ull, p.nch, l);
    const uint64_t back = (d < 64 ? cur << d : 0ull) | prev >> (64 - d);   // bit t: this lane's channel, d epochs before the chunk's epoch t
    // epoch t of the chunk has an epoch d before it when seen + t0 + t >= d
    const int lack = t0 >= d ? 0 : d - t0 - seen;
    const uint64_t valid = below(n) & ~below(lack);
    uint64_t row, col;
    if (mat == 0) {
      row = back & ~cur;                                         // left d = 1 epoch before
      col = cur & ~back & valid;                                 // arrived now
    } else {
      row = back;
      col = cur & valid;
      n_from += __popcll(back & valid);
      n_to += __popcll(col);
    }
#pragma unroll
    for (int i = 0; i < 64; i++) acc[i] += __popcll(from_lane(row, i) & col);
    prev = cur;
  }

  int *slot = p.slots + ((stream * p.parts + part) * mats + mat) * SLOT_WORDS;
  slot[l] = n_from;
  slot[64 + l] = n_to;
#pragma unroll
  for (int i = 0; i < 64; i++) slot[128 + i * 64 + l] = acc[i];
}

__device__ __forceinline__ int sat(long long v) { return (int)(v < SAT ? v : SAT); }

__global__ __launch_bounds__(JOIN_THREADS) void hops_join_kernel(const HopKernelParams p) {
  const int t = threadIdx.x;
  const int mats = p.n_lags + 1;
  const long long wg = p.first + blockIdx.x;
  const long long stream = wg / (mats * QUARTERS);
  const int r = (int)(wg - stream * mats * QUARTERS);
  const int mat = r / QUARTERS, quarter = r - mat * QUARTERS;
  const bool carried = p.verdict[stream * 2] != 0;
  const long long t_before = p.verdict[stream * 2 + 1];
  char *rec = p.records + stream * p.record_bytes;
  char *block = rec + HEAD_BYTES + HIST_BYTES + (mat == 0 ? 0 : MAT_BYTES + (long long)(mat - 1) * LAG_BYTES);   // hop, or the lag's from
  const int *src = p.slots + (stream * p.parts * mats + mat) * SLOT_WORDS;
  const long long step = (long long)mats * SLOT_WORDS;

  // the matrix: four cells a thread
  {
    int *dst = reinterpret_cast<int *>(block + (mat == 0 ? 0 : 512)) + quarter * 1024 + t;
    const int *at = src + 128 + quarter * 1024 + t;
    long long s[4] = {0, 0, 0, 0};
    if (carried) {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int v = dst[k * JOIN_THREADS];
        s[k] = v > 0 ? v : 0;
      }
    }
    // AHEAD parts' cells are loaded before the first is added (their addresses do not depend on the sums); a part past the last is the
    // last one again, and not added
    for (int q = 0; q < p.parts; q += AHEAD) {
      int v[AHEAD][4];
#pragma unroll
      for (int i = 0; i < AHEAD; i++) {
        const int qq = q + i < p.parts ? q + i : p.parts - 1;
#pragma unroll
        for (int k = 0; k < 4; k++) v[i][k] = at[qq * step + k * JOIN_THREADS];
      }
#pragma unroll
      for (int i = 0; i < AHEAD; i++) {
        if (q + i < p.parts) {
#pragma unroll
          for (int k = 0; k < 4; k++) s[k] += v[i][k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k * JOIN_THREADS] = sat(s[k]);
  }

  if (quarter != 0) return;
  if (mat != 0) {
    // from[64] and to[64] of this lag, side by side in the record and in a slot
    if (t < 128) {
      int *dst = reinterpret_cast<int *>(block) + t;
      long long s = 0;
      if (carried) {
        const int v = *dst;
        s = v > 0 ? v : 0;
      }
      for (int q = 0; q < p.parts; q++) s += src[q * step + t];
      *dst = sat(s);
    }
    return;
  }
  if (t >= 64) return;

  // the head, and the call's last epochs shifted into hist: lane k takes the word k epochs before the stream's last
  const int m = p.eps < 64 ? p.eps : 64;
  const uint64_t w = p.busy[stream * p.eps + (p.eps - 1 - (t < m ? t : m - 1))];
  const uint64_t x = transpose(t < m ? augment(w, p.nch) : 0ull, p.nch, t);
  const uint64_t old = carried_hist(p, rec, carried ? t_before : 0, t);
  reinterpret_cast<uint64_t *>(rec + HEAD_BYTES)[t] = x | (p.eps < 64 ? old << p.eps : 0ull);
  if (t < 16) {
    const long long room = 9223372036854775807ll - t_before;
    const long long now = p.eps < room ? t_before + p.eps : 9223372036854775807ll;
    int v = t == 0 ? (int)(uint32_t)(unsigned long long)now : t == 1 ? (int)(uint32_t)((unsigned long long)now >> 32) : t == 2 ? p.nch : t == 3 ? p.n_lags : 0;
#pragma unroll
    for (int m = 0; m < MAX_LAGS; m++) v = t == 4 + m ? p.lag[m] : v;
    reinterpret_cast<int *>(rec)[t] = v;
  }
}

// Why q cannot serve, as the text that follows the entry point's name, or null when it can.
const char *hop_params_refusal(const crn_hop_params &q) {
  if (q.n_channels < 1 || q.n_channels > 63) return "n_channels must be in 1..63";
  if (q.epochs_per_stream < 1) return "epochs_per_stream must be >= 1 and divide n_epochs";
  if (q.n_lags < 1 || q.n_lags > MAX_LAGS) return "n_lags must be in 1..8";
  for (int m = 0; m < q.n_lags; m++)
    if (q.lag[m] < 1 || q.lag[m] > 64 || (m > 0 && q.lag[m] <= q.lag[m - 1])) return "lag[] must be strictly ascending, each in 1..64";
  for (int r : q.reserved)
    if (r != 0) return "reserved must be 0";
  return nullptr;
}

// the workspace: the verdicts on the carried records, then the parts' matrices
struct Layout {
  int64_t verdict, slots, bytes, chunks, per, parts;   // offsets; chunks per stream, chunks per part, parts per stream
};
Layout layout_of(int64_t n_epochs, const crn_hop_params &q) {
  Layout y;
  y.chunks = chunks_per_stream(q.epochs_per_stream);
  const int64_t want = (y.chunks + PART_CHUNKS - 1) / PART_CHUNKS;
  y.per = (y.chunks + (want < MAX_PARTS ? want : MAX_PARTS) - 1) / (want < MAX_PARTS ? want : MAX_PARTS);
  y.parts = (y.chunks + y.per - 1) / y.per;             // (none of them empty)
  const int64_t n_streams = n_epochs / q.epochs_per_stream;
  y.verdict = 0;
  y.slots = n_streams * VERDICT_BYTES;
  y.bytes = y.slots + n_streams * y.parts * (q.n_lags + 1) * SLOT_WORDS * 4;
  if (y.bytes < 64) y.bytes = 64;
  return y;
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_hops_device: ") + why); }

}  // namespace
}  // namespace crn

int64_t crn_hops_bytes(int64_t n_streams, const crn_hop_params *params) {
  if (!params || n_streams < 0 || n_streams > (int64_t(1) << 40) || crn::hop_params_refusal(*params)) return -1;   // (2^40 records: no overflow)
  return n_streams * crn::record_bytes_of(params->n_lags);
}

int64_t crn_hops_workspace_bytes(int64_t n_epochs, const crn_hop_params *params) {
  if (!params || n_epochs < 0 || crn::hop_params_refusal(*params) || n_epochs % params->epochs_per_stream != 0) return -1;
  return crn::layout_of(n_epochs, *params).bytes;
}

int crn_hops_device(crn_handle *h, const uint64_t *d_busy, int64_t n_epochs, const crn_hop_params *params, void *d_records, int64_t record_bytes,
                    void *d_workspace, int64_t workspace_bytes, void *stream) {
  static_assert(sizeof(crn_hop_params) == 64, "include/crn_sense.h");
  if (!h || !params || !d_busy || !d_records || !d_workspace) return crn::refuse("null handle / params / busy / records / workspace");
  if (n_epochs < 0) return crn::refuse("n_epochs < 0");
  if (const char *why = crn::hop_params_refusal(*params)) return crn::refuse(why);
  if (n_epochs % params->epochs_per_stream != 0) return crn::refuse("epochs_per_stream must be >= 1 and divide n_epochs");
  if (crn::misaligned(d_busy, 8) || crn::misaligned(d_workspace, 8)) return crn::refuse("d_busy and d_workspace must be 8-byte aligned");
  if (crn::misaligned(d_records, 16)) return crn::refuse("d_records must be 16-byte aligned");
  const int64_t n_streams = n_epochs / params->epochs_per_stream;
  if (record_bytes < n_streams * crn::record_bytes_of(params->n_lags)) return crn::refuse("records too small (crn_hops_bytes)");
  const crn::Layout y = crn::layout_of(n_epochs, *params);
  if (workspace_bytes < y.bytes) return crn::refuse("workspace too small (crn_hops_workspace_bytes)");
  if (n_epochs == 0) return CRN_OK;

  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  char *ws = static_cast<char *>(d_workspace);
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  crn::HopKernelParams p;
  p.busy = d_busy;
  p.records = static_cast<char *>(d_records);
  p.verdict = reinterpret_cast<long long *>(ws + y.verdict);
  p.slots = reinterpret_cast<int *>(ws + y.slots);
  p.record_bytes = crn::record_bytes_of(params->n_lags);
  p.first = 0;
  p.nch = params->n_channels;
  p.n_lags = params->n_lags;
  p.eps = params->epochs_per_stream;
  p.chunks = (int)y.chunks;
  p.per = (int)y.per;
  p.parts = (int)y.parts;
  p.fresh = params->first != 0;
  for (int m = 0; m < crn::MAX_LAGS; m++) p.lag[m] = m < p.n_lags ? params->lag[m] : 0;
  const int64_t mats = p.n_lags + 1;
  err = crn::in_grids(err, n_streams * y.parts * mats, [&](int64_t first, unsigned cnt) {
    p.first = first;
    hipLaunchKernelGGL(crn::hops_chunk_kernel, dim3(cnt), dim3(64), 0, st, p);
    return hipGetLastError();
  });
  err = crn::in_grids(err, n_streams * mats * crn::QUARTERS, [&](int64_t first, unsigned cnt) {
    p.first = first;
    hipLaunchKernelGGL(crn::hops_join_kernel, dim3(cnt), dim3(crn::JOIN_THREADS), 0, st, p);
    return hipGetLastError();
  });
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_hops_device: ") + hipGetErrorString(err));
  return CRN_OK;
}

int crn_hop_forecast(const void *record, int32_t m, uint64_t word, double prior, double p[64]) {
  if (!record || !p) return crn::fail(CRN_ERR_ARG, "crn_hop_forecast: null record or p");
  if (!(prior >= 0.0) || !std::isfinite(prior)) return crn::fail(CRN_ERR_ARG, "crn_hop_forecast: prior must be finite and >= 0");
  const char *rec = static_cast<const char *>(record);
  int32_t head[16];
  std::memcpy(head, rec, sizeof head);
  const int nch = head[2], n_lags = head[3];
  if (nch < 1 || nch > 63 || n_lags < 1 || n_lags > crn::MAX_LAGS) return crn::fail(CRN_ERR_ARG, "crn_hop_forecast: the record's n_channels or n_lags is out of range");
  if (m < 0 || m >= n_lags) return crn::fail(CRN_ERR_ARG, "crn_hop_forecast: m must be in 0 .. n_lags - 1");
  const char *block = rec + crn::HEAD_BYTES + crn::HIST_BYTES + crn::MAT_BYTES + int64_t(m) * crn::LAG_BYTES;
  uint64_t a = word & ((uint64_t(1) << nch) - 1);
  if (a == 0) a = uint64_t(1) << crn::IDLE;
  for (int j = 0; j < 64; j++) p[j] = 0.0;
  for (int i = 0; i < 64; i++) {
    if (!((a >> i) & 1)) continue;
    int32_t from, pair[64];
    std::memcpy(&from, block + 4 * i, 4);
    std::memcpy(pair, block + 512 + 256 * i, sizeof pair);
    const double den = (double)(from > 0 ? from : 0) + 2.0 * prior;
    for (int j = 0; j < 64; j++) {
      if (j >= nch && j != crn::IDLE) continue;
      const double q = den > 0.0 ? ((double)(pair[j] > 0 ? pair[j] : 0) + prior) / den : 0.5;
      p[j] = q > p[j] ? q : p[j];
    }
  }
  return CRN_OK;
}
