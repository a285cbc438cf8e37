// crn_holes.hip — spectrum holes with idle age (crn_holes_device, include/crn_sense.h): the CFAR bit mask and, optionally, the `spectrum`
// rows of a batch become, per stream, the age of every bin (the epochs it has been clear, carried from call to call in the caller's
// d_age), the free mask age >= min_age, and the ordered list of its maximal runs with width, age range, peak and power.  Two launches on
// the caller's stream, both parallel along time, all scratch in the caller's workspace:
//
//   1. last     holes_last_kernel<N>, one workgroup of N / 8 threads per (stream, chunk of 64 epochs), the chunking of
//               channels_time_kernel (crn_channels.hip).  A thread takes mask words (coalesced) with their two neighbours in the row (the
//               neighbours wrap at both ends), dilates by `guard` <= 32 with shifts on the packed words, and leaves the dilated word in
//               LDS.  Then a thread owns 8 bins: it walks the chunk's epochs in time order and keeps, one byte per bin in two registers,
//               the offset of the last epoch whose bit was set (0xFF: none).  One 8-byte store per thread: [chunk][N] bytes.
//   2. stream   holes_stream_kernel<B>, one workgroup per stream, B = N / 64.  A thread owns groups of 4 bins; it walks the chunk rows
//               from the latest backwards, 16 rows in flight, until its wave has every bin resolved or the chunks are exhausted: a
//               stream of T epochs is at most T / 1024 dependent steps and as a rule one or two.  The result is combined with d_age under
//               the saturating rule; d_age and the free mask are written; ages and Pbar (the fp64 mean of the last A rows, coalesced
//               float4 loads) go to LDS, each lane piece padded by 4 words.  Wave 0 then extracts the runs with what it shares with
//               segments_kernel<B> (crn_mask_runs.h): lane l owns the B bins [l B, (l + 1) B), slots come from the bits alone
//               (run_plan<B>), one walk over the lane's bins with this unit's own accumulator, and join_spanning joins the lanes.
// Every value read from d_age or from the workspace is used as a value, never as an index.  Sums are fp64 and direct (no bin outside a
// hole enters its sum), rounded to fp32 once.  No scratch memory, no global atomics, plain vector stores.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_mask_runs.h"
#include "crn_segments.h"

namespace crn {
namespace {

constexpr int IN_FLIGHT = 16;    // chunk rows (CHUNK epochs each) the stream kernel loads before it looks at any
constexpr int32_t AGE_MAX = 0x7fffffff;

struct LastParams {
  const uint32_t *mask;   // [n_epochs][N / 32]
  uint8_t *last;          // [n_streams * chunks][N]
  long long first;        // chunk of workgroup 0
  int eps, chunks, guard;
};

template <int N>
__global__ __launch_bounds__(N / 8) void holes_last_kernel(const LastParams p) {
  constexpr int W = N / 32, TH = N / 8;
  __shared__ uint32_t blocked[CHUNK * W];
  const int tid = threadIdx.x;
  const long long chunk = p.first + blockIdx.x;
  const ChunkSpan cs = chunk_span(chunk, p.chunks, p.eps);
  const uint32_t *rows = p.mask + (cs.stream * p.eps + cs.t0) * W;
  for (int i = tid; i < cs.n * W; i += TH) {
    const int w = i & (W - 1), r = i - w;
    const uint32_t cur = rows[i];
    blocked[i] = p.guard == 0 ? cur : dilate(rows[r + ((w - 1) & (W - 1))], cur, rows[r + ((w + 1) & (W - 1))], p.guard);
  }
  __syncthreads();
  // bins 8 tid .. 8 tid + 7: byte tid % 4 of word tid / 4; four lanes read one LDS word (a broadcast), a wave 16 consecutive ones
  const uint32_t *col = blocked + tid / 4;
  const int sh = 8 * (tid & 3);
  uint32_t lo = 0xffffffffu, hi = 0xffffffffu;                    // one byte per bin: the last blocked epoch of the chunk so far
#pragma unroll 4
  for (int t = 0; t < cs.n; t++) {
    const uint32_t x = col[t * W] >> sh;
    // bits 0..3 to the low bits of four bytes (the four shifted copies do not overlap), then to whole bytes (m * 0xFF as a shift and a subtraction)
    const uint32_t blo = ((x & 15) * 0x00204081u) & 0x01010101u, bhi = (((x >> 4) & 15) * 0x00204081u) & 0x01010101u;
    const uint32_t mlo = (blo << 8) - blo, mhi = (bhi << 8) - bhi;
    const uint32_t tt = (uint32_t)t * 0x01010101u;
    lo = (lo & ~mlo) | (tt & mlo);
    hi = (hi & ~mhi) | (tt & mhi);
  }
  reinterpret_cast<uint2 *>(p.last + chunk * N)[tid] = make_uint2(lo, hi);
}

struct StreamParams {
  const uint8_t *last;      // [n_streams * chunks][N]
  const float *spectrum;    // [n_epochs][N] or null
  int32_t *age;             // [n_streams][N]
  crn_hole_stream *streams; // [n_streams]
  crn_hole *holes;          // [n_streams][max_holes] or null
  uint32_t *free_mask;      // [n_streams][N / 32] or null
  long long first;          // stream of workgroup 0
  int eps, chunks, fresh, min_age, min_width, max_holes, avg;
};

// what a run of free bins has accumulated; arg counts from the run's own first bin
struct Acc {
  int w, arg, amin, amax;   // bins, offset of the largest Pbar, smallest and largest age
  float mx;                 // that Pbar (-inf: none yet)
  double s0;                // sum Pbar
};

__device__ __forceinline__ Acc acc_zero() { return Acc{0, 0, AGE_MAX, 0, -__builtin_inff(), 0.0}; }

// a, then b right behind it
__device__ __forceinline__ Acc acc_join(const Acc &a, const Acc &b) {
  Acc r;
  r.s0 = a.s0 + b.s0;
  const bool later = b.mx > a.mx;   // ties stay with the earlier bin
  r.mx = later ? b.mx : a.mx;
  r.arg = later ? a.w + b.arg : a.arg;
  r.amin = a.amin < b.amin ? a.amin : b.amin;
  r.amax = a.amax > b.amax ? a.amax : b.amax;
  r.w = a.w + b.w;
  return r;
}

__device__ __forceinline__ Acc acc_from(const Acc &a, int lane) {
  Acc r;
  r.w = __shfl(a.w, lane, 64);
  r.arg = __shfl(a.arg, lane, 64);
  r.amin = __shfl(a.amin, lane, 64);
  r.amax = __shfl(a.amax, lane, 64);
  r.mx = __shfl(a.mx, lane, 64);
  r.s0 = __shfl(a.s0, lane, 64);
  return r;
}

template <int B>
__global__ __launch_bounds__(B == 8 ? 128 : 256) void holes_stream_kernel(const StreamParams p) {
  constexpr int N = 64 * B;
  constexpr int TH = B == 8 ? 128 : 256;     // threads
  constexpr int G = N / 4 / TH;              // groups of 4 bins per thread: group q = j TH + tid is bins 4 q .. 4 q + 3
  __shared__ float4 row4[padded_words(B) / 4];  // Pbar
  __shared__ int4 age4[padded_words(B) / 4];
  __shared__ uint32_t fw[N / 32];               // the free mask
  float *row = reinterpret_cast<float *>(row4);
  int *ages = reinterpret_cast<int *>(age4);
  const int tid = threadIdx.x;
  const long long stream = p.first + blockIdx.x;

  // the last blocked epoch of every bin: the chunk rows from the latest backwards
  int a[G][4];
#pragma unroll
  for (int j = 0; j < G; j++)
#pragma unroll
    for (int i = 0; i < 4; i++) a[j][i] = -1;                     // -1: not blocked in any row seen so far
  uint32_t seen[G];                                               // 0xFF in the bytes of the bins that are resolved
#pragma unroll
  for (int j = 0; j < G; j++) seen[j] = 0;
  const uint32_t *rows = reinterpret_cast<const uint32_t *>(p.last + stream * p.chunks * N);
  for (int c = p.chunks - 1; c >= 0; c -= IN_FLIGHT) {
    uint32_t v[IN_FLIGHT][G];
#pragma unroll
    for (int u = 0; u < IN_FLIGHT; u++)
#pragma unroll
      for (int j = 0; j < G; j++) v[u][j] = c - u >= 0 ? rows[(long long)(c - u) * (N / 4) + j * TH + tid] : 0xffffffffu;
    // four bins at a time: a byte below 0x80 is an offset, and the first one met (the latest row) stays; `row` keeps which row it was
    uint32_t val[G], row[G], fresh[G];
#pragma unroll
    for (int j = 0; j < G; j++) val[j] = row[j] = fresh[j] = 0;
#pragma unroll
    for (int j = 0; j < G; j++) {
      // the AND of the rows has a byte below 0x80 where some row has one: a group in which no lane of the wave finds anything new for an
      // open bin is skipped (bins that are blocked seldom or never cost 16 operations a round here, not 16 x 9)
      uint32_t all = v[0][j];
#pragma unroll
      for (int u = 1; u < IN_FLIGHT; u++) all &= v[u][j];
      if (__ballot(((~all >> 7) & 0x01010101u & ~seen[j]) != 0) == 0) continue;
#pragma unroll
      for (int u = 0; u < IN_FLIGHT; u++) {
        const uint32_t hit = (~v[u][j] >> 7) & 0x01010101u;
        const uint32_t take = ((hit << 8) - hit) & ~seen[j];      // 0xFF in the bytes this row resolves
        val[j] = (val[j] & ~take) | (v[u][j] & take);
        row[j] = (row[j] & ~take) | (((uint32_t)u * 0x01010101u) & take);
        fresh[j] |= take;
        seen[j] |= take;
      }
    }
    bool open = false;
#pragma unroll
    for (int j = 0; j < G; j++) {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if ((fresh[j] >> (8 * i)) & 1) a[j][i] = p.eps - 1 - ((c - (int)((row[j] >> (8 * i)) & 255)) * CHUNK + (int)((val[j] >> (8 * i)) & 255));
      open |= seen[j] != 0xffffffffu;
    }
    if (__ballot(open) == 0) break;                               // this wave's bins are all resolved
  }

  // the carry, d_age, the free mask; ages to LDS
#pragma unroll
  for (int j = 0; j < G; j++) {
    const int q = j * TH + tid;
    int4 *at = reinterpret_cast<int4 *>(p.age + stream * N) + q;
    int4 start = make_int4(0, 0, 0, 0);
    if (!p.fresh) start = *at;
    const int s[4] = {start.x, start.y, start.z, start.w};
    uint32_t f = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (a[j][i] < 0) {
        const long long grown = (long long)(s[i] > 0 ? s[i] : 0) + p.eps;
        a[j][i] = grown < AGE_MAX ? (int)grown : AGE_MAX;
      }
      f |= (uint32_t)(a[j][i] >= p.min_age) << i;
    }
    const int4 now = make_int4(a[j][0], a[j][1], a[j][2], a[j][3]);
    *at = now;
    *reinterpret_cast<int4 *>(padded<B>(ages, 4 * q)) = now;
    // eight neighbouring lanes hold one word of the free mask
    f <<= 4 * (tid & 7);
    f |= __shfl_xor(f, 1, 64);
    f |= __shfl_xor(f, 2, 64);
    f |= __shfl_xor(f, 4, 64);
    if ((tid & 7) == 0) {
      fw[q / 8] = f;
      if (p.free_mask != nullptr) p.free_mask[stream * (N / 32) + q / 8] = f;
    }
  }

  // Pbar: the mean of the last A rows, summed in fp64 in time order
  const int A = p.avg < p.eps ? p.avg : p.eps;
#pragma unroll
  for (int j = 0; j < G; j++) {
    const int q = j * TH + tid;
    float4 mean = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p.spectrum != nullptr) {
      const float4 *src = reinterpret_cast<const float4 *>(p.spectrum + (stream * p.eps + (p.eps - A)) * N) + q;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 4
      for (int t = 0; t < A; t++) {
        const float4 x = src[(long long)t * (N / 4)];
        s0 += (double)x.x;
        s1 += (double)x.y;
        s2 += (double)x.z;
        s3 += (double)x.w;
      }
      const double d = (double)A;
      mean = make_float4((float)(s0 / d), (float)(s1 / d), (float)(s2 / d), (float)(s3 / d));
    }
    *reinterpret_cast<float4 *>(padded<B>(row, 4 * q)) = mean;
  }
  __syncthreads();
  if (tid >= 64) return;

  // wave 0: lane l owns the bins [l B, (l + 1) B) and its piece of the free mask
  const int l = tid;
  const uint64_t c = mask_piece<B>(fw, l);

  // run structure from the bits
  const RunPlan plan = run_plan<B>(c, l, p.min_width, p.max_holes);
  crn_hole *holes = p.holes ? p.holes + stream * p.max_holes : nullptr;
  int best_w = 0, best_lo = 0, best_age = 0;                 // the widest hole this lane has emitted, stored or not

  auto emit = [&](const Acc &s, int lo, int rank) {
    if (s.w > best_w || (s.w == best_w && lo < best_lo)) {
      best_w = s.w;
      best_lo = lo;
      best_age = s.amin;
    }
    const int slot = plan.slot(rank);
    if (holes == nullptr || slot >= p.max_holes) return;
    crn_hole o;
    o.lo = lo;
    o.width = s.w;
    o.age = s.amin;
    o.age_max = s.amax;
    o.peak_bin = (lo + s.arg) & (N - 1);
    o.reserved = 0;
    o.power = (float)s.s0;
    o.peak_power = s.mx;
    holes[slot] = o;
  };

  // one walk over the lane's bins
  Acc r = acc_zero(), head = acc_zero();
  double fsum = 0.0;
  int rank = plan.incl - plan.cnt + (plan.head_kept ? 1 : 0);
  bool in_head = plan.cont_in;
  auto close_run = [&](int end) {
    if (in_head) {
      head = r;
    } else if (r.w >= p.min_width) {
      emit(r, l * B + end - r.w, rank);
      rank++;
    }
    r = acc_zero();
    in_head = false;
  };
  const float *mine = own_piece<B>(row, l);
  const int *mine_age = own_piece<B>(ages, l);
#pragma unroll 1
  for (int i4 = 0; i4 < B; i4 += 4) {
    const float4 qp = *reinterpret_cast<const float4 *>(mine + i4);
    const int4 qa = *reinterpret_cast<const int4 *>(mine_age + i4);
    const float pv[4] = {qp.x, qp.y, qp.z, qp.w};
    const int av[4] = {qa.x, qa.y, qa.z, qa.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = i4 + j;
      if ((c >> i) & 1) {
        const float P = pv[j];
        if (P > r.mx) {
          r.mx = P;
          r.arg = r.w;
        }
        r.s0 += (double)P;
        r.amin = av[j] < r.amin ? av[j] : r.amin;
        r.amax = av[j] > r.amax ? av[j] : r.amax;
        r.w++;
        fsum += (double)P;
      } else if (r.w) {
        close_run(i);
      }
    }
  }
  if (r.w && !plan.cont_out) close_run(B);

  // spanning holes: what leaves this lane through its high edge is joined back to the lane where the hole started
  const Acc carry = join_spanning(plan.cont_out ? r : acc_zero(), plan.pass, l);
  if (plan.head_kept) emit(acc_join(carry, head), plan.head_lo < 0 ? plan.head_lo + N : plan.head_lo, plan.incl - plan.cnt);

  // the stream's header, and zeros in the slots nobody filled
  int nfree = __popcll(c);
#pragma unroll
  for (int s = 32; s > 0; s /= 2) {
    nfree += __shfl_xor(nfree, s, 64);
    fsum += __shfl_xor(fsum, s, 64);
    const int ow = __shfl_xor(best_w, s, 64), olo = __shfl_xor(best_lo, s, 64), oage = __shfl_xor(best_age, s, 64);
    if (ow > best_w || (ow == best_w && ow > 0 && olo < best_lo)) {
      best_w = ow;
      best_lo = olo;
      best_age = oage;
    }
  }
  if (l == 0) {
    crn_hole_stream h;
    h.n_found = plan.n_found;
    h.n_stored = plan.n_stored;
    h.free_bins = nfree;
    h.widest_lo = best_lo;
    h.widest_width = best_w;
    h.widest_age = best_age;
    h.floor_mean = nfree && p.spectrum != nullptr ? (float)(fsum / (double)nfree) : 0.0f;
    h.reserved = 0;
    p.streams[stream] = h;
  }
  if (holes != nullptr) {
    crn_hole z{};
    for (int s = plan.n_stored + l; s < p.max_holes; s += 64) holes[s] = z;
  }
}

// Why q cannot serve n_epochs epochs, as the text that follows the entry point's name, or null when it can.  fft_len 0: not known (the
// size function has no handle), and min_width is then held to the largest fft_len.
const char *hole_params_refusal(const crn_hole_params &q, int64_t n_epochs, int fft_len = 0) {
  const int n = fft_len > 0 ? fft_len : MAX_N;
  if (n_epochs < 0) return "n_epochs < 0";
  if (q.epochs_per_stream < 1 || n_epochs % q.epochs_per_stream != 0) return "epochs_per_stream must be >= 1 and divide n_epochs";
  if (q.guard < 0 || q.guard > 32) return "guard must be in 0..32";
  if (q.min_age < 1) return "min_age < 1";
  if (q.min_width < 1 || q.min_width > n) return "min_width must be in 1..fft_len";
  if (q.max_holes < 1 || q.max_holes > 256) return "max_holes must be in 1..256";
  if (q.avg_epochs < 1 || q.avg_epochs > 64) return "avg_epochs must be in 1..64";
  if (q.reserved != 0) return "reserved must be 0";
  return nullptr;
}

// the workspace: one byte per bin and (stream, chunk), rows of n bytes
int64_t workspace_of(int64_t n_epochs, const crn_hole_params &q, int n) {
  const int64_t bytes = n_epochs / q.epochs_per_stream * chunks_per_stream(q.epochs_per_stream) * n;
  return bytes < 64 ? 64 : bytes;
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_holes_device: ") + why); }

template <int N>
hipError_t launch_last(const LastParams &p, unsigned n, hipStream_t stream) {
  hipLaunchKernelGGL(holes_last_kernel<N>, dim3(n), dim3(N / 8), 0, stream, p);
  return hipGetLastError();
}

template <int B>
hipError_t launch_streams(const StreamParams &p, unsigned n, hipStream_t stream) {
  hipLaunchKernelGGL(holes_stream_kernel<B>, dim3(n), dim3(B == 8 ? 128 : 256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace
}  // namespace crn

int64_t crn_holes_workspace_bytes(int64_t n_epochs, const crn_hole_params *params) {
  if (!params || crn::hole_params_refusal(*params, n_epochs)) return -1;
  return crn::workspace_of(n_epochs, *params, crn::MAX_N);
}

int crn_holes_device(crn_handle *h, const uint32_t *d_bin_mask, const float *d_spectrum, int64_t n_epochs, const crn_hole_params *params,
                     int32_t *d_age, crn_hole_stream *d_streams, crn_hole *d_holes, uint32_t *d_free_mask, void *d_workspace,
                     int64_t workspace_bytes, void *stream) {
  static_assert(sizeof(crn_hole_params) == 32 && sizeof(crn_hole) == 32 && sizeof(crn_hole_stream) == 32, "include/crn_sense.h");
  if (!h || !params || !d_bin_mask || !d_age || !d_streams || !d_workspace) return crn::refuse("null handle / params / mask / age / streams / workspace");
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  if (const char *why = crn::hole_params_refusal(*params, n_epochs, n)) return crn::refuse(why);
  if (crn::misaligned(d_bin_mask, 8) || crn::misaligned(d_free_mask, 8) || crn::misaligned(d_workspace, 8))
    return crn::refuse("d_bin_mask, d_free_mask and d_workspace must be 8-byte aligned");
  if (crn::misaligned(d_spectrum, 16) || crn::misaligned(d_age, 16) || crn::misaligned(d_streams, 16) || crn::misaligned(d_holes, 16))
    return crn::refuse("d_spectrum, d_age, d_streams and d_holes must be 16-byte aligned");
  if (workspace_bytes < crn::workspace_of(n_epochs, *params, n)) return crn::refuse("workspace too small (crn_holes_workspace_bytes)");
  if (n_epochs == 0) return CRN_OK;

  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t chunks = crn::chunks_per_stream(params->epochs_per_stream), n_streams = n_epochs / params->epochs_per_stream;
  crn::LastParams lp{d_bin_mask, static_cast<uint8_t *>(d_workspace), 0, params->epochs_per_stream, (int)chunks, params->guard};
  err = crn::in_grids(err, n_streams * chunks, [&](int64_t first, unsigned cnt) {
    lp.first = first;
    return n == 512 ? crn::launch_last<512>(lp, cnt, st) : n == 1024 ? crn::launch_last<1024>(lp, cnt, st)
           : n == 2048 ? crn::launch_last<2048>(lp, cnt, st) : crn::launch_last<4096>(lp, cnt, st);
  });
  crn::StreamParams sp{lp.last, d_spectrum, d_age, d_streams, d_holes, d_free_mask, 0, params->epochs_per_stream, (int)chunks,
                       params->first != 0, params->min_age, params->min_width, params->max_holes, params->avg_epochs};
  err = crn::in_grids(err, n_streams, [&](int64_t first, unsigned cnt) {
    sp.first = first;
    return n == 512 ? crn::launch_streams<8>(sp, cnt, st) : n == 1024 ? crn::launch_streams<16>(sp, cnt, st)
           : n == 2048 ? crn::launch_streams<32>(sp, cnt, st) : crn::launch_streams<64>(sp, cnt, st);
  });
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_holes_device: ") + hipGetErrorString(err));
  return CRN_OK;
}
