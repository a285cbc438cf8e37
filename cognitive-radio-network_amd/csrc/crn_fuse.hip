// crn_fuse.hip — cooperative sensing (crn_fuse_device, crn_fuse_member_pfa, include/crn_sense.h): the bit masks and `spectrum` rows of a
// group of M sensors become one fused mask, one fused row and a 16-byte header.  One launch, one workgroup per fused row, one
// instantiation per fft_len (fuse_kernel<N, TPB>: 128 threads at 512 points, 256 above), three steps:
//
//   1. row    every thread owns N / 4 / TPB float4 pieces of the row (coalesced: piece i * TPB + tid).  The active members' rows go by
//             once, in ascending order, straight from the loads into fp64 accumulators (4, 4, 8 and 16 per thread): F = fl32(acc) is
//             stored to the fused row from those registers and, under SOFT, left in LDS as fp64 (8 N bytes: the detector adds in fp64,
//             so the conversion is paid once per bin, not once per training cell).
//   2. votes  thread w < N / 32 owns mask word w: the active members' words are carry-saved into 6 bit planes (a bit-sliced counter,
//             32 bins side by side), "count >= votes" is a bitwise compare from the top plane down, n_any and n_all are the OR and the
//             AND of the same words.  Nothing is unpacked per bin.
//   3. SOFT   thread tid owns bins i * TPB + tid: consecutive lanes read consecutive fp64 cells of LDS (conflict-free ds_read_b64), each
//             bin adds its own 2 W training cells in the defined order, and a wave's ballot is 64 bits of the fused mask, stored by lane 0
//             as one 8-byte word.  Direct sums only: no sliding window, no prefix sums.  A wave whose 64 windows all lie inside the row
//             walks them without the wrap's index arithmetic (training_sum<false>); the others take the masked walk.
// The inactive members (weight 0) are left out on the host: the kernel gets the list of active ones and never forms an address inside
// the others' rows.  Counts meet in LDS (integer adds: the order does not matter).  No scratch memory, no global atomics, plain vector stores.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_segments.h"

namespace crn {
namespace {

struct FuseParams {
  const uint32_t *mask;     // [n_epochs][N / 32] or null
  const float *spectrum;    // [n_epochs][N] or null: the fused row is neither needed nor wanted
  uint32_t *fused_mask;     // [n_rows][N / 32] or null
  float *fused_spectrum;    // [n_rows][N] or null
  crn_fuse_row *rows;       // [n_rows] or null
  long long first;          // fused row of workgroup 0
  int eps, group, n_active;
  int soft, votes, guard, train;
  float alpha;
  float w[CRN_MAX_FUSE_MEMBERS];             // the active members' weights, in ascending order of the member ...
  int member[CRN_MAX_FUSE_MEMBERS];          // ... and which members they are
};

// T of the definition for bin k: the W cells on the left, then the W on the right, each side added in ascending distance.  WRAP = false
// where no index leaves the row: the two walks are then plain pointers, and the index arithmetic of the wrap (three instructions per
// cell next to the one fp64 add) is gone.
template <bool WRAP, int N>
__device__ __forceinline__ double training_sum(const double *frow, int k, int guard, int train) {
  double lsum = 0.0, rsum = 0.0;
#pragma unroll 4
  for (int i = guard + 1; i <= guard + train; i++) {
    lsum += frow[WRAP ? (k - i) & (N - 1) : k - i];
    rsum += frow[WRAP ? (k + i) & (N - 1) : k + i];
  }
  return lsum + rsum;
}

template <int N, int TPB>
__global__ __launch_bounds__(TPB) void fuse_kernel(const FuseParams p) {
  constexpr int V = N / 4 / TPB;      // float4 pieces of the row per thread
  constexpr int WORDS = N / 32;
  static_assert(V >= 1 && WORDS <= TPB && TPB % 64 == 0, "one thread per mask word, whole waves");
  __shared__ double frow[N];          // the fused row (SOFT)
  __shared__ int cnt[4];              // n_detected, n_any, n_all
  const int tid = threadIdx.x;
  const long long r = p.first + blockIdx.x;
  const long long j = r / p.eps;
  const long long e0 = j * p.group * p.eps + (r - j * p.eps);   // member 0's epoch; member m's is e0 + m * eps
  if (tid < 4) cnt[tid] = 0;

  // 1. the fused row
  if (p.spectrum != nullptr) {
    double acc[V][4];
#pragma unroll
    for (int i = 0; i < V; i++) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.0;
#pragma unroll 2
    for (int a = 0; a < p.n_active; a++) {
      const float4 *src = reinterpret_cast<const float4 *>(p.spectrum + (e0 + (long long)p.member[a] * p.eps) * N);
      const double w = (double)p.w[a];
      float4 q[V];
#pragma unroll
      for (int i = 0; i < V; i++) q[i] = src[i * TPB + tid];
#pragma unroll
      for (int i = 0; i < V; i++) {
        acc[i][0] += w * (double)q[i].x;
        acc[i][1] += w * (double)q[i].y;
        acc[i][2] += w * (double)q[i].z;
        acc[i][3] += w * (double)q[i].w;
      }
    }
    float4 *dst = p.fused_spectrum != nullptr ? reinterpret_cast<float4 *>(p.fused_spectrum + r * N) : nullptr;
#pragma unroll
    for (int i = 0; i < V; i++) {
      const float4 f = make_float4((float)acc[i][0], (float)acc[i][1], (float)acc[i][2], (float)acc[i][3]);
      if (dst != nullptr) dst[i * TPB + tid] = f;
      if (p.soft) {
        double *at = frow + 4 * (i * TPB + tid);
        at[0] = (double)f.x;
        at[1] = (double)f.y;
        at[2] = (double)f.z;
        at[3] = (double)f.w;
      }
    }
  }
  __syncthreads();

  // 2. the members' mask words: votes, any, all
  if (p.mask != nullptr && tid < WORDS) {
    uint32_t c[6] = {0, 0, 0, 0, 0, 0}, any = 0, all = ~0u;
    for (int a = 0; a < p.n_active; a++) {
      const uint32_t x = p.mask[(e0 + (long long)p.member[a] * p.eps) * WORDS + tid];
      any |= x;
      all &= x;
      uint32_t carry = x;
#pragma unroll
      for (int b = 0; b < 6; b++) {
        const uint32_t t = c[b] & carry;
        c[b] ^= carry;
        carry = t;
      }
    }
    atomicAdd(&cnt[1], __popc(any));
    atomicAdd(&cnt[2], __popc(all));
    if (!p.soft) {
      uint32_t gt = 0, eq = ~0u;      // count > votes, count == votes on the planes seen so far
#pragma unroll
      for (int b = 5; b >= 0; b--) {
        const uint32_t kb = (p.votes >> b) & 1 ? ~0u : 0u;
        gt |= eq & c[b] & ~kb;
        eq &= ~(c[b] ^ kb);
      }
      const uint32_t word = gt | eq;
      if (p.fused_mask != nullptr) p.fused_mask[r * WORDS + tid] = word;
      atomicAdd(&cnt[0], __popc(word));
    }
  }

  // 3. CA-CFAR on the fused row
  if (p.soft) {
    const double two_w = (double)(2 * p.train), alpha = (double)p.alpha;
    const int reach = p.guard + p.train;
    int nd = 0;
#pragma unroll 1
    for (int k = tid; k < N; k += TPB) {
      // the wave's 64 bins and their windows lie inside the row, or some window crosses the wrap: the same sums either way
      const int k0 = __builtin_amdgcn_readfirstlane(k);
      const double t = k0 - reach >= 0 && k0 + 63 + reach < N ? training_sum<false, N>(frow, k, p.guard, p.train)
                                                               : training_sum<true, N>(frow, k, p.guard, p.train);
      const bool det = frow[k] * two_w > alpha * t;
      const uint64_t bits = __ballot(det);
      if ((tid & 63) == 0) {
        if (p.fused_mask != nullptr) *reinterpret_cast<uint2 *>(p.fused_mask + r * WORDS + k / 32) = make_uint2((uint32_t)bits, (uint32_t)(bits >> 32));
        nd += __popcll(bits);
      }
    }
    if ((tid & 63) == 0) atomicAdd(&cnt[0], nd);
  }
  __syncthreads();
  if (tid == 0 && p.rows != nullptr) *reinterpret_cast<int4 *>(p.rows + r) = make_int4(cnt[0], cnt[1], cnt[2], p.n_active);
}

inline int refuse(const char *why) { return fail(CRN_ERR_ARG, std::string("crn_fuse_device: ") + why); }

template <int N, int TPB>
hipError_t launch(const FuseParams &p, unsigned n, hipStream_t stream) {
  hipLaunchKernelGGL((fuse_kernel<N, TPB>), dim3(n), dim3(TPB), 0, stream, p);
  return hipGetLastError();
}

// P(at least k of n independent sensors fire) when each fires with probability p: every term is positive, nothing cancels
double vote_tail(double p, int n, int k) {
  double s = 0.0;
  for (int j = k; j <= n; j++) {
    double c = 1.0;                                 // C(n, j): exact in double for n <= 32
    for (int i = 1; i <= j; i++) c = c * (n - j + i) / i;
    s += c * std::pow(p, j) * std::pow(1.0 - p, n - j);
  }
  return s;
}

}  // namespace
}  // namespace crn

int crn_fuse_device(crn_handle *h, const uint32_t *d_bin_mask, const float *d_spectrum, int64_t n_epochs, const crn_fuse_params *params,
                    uint32_t *d_fused_mask, float *d_fused_spectrum, crn_fuse_row *d_rows, void *stream) {
  static_assert(sizeof(crn_fuse_params) == 168 && sizeof(crn_fuse_row) == 16, "include/crn_sense.h");
  if (!h || !params) return crn::refuse("null handle / params");
  const crn_fuse_params &q = *params;
  if (!d_fused_mask && !d_fused_spectrum && !d_rows) return crn::refuse("no output: d_fused_mask, d_fused_spectrum and d_rows are all null");
  if (q.rule != CRN_FUSE_VOTE && q.rule != CRN_FUSE_SOFT) return crn::refuse("rule must be CRN_FUSE_VOTE or CRN_FUSE_SOFT");
  if (q.group_size < 1 || q.group_size > CRN_MAX_FUSE_MEMBERS) return crn::refuse("group_size must be in 1..32");
  if (n_epochs < 0) return crn::refuse("n_epochs < 0");
  if (q.epochs_per_stream < 1 || n_epochs % (int64_t(q.group_size) * q.epochs_per_stream) != 0)
    return crn::refuse("epochs_per_stream must be >= 1 and group_size * epochs_per_stream must divide n_epochs");
  for (int r : q.reserved)
    if (r != 0) return crn::refuse("reserved must be 0");
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  crn::FuseParams p{};
  for (int m = 0; m < CRN_MAX_FUSE_MEMBERS; m++) {
    const float w = q.weight[m];
    if (!std::isfinite(w) || w < 0.0f) return crn::refuse("a weight must be finite and >= 0");
    if (m >= q.group_size && w != 0.0f) return crn::refuse("weights at m >= group_size must be 0");
    if (w > 0.0f) {
      p.w[p.n_active] = w;
      p.member[p.n_active++] = m;
    }
  }
  if (p.n_active < 1) return crn::refuse("no active member: every weight is 0");
  if (q.rule == CRN_FUSE_VOTE) {
    if (!d_bin_mask) return crn::refuse("CRN_FUSE_VOTE needs d_bin_mask");
    if (q.votes < 1 || q.votes > p.n_active) return crn::refuse("votes must be in 1..n_active");
    if (q.guard != 0 || q.train != 0 || q.alpha != 0.0f) return crn::refuse("guard, train and alpha must be 0 under CRN_FUSE_VOTE");
  } else {
    if (!d_spectrum) return crn::refuse("CRN_FUSE_SOFT needs d_spectrum");
    if (q.votes != 0) return crn::refuse("votes must be 0 under CRN_FUSE_SOFT");
    if (q.train < 1 || q.train > 64 || q.guard < 0 || q.guard > n || 2 * (q.guard + q.train) + 1 > n)
      return crn::refuse("needs 1 <= train <= 64, guard >= 0 and 2 (guard + train) + 1 <= fft_len");
    if (!(q.alpha > 0.0f) || !std::isfinite(q.alpha)) return crn::refuse("alpha must be finite and > 0");
  }
  if (d_fused_spectrum && !d_spectrum) return crn::refuse("d_fused_spectrum needs d_spectrum");
  if (crn::misaligned(d_bin_mask, 8) || crn::misaligned(d_fused_mask, 8)) return crn::refuse("d_bin_mask and d_fused_mask must be 8-byte aligned");
  if (crn::misaligned(d_spectrum, 16) || crn::misaligned(d_fused_spectrum, 16) || crn::misaligned(d_rows, 16))
    return crn::refuse("d_spectrum, d_fused_spectrum and d_rows must be 16-byte aligned");
  if (n_epochs == 0) return CRN_OK;

  p.mask = d_bin_mask;
  p.soft = q.rule == CRN_FUSE_SOFT;
  // the members' rows are read only where something is made of them: the detector's input, or the fused row the caller asked for
  p.spectrum = p.soft || d_fused_spectrum ? d_spectrum : nullptr;
  p.fused_mask = d_fused_mask;
  p.fused_spectrum = d_fused_spectrum;
  p.rows = d_rows;
  p.eps = q.epochs_per_stream;
  p.group = q.group_size;
  p.votes = q.votes;
  p.guard = q.guard;
  p.train = q.train;
  p.alpha = q.alpha;
  hipError_t err = hipSetDevice(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n_rows = n_epochs / q.group_size;
  err = crn::in_grids(err, n_rows, [&](int64_t first, unsigned cnt) {
    p.first = first;
    return n == 512 ? crn::launch<512, 128>(p, cnt, st) : n == 1024 ? crn::launch<1024, 256>(p, cnt, st)
           : n == 2048 ? crn::launch<2048, 256>(p, cnt, st) : crn::launch<4096, 256>(p, cnt, st);
  });
  if (err != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("crn_fuse_device: ") + hipGetErrorString(err));
  return CRN_OK;
}

int crn_fuse_member_pfa(double pfa_fused, int32_t n, int32_t k, double *pfa_member) {
  if (!pfa_member) return crn::fail(CRN_ERR_ARG, "crn_fuse_member_pfa: null output");
  if (n < 1 || n > CRN_MAX_FUSE_MEMBERS || k < 1 || k > n) return crn::fail(CRN_ERR_ARG, "crn_fuse_member_pfa: needs n in 1..32 and k in 1..n");
  if (!(pfa_fused > 0.0) || !(pfa_fused < 1.0)) return crn::fail(CRN_ERR_ARG, "crn_fuse_member_pfa: pfa_fused must lie in (0, 1)");
  double lo = 0.0, hi = 1.0;               // the tail rises with p: from 0 at p = 0 to 1 at p = 1
  for (int it = 0; it < 2000; it++) {
    const double mid = 0.5 * (lo + hi);
    if (mid <= lo || mid >= hi) break;     // the interval is two neighbouring doubles
    if (crn::vote_tail(mid, n, k) < pfa_fused) lo = mid; else hi = mid;
  }
  *pfa_member = hi;                        // the smallest p whose tail reaches pfa_fused (n = k = 1: pfa_fused itself)
  return CRN_OK;
}
