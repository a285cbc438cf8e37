// crn_track_link.h — what crn_tracks.hip and crn_tracks_carry.hip share: the lock-free union-find over parent[], the link condition and
// the pair loop around it, what a member adds to its root, a record's centre, the zero fill of the unused track slots, the wave's add
// scan, and the one statement of which crn_track_params are usable (with the entry points' bookkeeping).
//
// The union.  parent[] starts with every node its own root.  find halves the path it walks; unite finds both roots and hooks the larger
// under the smaller with one atomicCAS, so a parent never exceeds its child, no cycle can form, and the root of a finished component is
// its smallest index.  A failed CAS returns the value that beat it and the loop goes on from there; a stale read of parent[] can only
// show a former ancestor, which is harmless for the same reason.
#ifndef CRN_TRACK_LINK_H
#define CRN_TRACK_LINK_H
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "crn_internal.h"
#include "crn_segments.h"

namespace crn {

constexpr int MAX_SLOTS = 256;   // max_segments at most

__device__ __forceinline__ int ld(const int *q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int *q, int v) { __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as far as this lane can see, halving the path on the way (every value written is an ancestor of the node it is written
// to).  LOWER: the halving writes are atomicMin, so a node that has been given its root keeps it whatever a slower lane writes later;
// that is what leaves parent[] flat after the gather pass.  The link pass, where roots still move, halves with plain stores.
template <bool LOWER>
__device__ __forceinline__ int find(int *parent, int x) {
  int px = ld(parent + x);
  while (px != x) {
    const int gp = ld(parent + px);
    if (gp != px) {
      if (LOWER) atomicMin(parent + x, gp);
      else st(parent + x, gp);
    }
    x = px;
    px = gp;
  }
  return x;
}

// unites the components of root-or-member rx and node y; returns the smaller root
__device__ __forceinline__ int unite(int *parent, int rx, int y) {
  rx = find<false>(parent, rx);
  int ry = find<false>(parent, y);
  while (rx != ry) {
    if (rx > ry) {
      const int t = rx;
      rx = ry;
      ry = t;
    }
    const int old = atomicCAS(parent + ry, ry, rx);
    if (old == ry) break;
    ry = find<false>(parent, old);   // somebody hooked ry first: go on from where it hangs now
    rx = find<false>(parent, rx);
  }
  return rx < ry ? rx : ry;
}

// one half of the link condition, on the circle of mask + 1 bins: a segment that begins at lo_b begins inside (lo, width) widened by
// slack.  Two segments are linked when either begins inside the other.  The halves stay two calls around the caller's ||, so that the
// partner's width is read only where the first half fails: as one function of two pairs the link kernels compiled differently and a
// one-stream list ran 4.9 % slower (profiles/r10_tracks_shared.txt).
__device__ __forceinline__ bool begins_in(int lo, int width, int lo_b, int mask, int slack) { return ((lo_b - lo) & mask) < width + slack; }

// the link pass's pair loop: lane l walks next[0 .. nb) (a broadcast read each) for each of its segments mine[l], mine[l + 64], ... below
// na and unites node a0 + a with node b0 + b on every hit.  The lane keeps the root it reached, so the second and later unions of one
// segment start at the root.
__device__ __forceinline__ void link_rows(int *parent, const int2 *mine, int na, int a0, const int2 *next, int nb, int b0, int l, int mask,
                                          int slack) {
  for (int a = l; a < na; a += 64) {
    const int2 sa = mine[a];
    int root = a0 + a;
    for (int b = 0; b < nb; b++) {
      const int2 sb = next[b];
      if (begins_in(sa.x, sa.y, sb.x, mask, slack) || begins_in(sb.x, sb.y, sa.x, mask, slack)) root = unite(parent, root, b0 + b);
    }
  }
}

// x - y on the circle of n bins (a power of two), in [-n / 2, n / 2)
__device__ __forceinline__ int wrapped(int x, int y, int half, int mask) { return ((x - y + half) & mask) - half; }

// segment g, `off` bins from its root's lo, adds itself to the root's accumulator (TrackAcc or CarryAcc): integer atomics, exact in any
// order, and the two fp64 sums with fp64 atomic adds.  first: no lower slot of g's epoch belongs to the same root; g is in slot s of S at
// time t, and last_key (as wide as Acc has it) orders the members by the latest epoch and there the lowest slot.
template <class Acc>
__device__ __forceinline__ void add_member(Acc *a, const crn_segment &g, int off, bool first, int t, int s, int S) {
  if (first) atomicAdd(&a->hits, 1);
  atomicAdd(&a->nseg, 1);
  atomicMax(&a->last_key, (decltype(a->last_key))((long long)t * S + (S - 1 - s)));
  atomicMin(&a->lo_off, off);
  atomicMax(&a->hi_off, off + g.width - 1);
  atomicMax(&a->peak, __float_as_uint(g.peak_power));
  atomicAdd(&a->width_sum, (unsigned long long)g.width);
  atomicAdd(&a->power, (double)g.power);
  atomicAdd(&a->moment, (double)g.power * ((double)off + (double)g.centroid));
}

// a record's centre: lo_root + moment / power, wrapped into [0, n) and rounded to float once
__device__ __forceinline__ float centre(int lo_root, double moment, double power, int n) {
  double c = (double)lo_root + (power > 0.0 ? moment / power : 0.0);
  c -= (double)n * floor(c / (double)n);
  const float cf = (float)c;
  return cf >= (float)n ? 0.0f : cf;
}

// zeros in a stream's slots [n_stored, max_tracks) by the 1024 threads of a workgroup: 64 bytes per slot as four 16-byte stores
__device__ __forceinline__ void zero_unused(crn_track *tracks, int n_stored, int max_tracks, int i) {
  uint4 *z = reinterpret_cast<uint4 *>(tracks);
  for (int k = 4 * n_stored + i; k < 4 * max_tracks; k += 1024) z[k] = make_uint4(0, 0, 0, 0);
}

// inclusive add scan over the 64 lanes of a wave; l: the lane
__device__ __forceinline__ int wave_scan(int v, int l) {
#pragma unroll
  for (int s = 1; s < 64; s *= 2) {
    const int y = __shfl_up(v, s, 64);
    if (l >= s) v += y;
  }
  return v;
}

// Why q cannot serve n_epochs epochs, as the text that follows the entry point's name, or null when it can.  fft_len 0: not known (the
// size functions have no handle), and slack_bins is then not bounded from above.
inline const char *track_params_refusal(const crn_track_params &q, int64_t n_epochs, int fft_len = 0) {
  if (n_epochs < 0) return "n_epochs < 0";
  if (q.max_segments < 1 || q.max_segments > MAX_SLOTS) return "max_segments must be in 1..256";
  if (q.epochs_per_stream < 1 || n_epochs % q.epochs_per_stream != 0) return "epochs_per_stream must be >= 1 and divide n_epochs";
  if (q.slack_bins < 0 || (fft_len > 0 && q.slack_bins >= fft_len)) return "slack_bins must be in 0..fft_len - 1";
  if (q.max_miss < 0 || q.max_miss > 15) return "max_miss must be in 0..15";
  if (q.min_epochs < 1) return "min_epochs < 1";
  if (q.max_tracks < 1 || q.max_tracks > 1024) return "max_tracks must be in 1..1024";
  if (q.reserved[0] != 0 || q.reserved[1] != 0) return "reserved must be 0";
  return nullptr;
}

// the entry points' bookkeeping: CRN_ERR_ARG / CRN_ERR_DEVICE as "<who>: <why>", the workspace from its first 64-byte boundary on (a
// pointer's alignment: misaligned, crn_segments.h)
inline int refuse(const char *who, const char *why) { return fail(CRN_ERR_ARG, std::string(who) + ": " + why); }
inline int fail_hip(const char *who, hipError_t err) { return fail(CRN_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(err)); }
inline char *align64(void *ptr) { return reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(ptr) + 63) & ~uintptr_t(63)); }

}  // namespace crn
#endif
