// crn_mask_runs.h — what the units that read a bit mask lane by lane share (crn_segments.hip, crn_holes.hip, crn_channels.hip; never a
// sensing kernel): the mapping, the small bit helpers, and the extraction of the mask's runs.
// The mapping.  One wave per row of N = 64 B bins; lane l owns the B contiguous bins [l B, (l + 1) B) and its piece of the mask in one
// 64-bit register.  The row's values sit in LDS with PAD words between lane pieces, so that the lanes' 16-byte reads spread over the banks.
// The runs.  run_plan<B> decides from the bits alone, before any value is summed, how many runs of at least min_width bins END in each
// lane (an erosion by min_width - 1 and a popcount of run starts) and, with an inclusive add scan over the wave, which slot each gets.
// Runs are disjoint, so ascending end equals ascending lo except for the one run that crosses the wrap: it ends first and is stored last.
// An all-ones circle is cut between lane 63 and lane 0: one run, lo = 0, width = N.  The unit then walks its lane's bins once with an
// accumulator of its own (Acc, with acc_zero, acc_join(a, b): a, then b right behind it, and acc_from(a, lane)), keeps the run that
// touches the lane's low edge (head) and the one that leaves through its high edge (tail), and join_spanning carries tail + whole lanes
// to the lane where a spanning run ends, which adds its head and emits it.
#ifndef CRN_MASK_RUNS_H
#define CRN_MASK_RUNS_H
#include <hip/hip_runtime.h>

#include <cstdint>

namespace crn {

__device__ __forceinline__ int ctz64(uint64_t x) { return x ? __builtin_ctzll(x) : 64; }
__device__ __forceinline__ int clz64(uint64_t x) { return x ? __builtin_clzll(x) : 64; }
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return r ? (x << r) | (x >> (64 - r)) : x; }
__device__ __forceinline__ uint64_t rotr64(uint64_t x, int r) { return r ? (x >> r) | (x << (64 - r)) : x; }
__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// bit x of the result = OR (AND) of bits x - i (x + i) of the argument, 0 <= i <= g <= 63; zeros come in at the ends
__device__ __forceinline__ uint64_t or_up(uint64_t x, int g) {
  int c = 1;
  for (; 2 * c <= g + 1; c *= 2) x |= x << c;
  return x | (x << (g + 1 - c));
}
__device__ __forceinline__ uint64_t or_down(uint64_t x, int g) {
  int c = 1;
  for (; 2 * c <= g + 1; c *= 2) x |= x >> c;
  return x | (x >> (g + 1 - c));
}
__device__ __forceinline__ uint64_t and_down(uint64_t x, int g) {
  int c = 1;
  for (; 2 * c <= g + 1; c *= 2) x &= x >> c;
  return x & (x >> (g + 1 - c));
}

// the word `cur` dilated by g <= 32 bins, `prev` and `next` its neighbours in the circular row
__device__ __forceinline__ uint32_t dilate(uint32_t prev, uint32_t cur, uint32_t next, int g) {
  const uint64_t below = (uint64_t)prev | ((uint64_t)cur << 32), above = (uint64_t)cur | ((uint64_t)next << 32);
  return (uint32_t)(or_up(below, g) >> 32) | (uint32_t)or_down(above, g);
}

// the B bits of a lane's piece
constexpr uint64_t piece_bits(int B) { return B == 64 ? ~0ull : (1ull << (B % 64)) - 1; }

// lane l's piece of the row whose mask words are mw[0 .. 2 B): global memory or LDS
template <int B>
__device__ __forceinline__ uint64_t mask_piece(const uint32_t *mw, int l) {
  if constexpr (B == 64) {
    return (uint64_t)mw[2 * l] | ((uint64_t)mw[2 * l + 1] << 32);
  } else if constexpr (B == 32) {
    return mw[l];
  } else {
    return (mw[l / (32 / B)] >> ((l % (32 / B)) * B)) & piece_bits(B);
  }
}

// the row in LDS: 64 (B + PAD) words, word k of the row at padded<B>(row, k), lane l's own bins from own_piece<B>(row, l) on
constexpr int PAD = 4;
constexpr int padded_words(int B) { return 64 * (B + PAD); }
template <int B, class T>
__device__ __forceinline__ T *padded(T *row, int k) { return row + k + (k / B) * PAD; }
template <int B, class T>
__device__ __forceinline__ T *own_piece(T *row, int l) { return row + l * (B + PAD); }

// the 64 B floats at src: coalesced float4 loads by the wave, to the lanes that own the bins through LDS
template <int B>
__device__ __forceinline__ void load_row(float *row, const float *src, int l) {
  const float4 *src4 = reinterpret_cast<const float4 *>(src);
#pragma unroll
  for (int j = 0; j < B / 4; j++) {
    const int k = 4 * (j * 64 + l);
    *reinterpret_cast<float4 *>(padded<B>(row, k)) = src4[j * 64 + l];
  }
}

// The run structure of the wave's mask, lane l holding the piece c: which runs of at least min_width bins there are and where each is
// stored when at most max_out are.  run_plan keeps its results as const locals in this order and join_spanning takes its tail by
// reference: with a constructor that assigned the members and a tail by value segments_kernel<64> measured 4 % slower on real traffic
// (profiles/r15_mask_runs.txt).
struct RunPlan {
  bool cont_in, cont_out;   // the run at the lane's low (high) edge goes on in the lane before (after)
  bool pass;                // a lane in the middle of a run
  int head_lo;              // the first bin of the run that enters through the low edge; < 0: it crosses the wrap
  bool head_kept;           // that run ends in this lane and is wide enough
  int cnt, incl;            // kept runs that end in this lane, and in lanes 0 .. l: this lane's ranks are incl - cnt .. incl - 1, the head first
  int n_found, n_stored;
  bool wrap_kept;           // a kept run crosses the wrap: it ends first (rank 0) and is stored last

  __device__ __forceinline__ int slot(int rank) const { return wrap_kept ? (rank == 0 ? n_found - 1 : rank - 1) : rank; }
};

template <int B>
__device__ __forceinline__ RunPlan run_plan(uint64_t c, int l, int min_width, int max_out) {
  constexpr uint64_t PM = piece_bits(B);
  const bool all_ones = __ballot(c == PM) == ~0ull;
  const uint64_t tops = __ballot((c >> (B - 1)) & 1), lows = __ballot(c & 1);
  const bool cont_in = (c & 1) && ((tops >> ((l - 1) & 63)) & 1) && !(all_ones && l == 0);
  const bool cont_out = ((c >> (B - 1)) & 1) && ((lows >> ((l + 1) & 63)) & 1) && !(all_ones && l == 63);
  const bool pass = c == PM && cont_in && cont_out;
  const int headlen = cont_in ? ctz64(~c & PM) < B ? ctz64(~c & PM) : B : 0;
  const int taillen = cont_out ? (clz64(~(c << (64 - B))) < B ? clz64(~(c << (64 - B))) : B) : 0;
  // the bins a run has gathered before it enters this lane: whole lanes back to the nearest lane that is not `pass`, and its tail
  const uint64_t pt = __ballot(pass);
  const int dist_s = clz64(rotl64(~pt, (64 - l) & 63));
  const int carry_w = dist_s * B + __shfl(taillen, (l - 1 - dist_s) & 63, 64);
  const bool head_final = cont_in && !pass;                  // a run from an earlier lane ends here
  const int head_w = carry_w + headlen;
  const int head_lo = l * B + headlen - head_w;
  const bool head_kept = head_final && head_w >= min_width;
  const uint64_t own = c & ~low_bits(headlen) & low_bits(B - taillen);   // runs that start and end in this lane
  const uint64_t er = min_width - 1 >= B ? 0 : and_down(own, min_width - 1);
  const int cnt = __popcll(er & ~(er << 1)) + (head_kept ? 1 : 0);
  int incl = cnt;
#pragma unroll
  for (int s = 1; s < 64; s *= 2) {
    const int y = __shfl_up(incl, s, 64);
    if (l >= s) incl += y;
  }
  const int n_found = __shfl(incl, 63, 64);
  const int n_stored = n_found < max_out ? n_found : max_out;
  const bool wrap_kept = __ballot(head_kept && head_lo < 0) != 0;
  return RunPlan{cont_in, cont_out, pass, head_lo, head_kept, cnt, incl, n_found, n_stored, wrap_kept};
}

// Spanning runs.  tail: what leaves this lane through its high edge (acc_zero() where nothing does).  A segmented scan over lanes (6 steps,
// circular) joins it back to the lane where the run started; returned is what enters this lane through its low edge.
template <class Acc>
__device__ __forceinline__ Acc join_spanning(const Acc &tail, bool pass, int l) {
  Acc v = tail;
  bool done = !pass;
#pragma unroll
  for (int s = 1; s < 64; s *= 2) {
    const Acc o = acc_from(v, (l - s) & 63);
    const bool o_done = __shfl((int)done, (l - s) & 63, 64) != 0;
    if (!done) {
      v = acc_join(o, v);
      done = o_done;
    }
  }
  return acc_from(v, (l - 1) & 63);
}

}  // namespace crn
#endif
