// crn_epoch_close.h — what runs once per K frames: band sums in their three forms, features, the 4-5-3 network and the cascade / the threshold
// decision (reference: CE_Predictive_Node.cpp:157-261, reset at :287-288).
#ifndef CRN_EPOCH_CLOSE_H
#define CRN_EPOCH_CLOSE_H
#include "crn_frame.h"

// In-kernel time stamps exist only in the measurement build (libcrnsense_ab.so, variant 17: crn_frame_ab.h).  The shipped library's
// hooks are empty: no stamp, no instruction.
#ifdef CRN_AB_VARIANTS
#include "crn_frame_ab.h"
#else
namespace crn {
template <class C>
struct CloseTrace {
  CRN_DEV void workgroup_start(const SenseParams &, int) {}
  CRN_DEV void enter(const SenseParams &, long long, bool, int, int) {}
  CRN_DEV void stamp1() {}
  CRN_DEV void stamp2() {}
  CRN_DEV void stamp3() {}
  CRN_DEV void leave(const SenseParams &, long long, bool, int) {}
};
}  // namespace crn
#endif

namespace crn {
// ---------------------------------------------------------------------------------------------
// Epoch close (reference .cpp:157-261 + the reset at :287-288): K-frame averages -> LDS in natural
// bin order -> band sums -> features -> decision.  Resets the accumulators for the next epoch.
// ---------------------------------------------------------------------------------------------
// (where the close's LDS lies — a lane group's exchange buffers, the band-table copy, the team partials: lds_layout, crn_forms.h)

// What the LDS form of the close keeps behind a lane group's image of the spectrum (N + N / 16 floats over the group's exchange
// buffers), in floats from the image's start
template <int R3>
struct CloseImage {
  static constexpr int kFeat = spec_phys(Geo<R3>::N);     // [CRN_MAX_BANDS = 80] features
  static constexpr int kBlk = kFeat + 80;                 // [T] totals of the 16-bin blocks
  static constexpr int kRows = kBlk + Geo<R3>::T;         // [R3] totals of the 256-bin rows
  static constexpr int kMask = kRows + R3;                // CFAR: [N / 16] half-words = [N / 32] words of detected bins
  static constexpr int kCnt = kMask + Geo<R3>::N / 32;    // CFAR: [n_bands] detected bins per band
};

// LDS address-space views for the epoch close (see epoch_close): ds_* instructions, lgkmcnt only.
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) int lds_i32;
typedef __attribute__((address_space(3))) double lds_f64;
typedef __attribute__((address_space(3))) unsigned short lds_u16;
typedef __attribute__((address_space(3))) unsigned int lds_u32;
CRN_DEV unsigned lds_offset(const void *p) {
  return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const void *)p;
}

// Sum over a team of TEAM consecutive lanes (32 or 64), every lane gets the total: butterflies on
// the DPP path (quad_perm xor 1, xor 2, row_half_mirror, row_mirror) up to 16-lane rows, then the
// four row sums come back through v_readlane.  No LDS-pipe shuffles.
template <int CTRL>
CRN_DEV float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int TEAM>
CRN_DEV float team_sum(float v, int tid) {
  static_assert(TEAM == 32 || TEAM == 64, "team is half a wave or a wave");
  v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  v = dpp_add<0x140>(v);  // row_mirror
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  if constexpr (TEAM == 64) return (r0 + r1) + (r2 + r3);
  else return (tid & 32) ? r2 + r3 : r0 + r1;
}

// W consecutive table words through the scalar cache into SGPRs (the epoch close must not touch
// vmcnt, and an LDS read queues behind the other waves' exchange traffic): issue with s_load_row,
// then s_wait_row before the first use.
template <int W> struct SWords;
template <> struct SWords<2> { typedef int T __attribute__((ext_vector_type(2))); };
template <> struct SWords<4> { typedef int T __attribute__((ext_vector_type(4))); };
template <> struct SWords<8> { typedef int T __attribute__((ext_vector_type(8))); };
template <> struct SWords<16> { typedef int T __attribute__((ext_vector_type(16))); };
template <int W, int BYTE_OFF>
CRN_DEV typename SWords<W>::T s_load_row(const int *base) {
  typename SWords<W>::T r;
  if constexpr (W == 2) asm volatile("s_load_dwordx2 %0, %1, %2" : "=s"(r) : "s"(base), "n"(BYTE_OFF));
  if constexpr (W == 4) asm volatile("s_load_dwordx4 %0, %1, %2" : "=s"(r) : "s"(base), "n"(BYTE_OFF));
  if constexpr (W == 8) asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(r) : "s"(base), "n"(BYTE_OFF));
  if constexpr (W == 16) asm volatile("s_load_dwordx16 %0, %1, %2" : "=s"(r) : "s"(base), "n"(BYTE_OFF));
  return r;
}
template <class V>
CRN_DEV void s_wait_row(V &r) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(r));
}

// The reference's 4-5-3 sigmoid network and cascade (CE_Predictive_Node.cpp:200-261), spread over the
// lanes of a team: hidden unit j on lane j, output k on lane k, values passed with v_readlane.  Each
// unit's sum is formed by one lane in the reference's order, so the results are those of the serial
// loop; what changes is the latency — two exp() in sequence instead of eight (one lane doing all of
// it cost the reference-mode kernel 3.8 %).  Weights come from the LDS copy of the table (a per-lane
// global load would wait on vmcnt behind the prefetch).  Every lane of the team must call this.
template <int TEAM>
CRN_DEV double lane_f64(double v, int src, int half) {
  const int lo = __builtin_amdgcn_readlane((int)(__double_as_longlong(v) & 0xffffffffll), src);
  const int hi = __builtin_amdgcn_readlane((int)(__double_as_longlong(v) >> 32), src);
  double r = __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
  if constexpr (TEAM == 32) {  // two groups share a wave: the upper one reads lanes 32 + src
    const int lo2 = __builtin_amdgcn_readlane((int)(__double_as_longlong(v) & 0xffffffffll), 32 + src);
    const int hi2 = __builtin_amdgcn_readlane((int)(__double_as_longlong(v) >> 32), 32 + src);
    const double r2 = __longlong_as_double(((long long)hi2 << 32) | (unsigned int)lo2);
    r = half ? r2 : r;
  }
  return r;
}

template <int TEAM>
CRN_DEV void ann_decide_team(const SenseParams &p, const lds_f64 *w_ih, const lds_f64 *w_ho, long long epoch,
                             bool store, int lane, int half, float nf, float ch1, float ch2, float ch3) {
  // .cpp:200: Features_Buffer = {0, NOISE_FLOOR, CH1, CH2, CH3} widened to double
  const double f1 = (double)nf, f2 = (double)ch1, f3 = (double)ch2, f4 = (double)ch3;
  const int j = (lane >= 1 && lane <= 5) ? lane : 1;  // .cpp:214-220, unit j
  double s = w_ih[0 * 6 + j];
  s += f1 * w_ih[1 * 6 + j];
  s += f2 * w_ih[2 * 6 + j];
  s += f3 * w_ih[3 * 6 + j];
  s += f4 * w_ih[4 * 6 + j];
  const double hj = 1.0 / (1.0 + exp(-s));
  double hid[6];
#pragma unroll
  for (int q = 1; q <= 5; q++) hid[q] = lane_f64<TEAM>(hj, q, half);
  const int k = (lane >= 1 && lane <= 3) ? lane : 1;  // .cpp:229-235, output k
  double so = w_ho[0 * 4 + k];
#pragma unroll
  for (int q = 1; q <= 5; q++) so += hid[q] * w_ho[q * 4 + k];
  const double ok = 1.0 / (1.0 + exp(-so));
  const double o1 = lane_f64<TEAM>(ok, 1, half), o2 = lane_f64<TEAM>(ok, 2, half), o3 = lane_f64<TEAM>(ok, 3, half);
  // .cpp:245-261 cascade
  int d = 0;
  if (o1 >= p.ann_threshold) d = 1;
  else if (o2 >= p.ann_threshold) d = 2;
  else if (o3 >= p.ann_threshold) d = 3;
  if (store) {
    if (lane >= 1 && lane <= 3 && p.ann_out != nullptr) p.ann_out[epoch * 3 + (lane - 1)] = ok;
    if (lane == 0 && p.decision != nullptr) p.decision[epoch] = d;
    if (lane < p.n_bands && p.occupancy != nullptr) p.occupancy[epoch * p.n_bands + lane] = (uint8_t)(lane >= 1 && lane == d);
  }
}

template <class C>
CRN_DEV void epoch_close(FrameCtx<C> &c, const SenseParams &p, long long epoch_base) {
  constexpr int R3 = C::R3;
  constexpr bool MAG = C::MAG;
  using G = Geo<R3>;
  constexpr int T = G::T, N = G::N, J = G::J;
  constexpr LdsLayout kLds = lds_layout(R3, C::NBUF, (C::OPT & kDeal) != 0);
  float (&acc)[16] = c.acc;
  const float Kf = c.Kf;
  // Everything this block needs is re-derived here from uniform values (SGPRs) and the hardware
  // lane id, so that nothing but the accumulators stays live in VGPRs across the frame loop for a
  // block that runs once per K frames: what the allocator kept for it, it spilled, and a scratch
  // reload waits on vmcnt behind the next frame's prefetch.
  // latency-bound stretch with nothing of this wave's in flight behind it, and the workgroup's other
  // waves waiting at its barriers: outrank the butterflies (+0.6 % at N = 4096, +1.3 % at 2048; the
  // barrier-free sizes lose 0.5 % with it)
  if constexpr ((C::OPT & kPrioValu) != 0 && G::XWAVE) __builtin_amdgcn_s_setprio(3);
  const int tid = c.wave * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int t = tid % T, grp = tid / T;
  const long long epoch = epoch_base + (long long)grp * c.grp_epoch_stride;
  const bool active = epoch < p.n_epochs;
  const int a = t / R3, m_lo = t % R3;
  CloseTrace<C> trace;
  trace.enter(p, epoch, active, t, T);
  // Energy mode: the division by K is applied to the band sums (and to the per-bin values only
  // when a spectrum is requested) — sixteen IEEE divides per thread per epoch were half a frame's
  // worth of VALU work.  Sum-then-divide differs from the reference order (divide-then-sum) by
  // rounding only.
  // The opaque values are 32-bit LDS offsets, not generic pointers: through a generic pointer every
  // access below became a FLAT instruction followed by s_waitcnt vmcnt(0), which also drained the
  // next frame's prefetch at every epoch close.
  const unsigned tab_off = c.lds_base + (unsigned)kLds.tab;
  const unsigned gb_off = c.lds_base + (unsigned)grp * (unsigned)kLds.group_bytes;
  const lds_i32 *tab = reinterpret_cast<const lds_i32 *>(tab_off);
  const lds_f32 *thr = reinterpret_cast<const lds_f32 *>(tab_off + kTabThresh * 4);
  const lds_f64 *w_ih = reinterpret_cast<const lds_f64 *>(tab_off + kTabWih * 4);  // [5][6]
  const lds_f64 *w_ho = reinterpret_cast<const lds_f64 *>(tab_off + kTabWho * 4);  // [6][4]
  lds_f32 *spec = reinterpret_cast<lds_f32 *>(gb_off);    // N + N/16 floats
  using Img = CloseImage<R3>;
  lds_f32 *featl = spec + Img::kFeat;
  constexpr int TEAM = G::TEAM;
  constexpr int TPG = T / TEAM;  // teams (waves) per group
  const int lane = t % TEAM;
  lds_f32 *part = reinterpret_cast<lds_f32 *>(tab_off + (unsigned)(kLds.part - kLds.tab));  // [256 / TEAM][16]
  [[maybe_unused]] const lds_f32 *feat = nullptr;
  // Three forms of the close, chosen per launch (one kernel holding several spilled in the frame loop):
  static_assert((C::OPT & kCfar) == 0 || (C::OPT & (kAlignedBands | kRegBands | kRows | kDeal)) == 0, "CFAR runs in the LDS form of the close");
  if constexpr ((C::OPT & kAlignedBands) != 0) {
    // Equal contiguous bands of W = 2^sh bins, sh = 6..8 (the Welch scan's 64 channels of 64 bins), N = 4096:
    // thread (a, m_lo) holds bins 256 d + 16 m_lo + a in acc[d], so band (256 d + 16 m_lo) >> sh is the sum over
    // all 16 a and over a group of G = W / 16 consecutive m_lo — lanes of one DPP row.  Group sums by DPP
    // (no LDS), the four rows of a wave through the wave's OWN exchange rows (only x1 writes of other waves
    // ever touch them, and those sit between the frame's two barriers), one barrier, then one lane per band adds
    // the 16 values of a: 2-4 DPP adds per register, <= 16 narrow LDS writes and one barrier instead of a
    // spectrum image, three barriers and a table walk (5 % of the Welch stream at K = 8).
    static_assert(R3 == 16 && !MAG, "aligned-band close: N = 4096, energy mode");
    const int sh = p.aligned_shift;   // uniform
    const int G = 1 << (sh - 4), nb = p.n_bands, al = (tid >> 4) & 3, r = m_lo & (G - 1), grp_b = m_lo >> (sh - 4);
    constexpr int kStride = 72;       // floats per a-row of partials: 72 mod 32 = 8 keeps a wave's rows on distinct banks
    lds_f32 *mine = reinterpret_cast<lds_f32 *>(c.lds_base + (unsigned)(4 * c.wave * Geo<R3>::ROW * sizeof(cx))) + al * kStride;
    const float thr_lane = thr[tid & 63];
#pragma unroll
    for (int d = 0; d < 16; d++) {
      float v = acc[d];
      acc[d] = 0.f;  // .cpp:287
      v = dpp_add<0xB1>(v);
      v = dpp_add<0x4E>(v);
      if (sh >= 7) v = dpp_add<0x141>(v);
      if (sh >= 8) v = dpp_add<0x140>(v);
      if ((d & (G - 1)) == r) mine[(d << (8 - sh)) + grp_b] = v;   // one lane of the group stores the group's sum
    }
    trace.stamp1();
    __syncthreads();
    trace.stamp2();
    if (c.wave == 0) {
      const int b = tid;  // one lane per band (n_bands <= 64)
      float sum = 0.f;
      if (b < nb) {
#pragma unroll
        for (int w4 = 0; w4 < 4; w4++) {
          const lds_f32 *src = reinterpret_cast<const lds_f32 *>(c.lds_base + (unsigned)(4 * w4 * Geo<R3>::ROW * sizeof(cx)));
          const float a0 = src[b], a1 = src[kStride + b], a2 = src[2 * kStride + b], a3 = src[3 * kStride + b];
          sum += a0;
          sum += a1;
          sum += a2;
          sum += a3;
        }
      }
      trace.stamp3();
      const float f = sc_unscale<C>(__fdiv_rn(sum, Kf), p);
      const bool in = b < nb;
      if (p.decide == CRN_DECIDE_THRESHOLD_K) {
        const float ref = p.ref_band >= 0 ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f), p.ref_band)) : 1.0f;
        const bool occ = active && in && f > thr_lane * ref;
        if (active && in && p.occupancy != nullptr) p.occupancy[epoch * nb + b] = (uint8_t)occ;
        const unsigned long long m = __ballot(occ);
        if (active && b == 0 && p.decision != nullptr) p.decision[epoch] = __popcll(m);
      } else if (active) {
        if (b == 0 && p.decision != nullptr) p.decision[epoch] = 0;
        if (in && p.occupancy != nullptr) p.occupancy[epoch * nb + b] = 0;
      }
      if (active && in && p.features != nullptr) p.features[epoch * nb + b] = f;
    }
  } else if constexpr ((C::OPT & kRegBands) != 0) {
    // Band sums straight from the accumulator registers: no LDS image of the spectrum, no barrier
    // before it (nothing aliases the exchange buffers) and none after the decision.  Thread bins are
    // row_start(d) + q_j (BinMap: row_start = 256 d, 256 d - 7 in the kTw1C kernels); the host cut the band
    // plan at those rows (crn_tables.cpp), so each entry is (row d, band, [lo, hi) in the row): masked add over j,
    // DPP team sum, lane `band` keeps it.
    // LDS round trips are what this block avoids (an LDS read here queues behind the exchange
    // traffic of the CU's other waves: measured ~500 ticks each): the entries come through the
    // scalar cache, the features stay in lanes, the thresholds are fetched first and used last.
    constexpr int CAP = kRowEntryWords / R3;  // entry slots per row
    constexpr unsigned AM = acc_mask<C>();   // registers j R3 + d the kernel keeps (all of them unless kRows)
    constexpr auto row_live = [](int d) {     // some register of row d is kept
      for (int j = 0; j < J; j++)
        if ((acc_mask<C>() >> (j * R3 + d)) & 1u) return true;
      return false;
    };
    float thr_lane = 0.f;
    if constexpr (TPG == 1) thr_lane = thr[lane & 15];  // fetched first, used last
    // one row's entries at a time, the next row's load in flight meanwhile: holding all of them
    // costs SGPRs the frame loop needs (the spill lanes' VGPR pushed a loop address to scratch)
    constexpr auto next_live = [](int d) {
      for (int x = d + 1; x < R3; x++)
        for (int j = 0; j < J; j++)
          if ((acc_mask<C>() >> (j * R3 + x)) & 1u) return x;
      return (int)R3;
    };
    constexpr int kFirst = next_live(-1);
    float fsum = 0.f;
    // (the kTw1C kernels read the entries cut at their own rows: same packing, a table of their own)
    constexpr bool SHIFTED = BinMap<C>::S != 0;
    constexpr int kEnt0 = SHIFTED ? 0 : kTabRowEntries;
    const int *ent_tab = SHIFTED ? p.row_entries_shift : p.band_tab;
    typename SWords<CAP>::T ent_next = s_load_row<CAP, (kEnt0 + kFirst * CAP) * 4>(ent_tab);
    static_for<R3>([&](auto dc) {
      constexpr int d = decltype(dc)::value;
      if constexpr (row_live(d)) {
        typename SWords<CAP>::T ent = ent_next;
        s_wait_row(ent);
        constexpr int dn = next_live(d);
        if constexpr (dn < R3) ent_next = s_load_row<CAP, (kEnt0 + dn * CAP) * 4>(ent_tab);
#pragma unroll
        for (int e = 0; e < CAP; e++) {
          const int w = ent[e];
          if (w != 0) {  // uniform; 0 = unused slot
            const int band = w >> 18, lo = (w >> 9) & 511, span = (w & 511) - lo;
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < J; j++) {
              if (((AM >> (j * R3 + d)) & 1u) == 0) continue;   // never accumulated: no band of the plan reaches it
              const int base = BinMap<C>::q(a, m_lo, j);
              v += (unsigned)(base - lo) < (unsigned)span ? acc[j * R3 + d] : 0.f;
            }
            v = team_sum<TEAM>(v, tid);
            fsum += lane == band ? v : 0.f;
          }
        }
      }
    });
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;  // .cpp:287
    trace.stamp1();
    if constexpr (TPG > 1) {
      if (lane < 16) part[(tid / TEAM) * 16 + lane] = fsum;
      __syncthreads();
      trace.stamp2();
      if (t < TEAM && lane < 16) {
        thr_lane = thr[lane];  // same LDS round trip as the partials
        fsum = 0.f;
#pragma unroll
        for (int w = 0; w < TPG; w++) fsum += part[(grp * TPG + w) * 16 + lane];
      }
    }
    trace.stamp3();
    // the first team of the group stores and decides; lane b holds band b (n_bands <= 16)
    if (t < TEAM) {
      const float fs1 = MAG ? sc_unscale<C>(fsum, p) : fsum;
      const float f = MAG ? fs1 * fs1 : sc_unscale<C>(__fdiv_rn(fsum, Kf), p);  // .cpp:194-197
      const int half = TEAM == 32 ? (tid & 32) : 0;             // two groups share a wave at T = 32
      auto from_lane = [&](int b) {
        const float lo_half = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f), b));
        if constexpr (TEAM == 32) {
          const float hi_half = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f), 32 + b));
          return half ? hi_half : lo_half;
        }
        return lo_half;
      };
      const bool in = lane < p.n_bands;
      if (p.decide == CRN_DECIDE_ANN_K) {
        const float nf = from_lane(0), ch1 = from_lane(1), ch2 = from_lane(2), ch3 = from_lane(3);
        ann_decide_team<TEAM>(p, w_ih, w_ho, epoch, active, lane, half, nf, ch1, ch2, ch3);
      } else if (p.decide == CRN_DECIDE_THRESHOLD_K) {
        const float ref = p.ref_band >= 0 ? from_lane(p.ref_band) : 1.0f;
        const bool occ = active && in && f > thr_lane * ref;
        if (active && in && p.occupancy != nullptr) p.occupancy[epoch * p.n_bands + lane] = (uint8_t)occ;
        unsigned long long m = __ballot(occ);
        if constexpr (TEAM == 32) m = (m >> half) & 0xffffffffull;
        if (active && t == 0 && p.decision != nullptr) p.decision[epoch] = __popcll(m);
      } else if (active) {
        if (t == 0 && p.decision != nullptr) p.decision[epoch] = 0;
        if (in && p.occupancy != nullptr) p.occupancy[epoch * p.n_bands + lane] = 0;
      }
      if (active && in && p.features != nullptr) p.features[epoch * p.n_bands + lane] = f;
    }
  } else {
    // descriptor of this lane's first band (one lane per band below): fetched now, used after the barriers
    int pre_s0 = 0, pre_s1 = 0, pre_lo = 0, pre_hi = 0;
    if (t < p.n_bands) {
      pre_s0 = tab[t];
      pre_s1 = tab[t + 1];
      if (pre_s1 > pre_s0) {
        pre_lo = tab[kTabSegLo + pre_s0];
        pre_hi = tab[kTabSegHi + pre_s0];
      }
    }
    if constexpr (G::XWAVE) __syncthreads();
    else wave_sync();
#pragma unroll
    for (int j = 0; j < J; j++)
#pragma unroll
      for (int d = 0; d < R3; d++) {
        // the pruned kernels never accumulate (or read back) the other registers
        if (((acc_mask<C>() >> (j * R3 + d)) & 1u) == 0) continue;
        // (S = 0 is written out where it has always stood: formed through the helper, the same value compiles to other instructions in
        // the twelve 4096-point kernels that close through this walk without kTw1C — tools/isa_diff.py)
        int k = a + 16 * (m_lo * J + j) + 256 * d;   // = bin_of<0>(lane_coord<0>(a, m_lo, j, J), d, N)
        if constexpr (BinMap<C>::S != 0) k = BinMap<C>::bin(a, m_lo, j, d);
        spec[spec_phys(k)] = acc[j * R3 + d];
      }
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;  // .cpp:287
    if constexpr (G::XWAVE) __syncthreads();
    else wave_sync();

    trace.stamp1();  // LDS form: spectrum image visible
    if (p.spectrum != nullptr && active) {
      float *dst = p.spectrum + epoch * N;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float x = spec[spec_phys(t + T * r)];
        dst[t + T * r] = sc_unscale<C>(MAG ? x : __fdiv_rn(x, Kf), p);
      }
    }

    // band sums (reference .cpp:173-191).  This stretch is pure latency (the wave has no loads in
    // flight beyond its prefetched frame), every LDS round trip queues behind the CU's exchange
    // traffic, and a dependent VALU chain issues one instruction per ~10 cycles — so the work is
    // spread over lanes instead of bands (one team per band, 16 bands in sequence per wave, cost
    // the 64-band Welch kernel 11 us per epoch, 40 % of the wave's time):
    //   every thread sums the 16 consecutive bins of "its" block (thread t: bins 16 t .. 16 t + 15,
    //   ascending like the reference) -> blk[t]; the 16 lanes of a DPP row add their block totals
    //   -> rows[t / 16] (256 bins);  then ONE LANE PER BAND walks its segments in steps of 256, 16
    //   and 1 bins (at most 15 + 15 + 16 + 15 + 15 reads), all bands at once.
    lds_f32 *blk = spec + Img::kBlk, *rows = spec + Img::kRows;
    {
      float bs = 0.f;
#pragma unroll
      for (int j = 0; j < 16; j++) bs += spec[17 * t + j];  // spec_phys(16 t + j)
      blk[t] = bs;
      float rs = dpp_add<0xB1>(bs);   // the 16 block totals of a 256-bin row sit in one DPP row
      rs = dpp_add<0x4E>(rs);
      rs = dpp_add<0x141>(rs);
      rs = dpp_add<0x140>(rs);
      if ((t & 15) == 0) rows[t >> 4] = rs;
    }
    if constexpr (G::XWAVE) __syncthreads();
    else wave_sync();
    // four block (or row) totals per LDS round trip, added in ascending order
    auto add_run = [&](float &sum, const lds_f32 *tot, int i, int n) {  // tot[i .. i + n)
      for (; n >= 4; n -= 4, i += 4) {
        const float a0 = tot[i], a1 = tot[i + 1], a2 = tot[i + 2], a3 = tot[i + 3];
        sum += a0;
        sum += a1;
        sum += a2;
        sum += a3;
      }
      for (; n > 0; n--, i++) sum += tot[i];
    };
    for (int b = t; b < p.n_bands; b += T) {
      float sum = 0.f;
      const bool first = b == t;  // this lane's first band: descriptor fetched before the barriers
      const int s0 = first ? pre_s0 : tab[b], s1 = first ? pre_s1 : tab[b + 1];
      for (int sg = s0; sg < s1; sg++) {
        int k = (first && sg == s0) ? pre_lo : tab[kTabSegLo + sg];
        const int hi = (first && sg == s0) ? pre_hi : tab[kTabSegHi + sg];
        while (k < hi && (k & 15) != 0) sum += spec[spec_phys(k++)];
        if (k + 16 <= hi) {
          // whole blocks up to the next row boundary, whole rows, whole blocks after them
          int n = ((hi - k) >> 4);                       // whole blocks available
          const int to_row = ((256 - (k & 255)) & 255) >> 4;  // blocks until k is row-aligned
          const int head = n < to_row ? n : to_row;
          add_run(sum, blk, k >> 4, head);
          k += head * 16;
          n -= head;
          const int nrows = n >> 4;
          add_run(sum, rows, k >> 8, nrows);
          k += nrows * 256;
          n -= nrows * 16;
          add_run(sum, blk, k >> 4, n);
          k += n * 16;
        }
        while (k < hi) sum += spec[spec_phys(k++)];
      }
      const float msum = MAG ? sc_unscale<C>(sum, p) : sum;
      featl[b] = MAG ? msum * msum : sc_unscale<C>(__fdiv_rn(sum, Kf), p);  // .cpp:194-197
    }
    trace.stamp2();  // LDS form: this wave's band sums done
    if constexpr (G::XWAVE) __syncthreads();
    else wave_sync();
    trace.stamp3();  // LDS form: every feature written

    feat = featl;

    // CFAR (kCfar): bin k is detected when P[k] > alpha Z[k], Z[k] the method's noise estimate from the 2 W training cells
    // g < |i| <= g + W around it, circular over the N bins (include/crn_sense.h, crn_cfar_method).  Every cell carries the same 1 / K,
    // so the test runs on the K-frame sums in the image with s = cfar_scale, rounded once to fp32 on the host: CA x[k] > s (T_L + T_R)
    // with s = alpha / 2 W, GO / SO x[k] > s max / min(T_L, T_R) with s = alpha / W, T_L and T_R the two sides' sums.  Thread t owns
    // bins 16 t .. 16 t + 15 (the band sums' blocks).  With y[i] = x[16 t - g - W + i] (left) and z[i] = x[16 t + g + 1 + i] (right),
    // bin 16 t + j's windows are y[j .. j+W-1] and z[j .. j+W-1].  The method is a launch parameter: one kernel holds all four.
    //   A window sum must never be formed by subtracting a cell that left it: a strong bin that enters and leaves a sliding fp32 sum
    //   leaves ~ulp32(strong bin) behind, 30-50 % of the training sum at 80-90 dB over the floor.
    //   W >= 16: every window contains position 15.  CA: T(16 t + j) = U[j] + (A + y[W] + ... + y[W+j-1]) + (B + z[W] + ... + z[W+j-1])
    //   with U[j] = (y[j] + z[j]) + U[j+1] (from U[15] = y[15] + z[15] down), A = y[16] + ... + y[W-1], B likewise (ascending, 0 at
    //   W = 16): fp32 additions of non-negative values only.  2 W + 46 LDS reads per thread and epoch.  GO / SO keep the sides apart:
    //   T_L(16 t + j) = U_L[j] + (A + y[W] + ... + y[W+j-1]) with U_L[j] = y[j] + U_L[j+1], T_R likewise.
    //   W < 16: the two sums slide, L(k+1) = (L(k) + x[k-g]) - x[k-g-W], R(k+1) = (R(k) - x[k+g+1]) + x[k+g+W+1], from ascending-distance
    //   sums at 16 t, in fp64 with the comparison: the residue of a strong bin is ~1e-16 of it (1e-7 of the floor at 90 dB).
    //   OS (s = alpha): bin k is detected when at least `rank` of its 2 W cells c have fl32(s c) < x[k], which is x[k] > fl32(alpha
    //   X_(rank)) because rounding is monotone: a count, no sort.  Cell-major, so that no register array is indexed at run time, in
    //   passes of B = 4 bins: each side's W + B - 1 cells of a pass are read once, scaled once and compared with the pass's bins that see
    //   them.  Cell q (0 <= q < W + B - 1, counted from the pass's first bin) is in bin j's windows for j <= q < j + W.  At W >= B the
    //   head cells q < B - 1 and the tail cells q >= W are unrolled (their bin ranges are compile-time) and the cells B - 1 <= q < W in
    //   between are seen by all B bins; below B each cell tests its range.
    // The 16 mask bits go to LDS as a half-word: lanes 2 w and 2 w + 1 form word w.  Then one lane per band counts its segments'
    // detected bins (popcount per 32-bit word); the team below stores them and decides.
    [[maybe_unused]] const lds_i32 *cfar_cnt = nullptr;
    if constexpr ((C::OPT & kCfar) != 0) {
      static_assert(!MAG && !C::SC16, "CFAR: energy mode, float samples");
      lds_u16 *mk16 = reinterpret_cast<lds_u16 *>(spec + Img::kMask);
      const lds_u32 *mk32 = reinterpret_cast<const lds_u32 *>(spec + Img::kMask);
      lds_i32 *cnt = reinterpret_cast<lds_i32 *>(spec + Img::kCnt);
      const int g = p.cfar_guard, W = p.cfar_train;
      const int k0 = 16 * t;
      const int yl = k0 - g - W, zl = k0 + g + 1;   // first cell of the left / right run
      const int method = p.cfar_method;
      unsigned bits = 0;
      if (method == CRN_CFAR_OS_K) {
        const float sc = p.cfar_scale;
        const int rank = p.cfar_rank;
        constexpr int B = 4;   // bins per pass: B counts and B bins beside the prefetched frame (8 of each spilled)
#pragma unroll
        for (int j0 = 0; j0 < 16; j0 += B) {
          float x[B];
          int n[B];
#pragma unroll
          for (int j = 0; j < B; j++) {
            x[j] = spec[17 * t + j0 + j];  // spec_phys(16 t + j0 + j)
            n[j] = 0;
          }
          // cell j0 + q of both runs against the pass's bins jlo .. jhi (bin j0 + j sees cells j0 + j .. j0 + j + W - 1)
          auto count = [&](int q, int jlo, int jhi) {
            const float cl = sc * spec[spec_phys((yl + j0 + q) & (N - 1))], cr = sc * spec[spec_phys((zl + j0 + q) & (N - 1))];
#pragma unroll
            for (int j = 0; j < B; j++)
              if (j >= jlo && j <= jhi) n[j] += (cl < x[j] ? 1 : 0) + (cr < x[j] ? 1 : 0);
          };
          if (W >= B) {
#pragma unroll
            for (int q = 0; q < B - 1; q++) count(q, 0, q);
            for (int q = B - 1; q < W; q++) count(q, 0, B - 1);
#pragma unroll
            for (int r = 0; r < B - 1; r++) count(W + r, r + 1, B - 1);
          } else {
            for (int q = 0; q < W + B - 1; q++) {
              const float cl = sc * spec[spec_phys((yl + j0 + q) & (N - 1))], cr = sc * spec[spec_phys((zl + j0 + q) & (N - 1))];
#pragma unroll
              for (int j = 0; j < B; j++)
                n[j] += (unsigned)(q - j) < (unsigned)W ? (cl < x[j] ? 1 : 0) + (cr < x[j] ? 1 : 0) : 0;
            }
          }
#pragma unroll
          for (int j = 0; j < B; j++) bits |= (n[j] >= rank ? 1u : 0u) << (j0 + j);
        }
      } else if (method == CRN_CFAR_CA_K) {
        if (W >= 16) {   // uniform
          const float sc = p.cfar_scale;
          float u[16];
          u[15] = spec[spec_phys((yl + 15) & (N - 1))] + spec[spec_phys((zl + 15) & (N - 1))];
#pragma unroll
          for (int q = 14; q >= 0; q--) u[q] = (spec[spec_phys((yl + q) & (N - 1))] + spec[spec_phys((zl + q) & (N - 1))]) + u[q + 1];
          float a = 0.f, b = 0.f;
          for (int q = 16; q < W; q++) {
            a += spec[spec_phys((yl + q) & (N - 1))];
            b += spec[spec_phys((zl + q) & (N - 1))];
          }
#pragma unroll
          for (int j = 0; j < 16; j++) {
            if (j > 0) {
              a += spec[spec_phys((yl + W + j - 1) & (N - 1))];
              b += spec[spec_phys((zl + W + j - 1) & (N - 1))];
            }
            const float x = spec[17 * t + j];  // spec_phys(16 t + j)
            bits |= (x > sc * (u[j] + (a + b)) ? 1u : 0u) << j;
          }
        } else {
          const double sd = (double)p.cfar_scale;
          double lsum = 0.0, rsum = 0.0;
          for (int i = g + 1; i <= g + W; i++) {
            lsum += spec[spec_phys((k0 - i) & (N - 1))];
            rsum += spec[spec_phys((k0 + i) & (N - 1))];
          }
#pragma unroll
          for (int j = 0; j < 16; j++) {
            const int k = k0 + j;
            const float x = spec[17 * t + j];
            bits |= ((double)x > sd * (lsum + rsum) ? 1u : 0u) << j;
            if (j < 15) {
              const float l_in = spec[spec_phys((k - g) & (N - 1))], l_out = spec[spec_phys((k - g - W) & (N - 1))];
              const float r_out = spec[spec_phys((k + g + 1) & (N - 1))], r_in = spec[spec_phys((k + g + W + 1) & (N - 1))];
              lsum = (lsum + (double)l_in) - (double)l_out;
              rsum = (rsum - (double)r_out) + (double)r_in;
            }
          }
        }
      } else {   // GO / SO: the same passes with max or min, each its own loop (no select, no sign constant held through the frame loop)
        auto go_so = [&](auto pick) {
          if (W >= 16) {   // uniform, in two halves of 8 bins (two suffix arrays of 16 spill); a and b carry over, so every sum is as above
            const float sc = p.cfar_scale;
            float a = 0.f, b = 0.f;
            for (int q = 16; q < W; q++) {
              a += spec[spec_phys((yl + q) & (N - 1))];
              b += spec[spec_phys((zl + q) & (N - 1))];
            }
#pragma unroll
            for (int j0 = 0; j0 < 16; j0 += 8) {
              float ul[8], ur[8];
              float sl = spec[spec_phys((yl + 15) & (N - 1))], sr = spec[spec_phys((zl + 15) & (N - 1))];
#pragma unroll
              for (int q = 15; q >= j0; q--) {
                if (q < 15) {
                  sl = spec[spec_phys((yl + q) & (N - 1))] + sl;
                  sr = spec[spec_phys((zl + q) & (N - 1))] + sr;
                }
                if (q < j0 + 8) {
                  ul[q - j0] = sl;
                  ur[q - j0] = sr;
                }
              }
#pragma unroll
              for (int j = j0; j < j0 + 8; j++) {
                if (j > 0) {
                  a += spec[spec_phys((yl + W + j - 1) & (N - 1))];
                  b += spec[spec_phys((zl + W + j - 1) & (N - 1))];
                }
                const float tl = ul[j - j0] + a, tr = ur[j - j0] + b;
                const float x = spec[17 * t + j];  // spec_phys(16 t + j)
                bits |= (x > sc * pick(tl, tr) ? 1u : 0u) << j;
              }
            }
          } else {
            const double sd = (double)p.cfar_scale;
            double lsum = 0.0, rsum = 0.0;
            for (int i = g + 1; i <= g + W; i++) {
              lsum += spec[spec_phys((k0 - i) & (N - 1))];
              rsum += spec[spec_phys((k0 + i) & (N - 1))];
            }
#pragma unroll
            for (int j = 0; j < 16; j++) {
              const int k = k0 + j;
              const float x = spec[17 * t + j];
              bits |= ((double)x > sd * pick(lsum, rsum) ? 1u : 0u) << j;
              if (j < 15) {
                const float l_in = spec[spec_phys((k - g) & (N - 1))], l_out = spec[spec_phys((k - g - W) & (N - 1))];
                const float r_out = spec[spec_phys((k + g + 1) & (N - 1))], r_in = spec[spec_phys((k + g + W + 1) & (N - 1))];
                lsum = (lsum + (double)l_in) - (double)l_out;
                rsum = (rsum - (double)r_out) + (double)r_in;
              }
            }
          }
        };
        if (method == CRN_CFAR_GO_K) go_so([](auto u, auto v) { return u > v ? u : v; });
        else go_so([](auto u, auto v) { return u < v ? u : v; });
      }
      mk16[t] = (unsigned short)bits;
      if constexpr (G::XWAVE) __syncthreads();
      else wave_sync();
      for (int b = t; b < p.n_bands; b += T) {
        int n = 0;
        for (int sg = tab[b], s1 = tab[b + 1]; sg < s1; sg++) {
          const int hi = tab[kTabSegHi + sg];
          for (int k = tab[kTabSegLo + sg]; k < hi;) {
            const int w = k >> 5, e = hi < ((w + 1) << 5) ? hi : ((w + 1) << 5);
            unsigned m = mk32[w] >> (k & 31);
            if (e - k < 32) m &= (1u << (e - k)) - 1u;
            n += __popc(m);
            k = e;
          }
        }
        cnt[b] = n;
      }
      if (active && p.cfar_mask != nullptr && t < N / 32) p.cfar_mask[epoch * (N / 32) + t] = mk32[t];
      if constexpr (G::XWAVE) __syncthreads();
      else wave_sync();
      cfar_cnt = cnt;
    }

    // LDS path: the first team of the group stores and decides.
    if (active && t < TEAM) {
      if (p.features != nullptr)
        for (int b = t; b < p.n_bands; b += TEAM) p.features[epoch * p.n_bands + b] = feat[b];

      if constexpr ((C::OPT & kCfar) != 0) {
        // CFAR: occupied = at least min_bins detected bins; the decision counts the occupied bands, as the threshold rule does
        int occ_bands = 0;
        for (int b0 = 0; b0 < p.n_bands; b0 += TEAM) {
          const int b = b0 + t;
          const bool in = b < p.n_bands;
          const int nb = in ? cfar_cnt[b] : 0;
          const bool occ = in && nb >= p.cfar_min_bins;
          if (in && p.occupancy != nullptr) p.occupancy[epoch * p.n_bands + b] = (uint8_t)occ;
          if (in && p.cfar_band_bins != nullptr) p.cfar_band_bins[epoch * p.n_bands + b] = nb;
          unsigned long long m = __ballot(occ);
          if constexpr (TEAM == 32) m = (m >> (tid & 32)) & 0xffffffffull;
          occ_bands += __popcll(m);
        }
        if (t == 0 && p.decision != nullptr) p.decision[epoch] = occ_bands;
      } else if (p.decide == CRN_DECIDE_ANN_K) {
        ann_decide_team<TEAM>(p, w_ih, w_ho, epoch, true, lane, TEAM == 32 ? (tid & 32) : 0, feat[0], feat[1], feat[2], feat[3]);
      } else if (p.decide == CRN_DECIDE_THRESHOLD_K) {
        // lane i takes bands i, i + TEAM, ...; the count of occupied bands is a ballot, not a serial walk
        {
          const float ref = p.ref_band >= 0 ? feat[p.ref_band] : 1.0f;
          int cnt = 0;
          for (int b0 = 0; b0 < p.n_bands; b0 += TEAM) {
            const int b = b0 + t;
            const bool in = b < p.n_bands;
            const bool occ = in && feat[in ? b : 0] > thr[in ? b : 0] * ref;
            if (in && p.occupancy != nullptr) p.occupancy[epoch * p.n_bands + b] = (uint8_t)occ;
            unsigned long long m = __ballot(occ);
            if constexpr (TEAM == 32) m = (m >> (tid & 32)) & 0xffffffffull;
            cnt += __popcll(m);
          }
          if (t == 0 && p.decision != nullptr) p.decision[epoch] = cnt;
        }
      } else {
        if (t == 0 && p.decision != nullptr) p.decision[epoch] = 0;
        if (p.occupancy != nullptr)
          for (int b = t; b < p.n_bands; b += TEAM) p.occupancy[epoch * p.n_bands + b] = 0;
      }
    }
  }
  // With one exchange buffer the next epoch's first frame syncs the workgroup before it writes
  // exchange 1 (frame_compute), which is after every wave has passed this point: no barrier here.
  if constexpr (G::XWAVE && C::NBUF == 2) __syncthreads();
  if constexpr (!G::XWAVE) wave_sync();
  trace.leave(p, epoch, active, t);
  if constexpr ((C::OPT & kPrioValu) != 0 && G::XWAVE) __builtin_amdgcn_s_setprio(0);
}

}  // namespace crn
#endif
