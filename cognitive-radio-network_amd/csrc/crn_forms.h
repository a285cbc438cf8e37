// crn_forms.h — which forms of the sensing kernel are compiled, and which of them a launch runs.  Plain host C++17 (no HIP construct:
// tests/harness compiles this and crn_forms.cpp with g++): the flag names, one row per compiled form (FormKey: the value of every Cfg
// parameter of crn_frame.h plus the kind of kernel), the facts a choice depends on (FormQuery) and the one rule (select_form).  The
// kernel units instantiate exactly the rows of their table (crn_sense_kernel.h: FormAt) and launch the row select_form names.
#ifndef CRN_FORMS_H
#define CRN_FORMS_H
#include <optional>

#include "crn_kernels.h"

namespace crn {

// OPT flags of a form (Cfg::OPT, crn_frame.h)
enum : int {
  kSpread = 4,   // next frame's loads issued from inside passes 1 and 2, one per radix-4 group
  kLdsBlk = 32,  // LDS reads as hand-written ds_read_b64 blocks (no ds_read2_b64 merging)
  kTw1C = 64,    // pass-1 twiddles stored compressed (9 instead of 15 complex values)
  kRows = 256,   // pass 3 and the accumulate limited to the registers that can hold a bin of the reference channel plan (ref_acc_mask)
  kMulti = 512,  // a workgroup streams through several consecutive epoch groups
  kPrioValu = 1024, // s_setprio 1 through the butterflies of passes 1 and 2 (where the prefetch loads issue)
#ifdef CRN_AB_VARIANTS
  kTrace = 4096,    // MEASUREMENT BUILD ONLY: time stamps of the workgroup start and the epoch close, written over the ann_out buffer (crn_frame_ab.h)
#endif
  kRegBands = 8192, // epoch close forms the band sums from registers (plans with n_row_entries > 0, no spectrum)
  kHannSym = 16384, // periodic Hann folded into pass 1's first butterflies (w[n + N/2] = 1 - w[n]): 8 window registers
  kTw2Early = 32768, // TW2LDS: the first block of pass-2 twiddles is read from LDS before the butterflies that precede its use
  kAlignedBands = 65536, // N = 4096, equal contiguous bands of 64 / 128 / 256 bins (p.aligned_shift): band sums by DPP + one barrier
  kSc16 = 131072,   // samples in HBM are the radio's wire format (two int16 per complex sample, 4 bytes): converted in pass 1
                    // (instantiated by crn_kernels_sc16.hip: a library built with make SC16=1)
  kDeal = 1048576,  // sense_kernel_dealt (launches of a few epochs): one epoch per workgroup, its frames dealt to the lane groups; pass 3
                    // parks each frame's per-bin values in LDS (ph_pass3_park) and the accumulate is replayed in frame order afterwards
  kCfar = 2097152,  // per-bin CA-CFAR on the LDS spectrum image after the band sums (crn_sense_set_cfar): bit mask, per-band counts and
                    // the decision in place of the threshold rule (epoch_close, LDS form only)
};

// The reference channel plan's accumulator registers
// The reference hard-codes its channel plan (bins 0-15 + 496-510, 55-84, 189-221, 300-309 of 512:
// CE_Predictive_Node.cpp:173-191).  At N = 4096 those bands touch 7 of the 16 blocks of 256 bins, and
// the last radix-4 level of pass 3 produces exactly one block per output: row d = bins
// [256 d, 256 d + 256).  For band tables inside these rows, and when no per-bin spectrum is asked
// for, pass 3 forms and accumulates only the needed outputs (bit-identical for those bins).
static constexpr unsigned kRefPlanRows = 0x8267u;  // rows {0, 1, 2, 5, 6, 9, 15}

// The same at every size.  After pass 3 thread (a, g) holds bin a + 16 (g J + j) + 256 d in accumulator register j R3 + d
// (J = 16 / R3, N = 256 R3): which of the 16 registers can hold a bin of the reference's channel plan scaled to N points — bit
// j R3 + d.  N = 4096: the rows above (J = 1: register = row), 7 of 16; N = 512: 7; N = 1024: 12; N = 2048: 11.  Band tables inside
// the mask, with no per-bin spectrum asked for, run kernels whose pass 3 forms and accumulates only those registers.
// ref_acc_mask_shifted: the same under the bin map of the kTw1C kernels (crn_kernels.h: bin_of<S>), every bin moved up by S.
constexpr unsigned ref_acc_mask_shifted(int R3, int S) {
  const int seg[5][2] = {{0, 16}, {496, 511}, {55, 85}, {189, 222}, {300, 310}};   // CE_Predictive_Node.cpp:173-191, of 512 bins
  const int J = 16 / R3, Sc = R3 / 2, N = 256 * R3;                                // Sc = N / 512
  unsigned mask = 0;
  for (int s = 0; s < 5; s++)
    for (int k = seg[s][0] * Sc; k < seg[s][1] * Sc; k++) {
      const int ks = (k + S) & (N - 1);
      mask |= 1u << ((((ks & 255) >> 4) % J) * R3 + (ks >> 8));
    }
  return mask;
}
constexpr unsigned ref_acc_mask(int R3) { return ref_acc_mask_shifted(R3, 0); }
static_assert(ref_acc_mask(16) == kRefPlanRows, "N = 4096: register = 256-bin row");
static_assert(ref_acc_mask(2) == 0x85e1u && ref_acc_mask(4) == 0xbf73u && ref_acc_mask(8) == 0x9f9bu, "7, 12 and 11 registers at 512, 1024 and 2048 points");
static_assert(ref_acc_mask_shifted(16, kTw1cRowShift) == kRefPlanRows, "N = 4096: the plan reaches the same seven rows when they start 7 bins early");

// LDS behind the exchange buffers and the tw2 table, used by the epoch close: the band table copy,
// then [8 teams][16] per-team band partials of the register path.
constexpr int kCloseLdsBytes = kBandTabWords * 4 + 8 * 16 * 4;

// The sensing kernel's dynamic LDS, stated once for the kernels, their launches and crn_sense_kernel_info: byte offsets from the start
// of the segment for a form of size r3 with nbuf exchange buffers, streaming or dealt.
struct LdsLayout {
  int group_bytes;   // a lane group's exchange buffers, nbuf x [16][T + R3] complex: group g's at g * group_bytes (the LDS close lays its
                     // image of the spectrum over them)
  int tw2;           // [16][R3] complex: the pass-2 twiddle table (read by the TW2LDS forms; every form leaves the room)
  int tab;           // the band-table copy, kBandTabWords words
  int part;          // [8 teams][16] floats: per-team band partials of the register close
  int bytes;         // all of the above: what a streaming launch asks for
  int slots;         // dealt forms: the frame slots, [rounds x lane groups] of N per-bin values each (0: a streaming form has none)
  int round_values;  // values one round of slots holds: lane groups x N
  constexpr size_t bytes_with_slots(int rounds, bool mag) const { return (size_t)bytes + (slots != 0 ? (size_t)rounds * round_values * (mag ? 4 : 8) : 0); }
};
constexpr LdsLayout lds_layout(int r3, int nbuf, bool dealt) {
  const int t = 16 * r3, groups = 256 / t, cplx = 8;
  LdsLayout l{};
  l.group_bytes = nbuf * 16 * (t + r3) * cplx;
  l.tw2 = groups * l.group_bytes;
  l.tab = l.tw2 + 16 * r3 * cplx;
  l.part = l.tab + kBandTabWords * 4;
  l.bytes = l.tab + kCloseLdsBytes;
  l.slots = dealt ? l.bytes : 0;
  l.round_values = groups * 256 * r3;
  return l;
}

// A compiled form: one row of a unit's table
// (Cfg's PREFETCH and PK are true in every form.)  The with-functions let a table row and the rule below name what a form has
// instead of listing ten positional values.
struct FormKey {
  int r3, nbuf;
  bool nt, mag, win, tw2lds;
  int occ;
  bool full;
  int opt;
  bool dealt;   // sense_kernel_dealt (one epoch per workgroup) instead of sense_kernel
  constexpr FormKey magnitude(bool m = true) const { FormKey k = *this; k.mag = m; return k; }        // |X| mode (CRN_MODE_REF_MAG)
  constexpr FormKey window() const { FormKey k = *this; k.win = true; return k; }                     // multiplies by the window table
  constexpr FormKey tw2_from_lds() const { FormKey k = *this; k.tw2lds = true; return k; }            // pass-2 twiddles: LDS table, not 30 registers
  constexpr FormKey per_cu(int n) const { FormKey k = *this; k.occ = n; return k; }                   // workgroups per CU the registers must allow
  constexpr FormKey whole(bool f = true) const { FormKey k = *this; k.full = f; return k; }           // every frame brings N samples: no padding mask
  constexpr FormKey buffers(int n) const { FormKey k = *this; k.nbuf = n; return k; }                 // LDS exchange buffers
  constexpr FormKey with(int flags) const { FormKey k = *this; k.opt |= flags; return k; }
  constexpr FormKey without(int flags) const { FormKey k = *this; k.opt &= ~flags; return k; }
};
constexpr bool operator==(const FormKey &a, const FormKey &b) {
  return a.r3 == b.r3 && a.nbuf == b.nbuf && a.nt == b.nt && a.mag == b.mag && a.win == b.win && a.tw2lds == b.tw2lds && a.occ == b.occ &&
         a.full == b.full && a.opt == b.opt && a.dealt == b.dealt;
}
// The two kinds of kernel.  Streaming: nontemporal loads, twiddles in registers, 3 workgroups per CU, frames masked at run time,
// energy mode, closed through the LDS walk — until a row says otherwise.  Dealt: one workgroup per CU slot, plain loads.
constexpr int kStreamFlags = kSpread | kLdsBlk | kPrioValu | kMulti, kDealtFlags = kSpread | kLdsBlk | kDeal;
constexpr FormKey streaming(int r3, int opt = 0) { return FormKey{r3, 1, true, false, false, false, 3, false, kStreamFlags | opt, false}; }
constexpr FormKey dealt_frames(int r3, int opt = 0) { return FormKey{r3, 1, false, false, false, false, 1, false, kDealtFlags | opt, true}; }

template <int CAP>
struct FormTable {
  FormKey row[CAP]{};
  int n = 0;
  constexpr void add(const FormKey &k) { row[n++] = k; }   // (a row too many does not compile: the write is outside the array)
  constexpr int find(const FormKey &k) const {
    for (int i = 0; i < n; i++) if (row[i] == k) return i;
    return -1;
  }
};

// What is compiled, per transform size: the rows crn_kernels.hip (float samples) and crn_kernels_sc16.hip (wire format: every row
// carries kSc16) instantiate.  select_form below says when each one runs.
template <int CAP>
constexpr void add_forms_of_size(FormTable<CAP> &t, int r3, bool wire) {
  const int x = wire ? kSc16 : 0;
  if (r3 <= 4) {   // launches of a few epochs: |X| or energy, band sums from registers or through the LDS walk; the periodic Hann
    for (int mag = 0; mag < 2; mag++) {
      t.add(dealt_frames(r3, x).magnitude(mag != 0));
      t.add(dealt_frames(r3, x | kRegBands).magnitude(mag != 0));
    }
    t.add(dealt_frames(r3, x | kHannSym).window());
  }
  // windowed: the Welch configuration's kernel (periodic Hann folded into pass 1, whole frames, energy), at N = 4096 also with the
  // aligned-band close; table windows, one form per mode
  t.add(streaming(r3, x | kHannSym | kTw2Early).window().tw2_from_lds().whole());
  if (r3 == 16) t.add(streaming(r3, x | kHannSym | kTw2Early | kAlignedBands).window().tw2_from_lds().whole());
  t.add(streaming(r3, x).window().tw2_from_lds());
  t.add(streaming(r3, x).window().tw2_from_lds().magnitude());
  // no window, any plan, spectrum requests: the LDS walk.  |X| masks at run time; energy has a whole-frame form (at N = 4096 that one
  // is the plain kernel below)
  t.add(streaming(r3, x).magnitude());
  t.add(streaming(r3, x));
  if (r3 != 16) t.add(streaming(r3, x).whole());
  // a small plan: the register close for |X| (any packet length) and for energy on whole frames
  t.add(streaming(r3, x | kRegBands).magnitude());
  if (r3 != 16) t.add(streaming(r3, x | kRegBands).whole());
  if (wire) {
    t.add(streaming(r3, x | kRegBands));   // the reference plan's short packets: from registers, every row (no plan-specific pruning in wire format)
  } else {
    // the reference channel plan: pass 3 and the accumulate keep its registers only — |X| and energy, whole frames and short packets
    t.add(streaming(r3, kRegBands | kRows).magnitude());
    t.add(streaming(r3, kRegBands | kRows).magnitude().whole());
    t.add(streaming(r3, kRegBands | kRows));
    if (r3 != 16) t.add(streaming(r3, kRegBands | kRows).whole());
  }
  if (r3 == 16) {   // the plain 4096-point kernel (energy, no window, whole frames): compressed pass-1 table, pass 2 from LDS, 4 per CU
    const FormKey plain = streaming(r3, x | kTw1C).tw2_from_lds().per_cu(4).whole();
    t.add(plain.with(kRows | kRegBands));
    t.add(plain.with(kRegBands));
    t.add(plain);
  }
  if (!wire) {   // CFAR (energy mode, float samples): the frame loop of the CFAR-off form, closed through the LDS walk with the CFAR pass
    const int win_per_cu = r3 == 16 ? 3 : 2;
    t.add(streaming(r3, kCfar | kHannSym | kTw2Early).window().tw2_from_lds().per_cu(win_per_cu).whole());
    t.add(streaming(r3, kCfar).window().tw2_from_lds().per_cu(win_per_cu));
    if (r3 == 16) t.add(streaming(r3, kCfar | kTw1C).tw2_from_lds().per_cu(4).whole());
    t.add(streaming(r3, kCfar));
  }
}

#ifdef CRN_AB_VARIANTS
// MEASUREMENT BUILD ONLY (libcrnsense_ab.so): the forms crn_sense_set_variant selects besides the product's two (13 = default,
// 2 = unpruned) — combinations of the shipped flags, and the build with in-kernel time stamps (kTrace).  Whole frames, energy mode.
//    7  the default without the wave-priority raise in passes 1 and 2
//   17  the default + time stamps of the epoch close in the ann_out buffer (windowed handles: the Welch kernel with stamps)
//   19  windowed kernels: Hann folded into pass 1's first butterflies          20  = 19 + early pass-2 twiddle reads (what ships)
//   21  windowed kernels: early pass-2 twiddle reads alone                     22  the plain windowed kernel (table window)
//   26  the Welch kernel with pass-2 twiddles in registers, 2 workgroups / CU  27  = 26 + two exchange buffers (one barrier per frame)
constexpr int kMeasurementForms = 20;
template <int CAP>
constexpr void add_measurement_forms(FormTable<CAP> &t) {
  for (int r3 = 2; r3 <= 16; r3 *= 2) {   // 19, 21, 22 (20 is the product's Welch form), every size
    const FormKey w = streaming(r3).window().tw2_from_lds().whole();
    t.add(w.with(kHannSym));
    t.add(w.with(kTw2Early));
    t.add(w);
  }
  const FormKey w26 = streaming(16, kHannSym).window().per_cu(2).whole();   // 26, 27: N = 4096, with and without the aligned-band close
  t.add(w26);
  t.add(w26.with(kAlignedBands));
  t.add(w26.buffers(2));
  t.add(w26.buffers(2).with(kAlignedBands));
  const FormKey plain = streaming(16, kTw1C).tw2_from_lds().per_cu(4).whole();   // 7, 17: the plain 4096-point kernel
  t.add(plain.without(kPrioValu).with(kRows | kRegBands));
  t.add(plain.without(kPrioValu));
  t.add(plain.with(kRows | kRegBands | kTrace));
  t.add(streaming(16, kTrace).window().tw2_from_lds().whole());                  // 17 on a windowed handle
}
#else
constexpr int kMeasurementForms = 0;   // the shipped library carries no measurement form
#endif

constexpr int kNumFloatForms = 72 + kMeasurementForms, kNumWireForms = 48;
constexpr FormTable<kNumFloatForms> make_float_forms() {
  FormTable<kNumFloatForms> t;
  for (int r3 = 2; r3 <= 16; r3 *= 2) add_forms_of_size(t, r3, false);
#ifdef CRN_AB_VARIANTS
  add_measurement_forms(t);
#endif
  return t;
}
constexpr FormTable<kNumWireForms> make_wire_forms() {
  FormTable<kNumWireForms> t;
  for (int r3 = 2; r3 <= 16; r3 *= 2) add_forms_of_size(t, r3, true);
  return t;
}
inline constexpr FormTable<kNumFloatForms> kFloatForms = make_float_forms();   // crn_kernels.hip
inline constexpr FormTable<kNumWireForms> kWireForms = make_wire_forms();      // crn_kernels_sc16.hip
static_assert(kFloatForms.n == kNumFloatForms && kWireForms.n == kNumWireForms, "every slot of a table is a form");

// Which form a launch runs
struct FormQuery {
  int fft_len;
  bool sc16;                          // wire-format samples (crn_kernels_sc16.hip's table)
  bool mag, win, hann_sym;
  bool whole_frames;                  // L == N
  bool cfar_on, spectrum, aligned;    // CFAR on; a per-bin spectrum is asked for; SenseParams::aligned_shift != 0
  int variant;                        // crn_sense_set_variant (0 = the default, 13)
  bool dealt;                         // SenseParams::deal_rounds > 0: a launch of a few epochs
  int n_row_entries;                  // the band plan cut into register rows, and the registers it reaches ...
  unsigned acc_mask;
  int n_row_entries_shift;            // ... and the same for the kTw1C kernels, whose rows start kTw1cRowShift bins early
  unsigned acc_mask_shift;
};
FormQuery make_form_query(const SenseParams &p, int fft_len, bool mag, bool win, int variant, bool sc16);
// The form, a row of the unit's table (kWireForms when q.sc16, else kFloatForms); nothing where no form exists (hipErrorInvalidValue).
std::optional<FormKey> select_form(const FormQuery &q);

// What crn_sense_kernel_info reports of a form.
struct FormGeometry {
  int threads, lds_bytes, epochs_per_block;   // (lds_bytes: without the frame slots a dealt launch adds, sense_deal_rounds)
};
FormGeometry form_geometry(const FormKey &k);
void form_name(const FormKey &k, char *name, size_t name_len);   // "sense_kernel<R3=..,..,CLOSE=..>"

int sense_num_variants();
// Rounds of dealt frames (ceil(K / lane groups)) when sense_kernel_dealt can take this size / mode / window / K — N <= 1024, no window or
// the periodic Hann on whole frames in energy mode, and the frame slots fit in the device's LDS per workgroup (lds_budget_bytes:
// hipDeviceAttributeMaxSharedMemoryPerBlock, 160 KiB on gfx950) — else 0: the streaming kernel takes the launch.
int sense_deal_rounds(int fft_len, bool mag, bool win, bool hann_whole_frames, int frames_per_epoch, size_t lds_budget_bytes);
unsigned sense_ref_acc_mask(int fft_len);    // accumulator registers (bit j R3 + d) the reference channel plan reaches at this size
bool sense_variant_available(int variant);   // the shipped library carries 0 (= 13) and 2; libcrnsense_ab.so the measurement forms too
bool sense_variant_traces(int variant);      // a measurement form that writes time stamps over the ann_out buffer (never in the shipped library)

}  // namespace crn
#endif
