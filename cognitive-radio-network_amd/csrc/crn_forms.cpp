// crn_forms.cpp — the rule that picks a sensing-kernel form (select_form) and the host-side facts about forms and variants.  Plain C++:
// compiled into the library, and as it is into the unit programs of tests/harness.
#include "crn_forms.h"

#include <cstdio>

namespace crn {

// Kernel forms selectable through crn_sense_set_variant (0 = default).  The shipped library (libcrnsense.so) compiles the two that are
// forms of the product — 13 (= 0, the default) and 2 (no pass-3 row pruning: what any band table outside the reference plan's rows runs
// anyway) — and refuses every other number.  libcrnsense_ab.so (-DCRN_AB_VARIANTS; tools/ and the A/B test) adds the measurement forms
// (crn_forms.h: add_measurement_forms).  The numbers are the ones profiles/ and docs/history/ quote; the schedules, ablations
// and layouts of rounds 1-4 that were measured and not kept are gone from the tree (docs/history/removed_variants.md).
static constexpr int kNumVariants = 27, kDefaultVariant = 13;
#ifdef CRN_AB_VARIANTS
static bool measurement_variant(int v) { return v == 7 || v == 17 || (v >= 19 && v <= 22) || v == 26 || v == 27; }
bool sense_variant_traces(int v) { return v == 17; }
#else
static bool measurement_variant(int) { return false; }
bool sense_variant_traces(int) { return false; }
#endif
int sense_num_variants() { return kNumVariants; }
bool sense_variant_available(int v) { return v == 0 || v == kDefaultVariant || v == 2 || measurement_variant(v); }
unsigned sense_ref_acc_mask(int fft_len) { return ref_acc_mask(fft_len / 256); }

int sense_deal_rounds(int fft_len, bool mag, bool win, bool hann_whole_frames, int K, size_t lds_budget) {
  if (fft_len != 512 && fft_len != 1024) return 0;
  if (win && (mag || !hann_whole_frames)) return 0;   // the one windowed dealt form: periodic Hann, energy mode, whole frames
  if (K < 2) return 0;   // one frame: nothing to deal
  const int r3 = fft_len / 256, groups = 256 / (16 * r3);
  const int rounds = (K + groups - 1) / groups;
  const size_t lds = lds_layout(r3, 1, true).bytes_with_slots(rounds, mag);
  return lds <= lds_budget ? rounds : 0;
}

FormGeometry form_geometry(const FormKey &k) {
  return FormGeometry{256, lds_layout(k.r3, k.nbuf, k.dealt).bytes, k.dealt ? 1 : 256 / (16 * k.r3)};
}

void form_name(const FormKey &k, char *name, size_t name_len) {
  char prune_note[64] = "";
  if ((k.opt & kRows) != 0)   // (the same seven rows in both labellings at N = 4096)
    std::snprintf(prune_note, sizeof(prune_note), ",PASS3_ROWS=%d-of-16(reference channel plan)", __builtin_popcount(ref_acc_mask(k.r3)));
  std::snprintf(name, name_len, "sense_kernel<R3=%d,NBUF=%d,PREFETCH=1,NT=%d,TW2LDS=%d,PK=1,MAG=%d,WIN=%s,CLOSE=%s%s>", k.r3, k.nbuf, k.nt,
                k.tw2lds, k.mag, !k.win ? "0" : (k.opt & kHannSym) != 0 ? "hann-in-pass1" : "table",
                (k.opt & kCfar) != 0 ? "lds+cfar" : (k.opt & kAlignedBands) != 0 ? "aligned-bands(dpp)" : (k.opt & kRegBands) != 0 ? "registers" : "lds",
                prune_note);
}

FormQuery make_form_query(const SenseParams &p, int fft_len, bool mag, bool win, int variant, bool sc16) {
  return FormQuery{fft_len, sc16, mag, win, p.hann_sym != 0, p.L == fft_len, p.cfar_on != 0, p.spectrum != nullptr, p.aligned_shift != 0, variant,
                   p.deal_rounds > 0, p.n_row_entries, p.acc_mask, p.n_row_entries_shift, p.acc_mask_shift};
}

#ifdef CRN_AB_VARIANTS
// MEASUREMENT BUILD ONLY: the form a measurement variant (the list is in crn_forms.h) runs in place of the product's; whole frames,
// energy mode, streaming.  Nothing for the launches it leaves to the rule below.
static std::optional<FormKey> select_measurement_form(const FormQuery &q, int r3, bool ref_rows_shift) {
  const int v = q.variant;
  if (!measurement_variant(v) || q.mag || !q.whole_frames) return std::nullopt;
  if (r3 == 16) {
    if (q.win && q.hann_sym && (v == 26 || v == 27))
      return streaming(r3, kHannSym | (q.aligned ? kAlignedBands : 0)).window().per_cu(2).whole().buffers(v == 27 ? 2 : 1);
    if (q.win && v == 17) return streaming(r3, kTrace).window().tw2_from_lds().whole();   // close stamps for the windowed / Welch kernel
    if (!q.win && (v == 7 || v == 17)) {
      const FormKey plain = streaming(r3, kTw1C).tw2_from_lds().per_cu(4).whole();
      if (v == 17) return plain.with(kRows | kRegBands | kTrace);
      return ref_rows_shift ? plain.without(kPrioValu).with(kRows | kRegBands) : plain.without(kPrioValu);
    }
  }
  if (q.win && v >= 19 && v <= 22) {
    const FormKey w = streaming(r3).window().tw2_from_lds().whole();
    if (v == 19 && q.hann_sym) return w.with(kHannSym);
    if (v == 20 && q.hann_sym) return w.with(kHannSym | kTw2Early);
    if (v == 21) return w.with(kTw2Early);
    return w;
  }
  return std::nullopt;
}
#endif

std::optional<FormKey> select_form(const FormQuery &q) {
  if (q.fft_len != 512 && q.fft_len != 1024 && q.fft_len != 2048 && q.fft_len != 4096) return std::nullopt;
  const int r3 = q.fft_len / 256;
  const int x = q.sc16 ? kSc16 : 0;   // every wire-format form carries the flag
  // The band plan.  The register form of the epoch close applies to plans the host could cut into row entries (crn_tables.cpp) when no
  // per-bin spectrum is stored ...
  const bool reg_bands = q.n_row_entries > 0 && !q.spectrum;
  // ... and pass 3 / the accumulate keep only the reference channel plan's registers when every band bin sits in one of them: 7 of 16
  // at N = 512 (where the reference's |X| costs a square root per bin and frame), 12 / 11 / 7 at 1024 / 2048 / 4096.
  const bool ref_rows = reg_bands && ref_acc_mask(r3) != 0xFFFFu && (q.acc_mask & ~ref_acc_mask(r3)) == 0;
  // The same two questions for the kTw1C kernels (the plain 4096-point forms), whose register rows start kTw1cRowShift bins early: the
  // entries cut at those rows, and the reference plan's rows among them (ref_acc_mask_shifted: the same seven).
  const bool reg_bands_shift = q.n_row_entries_shift > 0 && !q.spectrum;
  const bool ref_rows_shift = reg_bands_shift && (q.acc_mask_shift & ~ref_acc_mask_shifted(16, kTw1cRowShift)) == 0;
  // Which close a launch gets is ONE rule for the streaming and the dealt-frame kernels (their outputs are bit-identical because they sum
  // in the same order): the register close for |X| mode, and for energy mode on whole frames or on the reference plan; the LDS walk
  // otherwise (energy mode, short packets, another small plan; every plan too big for row entries; every spectrum request).
  const bool register_close = reg_bands && (q.mag || q.whole_frames || ref_rows);
  // Periodic Hann (the Welch configuration), whole frames, energy mode: the window rides in pass 1's first butterflies
  const bool welch = q.win && !q.mag && q.hann_sym && q.whole_frames;

  // A handle with CFAR on (crn_sense_set_cfar; energy mode, float samples — on wire-format samples the API refuses the call, and the
  // flag is not looked at): the frame loop of the form the same handle runs with CFAR off — so that the spectrum and the features are
  // the same bits — closed through the LDS walk with the CFAR pass (crn_epoch_close.h).  No register-band, pruned-row, aligned-band or
  // dealt forms.
  if (q.cfar_on && !q.sc16) {
    if (q.mag) return std::nullopt;
    // The windowed forms below 4096 points take two workgroups per CU: at three their frame loop spills (as the CFAR-off forms do),
    // and a scratch reload in the loop waits behind the prefetch.
    const int win_per_cu = r3 == 16 ? 3 : 2;
    if (welch) return streaming(r3, kCfar | kHannSym | kTw2Early).window().tw2_from_lds().per_cu(win_per_cu).whole();
    if (q.win) return streaming(r3, kCfar).window().tw2_from_lds().per_cu(win_per_cu);
    if (r3 == 16 && q.whole_frames) return streaming(r3, kCfar | kTw1C).tw2_from_lds().per_cu(4).whole();
    return streaming(r3, kCfar);
  }

  // A launch of a few epochs (crn_api.cpp sets deal_rounds): one epoch per workgroup, frames dealt to its lane groups.  Sizes whose
  // frames stay inside one wave; short frames are masked at run time.
  if (q.dealt && r3 <= 4) {
    // The windowed dealt-frame form: periodic Hann on whole frames in energy mode, riding in pass 1's first butterflies (kHannSym)
    // exactly as the streaming rule picks it for the same launch, so that the arithmetic is the same bit for bit — what the engine's
    // `-m welch` / `-m scan` launch.  (Other windows and |X| mode have no dealt form: sense_deal_rounds says 0 for them, and this rule
    // does not ask again.)  Windowed kernels close through the LDS walk.
    if (q.win) return dealt_frames(r3, x | kHannSym).window();
    return dealt_frames(r3, x | (register_close ? kRegBands : 0)).magnitude(q.mag);
  }

#ifdef CRN_AB_VARIANTS
  if (!q.sc16)
    if (const std::optional<FormKey> k = select_measurement_form(q, r3, ref_rows_shift)) return k;
#endif

  // Windowed kernels (16 window registers, and for Welch three half-frame sets) read the pass-2 twiddles from LDS at every size: in
  // registers they spill inside the frame loop.  3 workgroups per CU (they carry 16 more registers than the plain ones: the window).
  if (welch) {
    // ... and the first block of pass-2 twiddles is read ahead of its use (+1 % on the Welch stream, and 8 window registers fewer;
    // the A/B numbers are in docs/history/DESIGN_r03.md §5).  A windowed handle runs this whatever plain-kernel variant it selects.
    // The Welch scan's plan at N = 4096 (equal contiguous bands): band sums without the spectrum image.
    const int aligned = r3 == 16 && q.aligned ? kAlignedBands : 0;
    return streaming(r3, x | kHannSym | kTw2Early | aligned).window().tw2_from_lds().whole();
  }
  if (q.win) return streaming(r3, x).window().tw2_from_lds().magnitude(q.mag);   // table windows: one form per mode, masked at run time

  // The plain 4096-point kernel runs 4 workgroups per CU with the compressed pass-1 table and pass 2 from LDS.
  // (kTw1C: its register rows start 7 bins early — BinMap — so the plan is judged by the entries and the mask cut at those rows)
  if (r3 == 16 && !q.mag && q.whole_frames) {
    const FormKey plain = streaming(r3, x | kTw1C).tw2_from_lds().per_cu(4).whole();
    // the reference channel plan's rows only (the default, 13); variant 2 of the float unit never prunes
    if (ref_rows_shift && (q.sc16 || q.variant != 2)) return plain.with(kRows | kRegBands);
    // another plan, a per-bin spectrum request, or variant 2: no pruning
    return reg_bands_shift ? plain.with(kRegBands) : plain;
  }

  // Everything else: 3 workgroups per CU, all 30 twiddles in registers (4 per CU with the compressed tables was measured at the
  // smaller sizes: equal at 1024, -3 % at 512, -7 % at 2048), streaming workgroups (+2.5-3 % everywhere; N = 1024 used to spill with
  // them until the epoch close was slimmed).  What is specialised is what BASELINE.json's configurations and the engine run: whole
  // frames (no zero-padding mask) where the band plan is the reference's (kRows | kRegBands) or a small one in energy mode
  // (kRegBands); everything else — |X| mode with another plan or a spectrum request, short packets with a small custom plan — runs
  // ONE form that masks at run time (and closes through the LDS walk where the register close has no form).
  if (register_close) {
    // (the wire-format unit has no plan-specific pruning: it closes the reference plan's short packets from registers all the same —
    // the same sums in the same order as the float path's pruned form)
    const bool rows = ref_rows && !q.sc16;
    const FormKey k = streaming(r3, x | kRegBands | (rows ? kRows : 0));
    if (q.mag) return k.magnitude().whole(rows && q.whole_frames);   // |X| on another small plan: any packet length, one form
    return k.whole(q.whole_frames);   // (energy on short packets gets here on the reference plan only: register_close)
  }
  if (q.mag) return streaming(r3, x).magnitude();   // any plan, spectrum requests: the LDS walk
  return streaming(r3, x).whole(q.whole_frames);
}

}  // namespace crn
