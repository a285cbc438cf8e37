// crn_kernels.h — kernel parameter blocks shared by the kernel translation units and the host code that fills them (internal).
#ifndef CRN_KERNELS_H
#define CRN_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crn {

constexpr int kBandTabWords = 656;   // SenseParams::band_tab, copied to LDS by every workgroup
constexpr int kRowEntryWords = 32;   // row-entry slots of the register-resident band sums: 32 / R3 per row
// band_tab's layout, word offset and length of every region (written by crn_tables.cpp, thresholds and weights rewritten in place by
// crn_updates.cpp, read from LDS by crn_epoch_close.h)
constexpr int kTabSegBegin = 0, kTabSegBeginWords = 96;              // band_seg_begin: n_bands + 1 words
constexpr int kTabSegLo = 96, kTabSegHi = 256, kTabSegWords = 160;   // seg_lo, seg_hi: one word per segment each
constexpr int kTabThresh = 416, kTabThreshWords = 80;                // thresh (float bits), one per band
constexpr int kTabRowEntries = 512;   // kRowEntryWords entries band<<18 | lo<<9 | hi, 32 / R3 slots per 256-bin row, 0 = unused (only when n_row_entries > 0)
constexpr int kTabWih = 544, kTabWihWords = 60, kTabWho = 604, kTabWhoWords = 48;   // ann_w_ih as 30 doubles, ann_w_ho as 24 doubles
static_assert(kTabSegBegin + kTabSegBeginWords <= kTabSegLo && kTabSegLo + kTabSegWords <= kTabSegHi && kTabSegHi + kTabSegWords <= kTabThresh &&
              kTabThresh + kTabThreshWords <= kTabRowEntries && kTabRowEntries + kRowEntryWords <= kTabWih && kTabWih % 2 == 0 &&
              kTabWih + kTabWihWords <= kTabWho && kTabWho + kTabWhoWords <= kBandTabWords, "band_tab: regions in order, disjoint, inside the table");

// Which bin an accumulator register holds after pass 3, stated once for the kernels and the host tables.  Thread (a, g) — a = t / R3 the
// pass-1 row, g = t % R3 — holds in register j R3 + d (J = 16 / R3, j < J, d < R3) the bin
//   bin_of<S>(q, d) = 256 d - S + q (mod N),  q = lane_coord<S>(a, g, j) = ((a + S) & 15) + 16 (g J + j) in 0..255.
// S = 0 is the plain labelling a + 16 (g J + j) + 256 d.  The kernels that keep their pass-1 twiddles compressed (kTw1C, crn_frame.h) run
// pass-1 rows 9..15 as the negative frequencies a - 16 (a 16-point DFT's output index is periodic, and W_N^{t (a - 16)} is the conjugate
// of a stored twiddle), so their register row d covers bins [256 d - 7, 256 d + 249): S = kTw1cRowShift, the same offset for every lane.
constexpr int kTw1cRowShift = 7;
// (S is a template argument and the S = 0 branch the only code those instantiations hold: in the kernels the plain forms must stay the
// expression they have always been — a branch on a function argument, folded later, compiled the 4096-point LDS close differently)
template <int S>
constexpr int lane_coord(int a, int g, int j, int J) {
  if constexpr (S == 0) return a + 16 * (g * J + j);
  else return ((a + S) & 15) + 16 * (g * J + j);
}
template <int S>
constexpr int bin_of(int q, int d, int N) {
  if constexpr (S == 0) return q + 256 * d;
  else return (q + 256 * d - S) & (N - 1);
}

enum { CRN_DECIDE_ANN_K = 0, CRN_DECIDE_THRESHOLD_K = 1, CRN_DECIDE_NONE_K = 2 };  // == crn_decide
enum { CRN_CFAR_CA_K = 0, CRN_CFAR_GO_K = 1, CRN_CFAR_SO_K = 2, CRN_CFAR_OS_K = 3 };     // == crn_cfar_method

struct SenseParams {
  // input stream
  const float2 *iq;        // device, interleaved complex fp32
  long long n_epochs;
  long long epoch_stride;  // samples between epoch starts
  long long total_samples; // samples the batch holds (loads beyond it return zero)
  int frame_stride;        // samples between frame starts inside an epoch
  int L;                   // samples taken per frame (zero-padded to N)
  int K;                   // frames per epoch
  int groups_per_wg;       // consecutive epoch groups one workgroup streams through (>= 1)
  long long n_big_wgs;     // workgroups [0, n_big_wgs) take groups_per_wg groups each; the ones after them
                           // tail_groups_per_wg each (they are dispatched last: the end of the kernel drains in small steps)
  int tail_groups_per_wg;  // >= 1 (1 for the plain kernels; the Welch stream, which re-reads one half-frame per workgroup span,
                           // keeps its tail workgroups longer)
  // tables (device, built at crn_sense_create)
  const float2 *tw1;       // [17][T]  W_N^{t a}, a = 0..16
  const float2 *tw2;       // [16][R3] W_T^{m c}
  const float *window;     // [N] or null
  const int *band_tab;        // [kBandTabWords] packed copy of the tables below, staged into LDS by every workgroup (layout: kTab* above)
  const int *band_seg_begin;  // [n_bands + 1] into seg_lo/seg_hi (segments grouped by band)
  const int *seg_lo;
  const int *seg_hi;
  const float *thresh;     // [n_bands]
  const double *ann_w_ih;  // [5][6]
  const double *ann_w_ho;  // [6][4]
  double ann_threshold;
  int n_bands;
  int decide;
  int ref_band;
  int n_row_entries;       // > 0: band sums from registers (epoch_close); entries in band_tab
  int aligned_shift;       // N = 4096 and the plan is n_bands equal contiguous bands of 2^aligned_shift bins (6..8), else 0
  int hann_sym;            // the window table is a periodic Hann: w[n + N/2] = 1 - w[n] (may be folded into pass 1)
  unsigned acc_mask;       // bit j R3 + d set when some band holds a bin of the form a + 16 (g J + j) + 256 d, i.e. when accumulator
                           // register j R3 + d of some thread holds a band bin (N = 4096: bit d = the 256-bin row d)
  int deal_rounds;         // > 0: sense_kernel_dealt (one epoch per workgroup, its frames dealt to the lane groups, this many rounds of them);
                           // set by the host for launches of a few epochs at N <= 1024 (crn_api.cpp: run_device_impl)
  float wire_unscale;      // wire-format launches: 1 / full scale (2^-15 by default) for a sum of magnitudes, its square for energies
  // outputs (device, nullable)
  float *features;
  double *ann_out;
  int32_t *decision;
  uint8_t *occupancy;
  float *spectrum;
  // CA-CFAR (crn_sense_set_cfar): read only by the kCfar kernels, which launch_sense picks when cfar_on != 0
  int cfar_on;
  int cfar_guard;          // g: guard cells on each side
  int cfar_train;          // W: training cells on each side (1..64)
  int cfar_min_bins;       // a band is occupied when at least this many of its bins are detected
  float cfar_scale;        // bin k is detected when sum_K P[k] > cfar_scale * (the method's statistic of the K-frame training sums):
                           // CA alpha / (2 W) on both sides' total, GO / SO alpha / W on the larger / smaller side, OS alpha on each cell
  uint32_t *cfar_mask;     // [n_epochs][N / 32] or null: bit k % 32 of word k / 32 = bin k detected
  int32_t *cfar_band_bins; // [n_epochs][n_bands] or null: detected bins per band (segment listings counted as the band sums count them)
  int cfar_method;         // crn_cfar_method (crn_sense_set_cfar_ex)
  int cfar_rank;           // OS: detected when at least this many training cells c have fl32(cfar_scale c) < sum_K P[k]
  // The band plan once more for the kTw1C kernels, whose register rows start kTw1cRowShift bins early (bin_of above): read by them in
  // place of n_row_entries, band_tab's row entries and acc_mask — which stay what every other kernel reads.
  const int *row_entries_shift;  // [kRowEntryWords] device; band_tab's row-entry packing, rows cut at ((k + 7) mod N) >> 8, lo / hi from 256 d - 7
  int n_row_entries_shift;       // > 0: the plan fits those slots (register close of the kTw1C kernels)
  unsigned acc_mask_shift;       // acc_mask for those rows (N = 4096: bit d = bins [256 d - 7, 256 d + 249) mod N hold a band bin)
};

struct SynthParams {
  float2 *iq;
  long long n_epochs;
  long long samples_per_epoch;
  unsigned long long seed;
  float noise_sigma;  // per component
  float tone_amp;     // per tone
  int tones;
  int fft_len;
  int n_active;       // pick uniformly in 0..n_active (0 = idle)
  int active_band0;   // first band index that can be picked
  const int *band_bins_begin;  // [n_bands + 1]
  const int *band_bins;        // flattened bin lists per band
  const int *band_c2;          // [n_bands] twice the band's signed centre bin (modulated carriers)
  int32_t *truth;              // [n_epochs] or null
  int pu_model;                // crn_pu_model; the Markov models read truth[] (filled by launch_pu_pattern)
  int signal_kind;             // crn_signal_kind
  float signal_rms;
  long long epochs_per_stream; // Markov models
  float adc_scale;             // 0: off; 2^(adc_bits - 1): components rounded to multiples of 1 / adc_scale, clipped to [-1, 1)
};

// *deal_rounds_run (when asked for) = the form that was really launched: p.deal_rounds when the dealt-frame kernel took it, 0 when the
// streaming kernel did — also when the device refused the dealt form's LDS and the launch fell back (crn_sense_dealt_launches counts from this)
hipError_t launch_sense(const SenseParams &p, int fft_len, bool mag, bool win, int variant,
                        hipStream_t stream, bool sc16 = false, int *deal_rounds_run = nullptr);
struct FftParams {
  const float2 *in;        // [n_frames] frames of L samples, frame_stride samples apart
  float2 *out;             // [n_frames][N]
  long long n_frames;
  long long frame_stride;
  int L;                   // samples taken per frame (zero-padded to N)
  const float2 *tw1;       // [17][T]
  const float2 *tw2;       // [16][R3]
};
hipError_t launch_fft(const FftParams &p, int fft_len, hipStream_t stream);
struct MonitorParams {
  const float *spectrum;   // [n_rows][n] the sensing kernel's per-bin output (mean |X|^2 over the row's frames)
  long long n_rows;
  int n;                   // fft_len (power of two)
  float alpha;             // IIR weight of the new row
  float scale;             // 1 / normalisation of |X|^2
  int db_domain;           // 1: average the dB values (gr-qtgui); 0: average linear power
  int first;               // 1: the state is seeded with row 0
  float *state;            // [n] IIR state per displayed column, in / out
  float *waterfall_db;     // [n_rows][n] or null
  float *average_db;       // [n_rows][n] or null
};
hipError_t launch_monitor(const MonitorParams &p, hipStream_t stream);
// noise-floor estimate: scratch holds kNoiseFloorMaxEpochs per-epoch medians + the result
constexpr int kNoiseFloorMaxEpochs = 4096;
hipError_t launch_noise_floor(const float *feat, int n_epochs, int nb, float *scratch, hipStream_t stream);
hipError_t launch_synth(const SynthParams &p, hipStream_t stream);
hipError_t launch_pack_sc16(const float *iq, long long n_samples, short *out, float full_scale, hipStream_t stream);   // crn_kernels_sc16.hip (make SC16=1)
hipError_t launch_pu_pattern(const SynthParams &p, hipStream_t stream);
hipError_t launch_nop(hipStream_t stream);   // one empty workgroup (crn_sense_warm_stream)

}  // namespace crn
#endif
