/*
 * crn_sense.h — C ABI of libcrnsense: the MI355X (gfx950) spectrum-sensing hot path.
 *
 * This is the drop-in boundary for the FFT + energy-detect + decision loop that the
 * reference engine runs on every USRP rx buffer
 *   (reference: cognitive_engines/CE_Predictive_Node/CE_Predictive_Node.cpp:146-289).
 * The reference has no FFI of its own: the path is C++ calling liquid-dsp's C API
 *   fft_create_plan / fft_execute        (CE_Predictive_Node.cpp:42-45, :150)
 * followed by inline loops.  Every entry point below names the reference lines it replaces.
 *
 * Conventions
 *   - plain C, no C++/torch types; all pointers are raw host or device addresses.
 *   - every function returns 0 on success or a negative crn_status; crn_last_error()
 *     returns a thread-local human readable message (the reference itself has no error
 *     convention: void returns, printf + exit — src/crts.cpp:111-115).
 *   - IQ samples are interleaved complex fp32 (re, im), 8 bytes per sample — the layout of
 *     ExtensibleCognitiveRadio::ce_usrp_rx_buffer (include/extensible_cognitive_radio.hpp:547)
 *     and of liquid_float_complex.
 *   - a "frame" is one FFT input (N samples, of which the first L <= N come from the
 *     caller and the rest are zero: CE_Predictive_Node.cpp:37,149);
 *     an "epoch" is K consecutive frames that yield one decision (fft_averaging, .hpp:32).
 *   - thread-compatible: one handle per host thread.  The one concurrency a handle is built for: an ingest ring's launcher thread
 *     launching through it while the thread that owns it changes thresholds, weights or the band plan (crn_sense_set_thresholds /
 *     _set_ann / _set_bands) — launches and those updates are serialised inside the handle, each launch sees one plan, whole.
 *   - every entry point that touches the GPU makes cfg.device current on the calling thread first
 *     (a new thread starts on device 0), so handles of several devices can be driven from any thread.
 */
#ifndef CRN_SENSE_H
#define CRN_SENSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRN_ABI_VERSION 4

#if defined(__GNUC__)
#define CRN_API __attribute__((visibility("default")))
#else
#define CRN_API
#endif

#define CRN_MAX_BANDS 80   /* features per epoch (reference: 4 = NF, CH1, CH2, CH3)     */
#define CRN_MAX_SEGS 160   /* contiguous bin ranges (reference: 5, CH1 wraps around DC) */
#define CRN_ANN_IN 4       /* INPUTS          CE_Predictive_Node.hpp:20 */
#define CRN_ANN_HID 5      /* HIDDEN_NEURONS  CE_Predictive_Node.hpp:21 */
#define CRN_ANN_OUT 3      /* OUTPUT_NEURONS  CE_Predictive_Node.hpp:22 */

typedef enum crn_status {
  CRN_OK = 0,
  CRN_ERR_ARG = -1,      /* bad argument / unsupported configuration   */
  CRN_ERR_DEVICE = -2,   /* HIP runtime error (message has the detail) */
  CRN_ERR_NOMEM = -3,
  CRN_ERR_STATE = -4,    /* call sequence error                        */
  CRN_ERR_BUSY = -5      /* ingest ring: both batch buffers are on the GPU; the packet was NOT taken */
} crn_status;

/* How per-bin values are accumulated over the K frames of an epoch and turned into features. */
typedef enum crn_mode {
  /* Reference-exact: a[k] += |X[k]| / K per frame (CE_Predictive_Node.cpp:152-154);
   * M_b = sum_{k in band b} a[k] (:173-191); feature_b = M_b * M_b (:194-197). */
  CRN_MODE_REF_MAG = 0,
  /* Energy detector (BASELINE.json configs[1..4]): P[k] = (sum_f |X_f[k]|^2) / K;
   * feature_b = sum_{k in band b} P[k]. */
  CRN_MODE_ENERGY = 1
} crn_mode;

/* How features become the occupied/idle decision. */
typedef enum crn_decide {
  /* 4-5-3 sigmoid net in double + first-output->=0.8 cascade (CE_Predictive_Node.cpp:214-261).
   * Requires n_bands == 4 with band order {NF, CH1, CH2, CH3} (.cpp:200). */
  CRN_DECIDE_ANN = 0,
  /* occupancy[b] = feature_b > thresh[b] * (ref_band >= 0 ? feature_ref : 1), fp32. */
  CRN_DECIDE_THRESHOLD = 1,
  CRN_DECIDE_NONE = 2
} crn_decide;

typedef enum crn_window {
  CRN_WINDOW_RECT = 0,   /* the reference applies no window (CE_Predictive_Node.cpp:149-150) */
  CRN_WINDOW_HANN = 1,   /* periodic Hann, w[n] = 0.5 - 0.5 cos(2 pi n / N) (Welch mode)     */
  /* 4-term Blackman-Harris over N-1, a = {0.35875, 0.48829, 0.14128, 0.01168}: the window of the
   * reference's GNU Radio monitor (spectrum_analyzer.py:262-275, firdes.WIN_BLACKMAN_hARRIS). */
  CRN_WINDOW_BLACKMAN_HARRIS = 2
} crn_window;

/* Bins [lo, hi) of the N-point spectrum contribute to feature `band`. */
typedef struct crn_band_seg {
  int32_t lo;
  int32_t hi;
  int32_t band;
} crn_band_seg;

/* Everything the reference hard-codes as `static constexpr` members
 * (CE_Predictive_Node.hpp:30-33,42-43,55-57) or literals (.cpp:78-120,173-191,245-261). */
typedef struct crn_cfg {
  int32_t abi_version;        /* must be CRN_ABI_VERSION                                   */
  int32_t fft_len;            /* N in {512, 1024, 2048, 4096}; reference: 512 (.hpp:31)    */
  int32_t frames_per_epoch;   /* K >= 1; reference: 10 (.hpp:32)                           */
  int32_t hop;                /* samples between frame starts. hop == fft_len: disjoint
                                 frames (reference). hop == fft_len/2: Welch, 50 % overlap */
  int32_t mode;               /* crn_mode                                                  */
  int32_t decide;             /* crn_decide                                                */
  int32_t window;             /* crn_window                                                */
  int32_t n_bands;            /* 1..CRN_MAX_BANDS                                          */
  int32_t n_segs;             /* 1..CRN_MAX_SEGS                                           */
  int32_t ref_band;           /* THRESHOLD: band whose feature scales the thresholds, or -1 */
  int32_t device;             /* HIP device ordinal                                        */
  int32_t reserved0;
  crn_band_seg segs[CRN_MAX_SEGS];
  float thresh[CRN_MAX_BANDS];
  /* ANN weights, reference indexing: w_ih[i][j], i = 0 bias, 1..4 inputs {NF,CH1,CH2,CH3},
   * j = 1..5 hidden (column 0 unused); w_ho[j][k], j = 0 bias, 1..5 hidden, k = 1..3 outputs
   * (CE_Predictive_Node.hpp:66,71; values .cpp:78-120). */
  double ann_w_ih[CRN_ANN_IN + 1][CRN_ANN_HID + 1];
  double ann_w_ho[CRN_ANN_HID + 1][CRN_ANN_OUT + 1];
  double ann_threshold;       /* 0.8 (.cpp:245,250,255)                                    */
  /* Transmit frequency the engine tunes to for decision d = 0 (none), 1, 2, 3
   * (.cpp:247,252,257: CH1 busy -> CHANNEL2, CH2 busy -> CHANNEL1, CH3 busy -> CHANNEL2;
   * entry 0 is unused: "ALL BUSY" makes no call, .cpp:260-261). */
  double tx_freq_for_decision[4];
} crn_cfg;

typedef struct crn_handle crn_handle;

/* Per-epoch results.  Any pointer may be NULL (that output is skipped).  For the *_device
 * entry point these are device addresses, for the *_host entry point host addresses. */
typedef struct crn_out {
  float *features;      /* [n_epochs][n_bands] fp32. REF_MAG order {NF,CH1,CH2,CH3}: the
                           Features_Buffer[1..4] of CE_Predictive_Node.cpp:200               */
  double *ann_out;      /* [n_epochs][3] Output[1..3] (.cpp:229-235); DECIDE_ANN only        */
  int32_t *decision;    /* [n_epochs] DECIDE_ANN: 0 = "ALL BUSY" (no output >= 0.8), 1/2/3 =
                           Channel_State[d] OCCUPIED (.cpp:245-261). DECIDE_THRESHOLD: number
                           of occupied bands.                                               */
  uint8_t *occupancy;   /* [n_epochs][n_bands] 1 = occupied. DECIDE_ANN: one-hot over
                           bands 1..3 from `decision`; band 0 (NF) always 0.                */
  float *spectrum;      /* [n_epochs][fft_len] the K-frame average per bin: fft_avg[] of
                           CE_Predictive_Node.hpp:51 (REF_MAG) or P[k] (ENERGY).             */
} crn_out;

/* -- configuration helpers ------------------------------------------------------------ */

/* The reference engine's own parameters: N=512, K=10, rectangular, REF_MAG, the five bin
 * ranges of CE_Predictive_Node.cpp:173-191 (bin 511 is NOT part of CH1), DECIDE_ANN with the
 * weights of .cpp:78-120, threshold 0.8, tx map 835e6/833e6/835e6 (.hpp:55-57, .cpp:245-258). */
CRN_API int crn_cfg_reference(crn_cfg *cfg);

/* The reference engine's estimator at another FFT size: crn_cfg_reference with fft_len N (multiple of 512) and the five bin
 * ranges scaled by N/512 (the same frequency spans at fs = 13 MHz); REF_MAG + DECIDE_ANN.  The weights stay the reference's,
 * which were fitted at N = 512 and one receiver gain (features grow with N^2): fit others with crn_ann_train_device and put
 * them in with crn_cfg_load_ann / crn_sense_set_ann. */
CRN_API int crn_cfg_reference_scaled(crn_cfg *cfg, int32_t fft_len);

/* The 4-5-3 network's weights as a text file — what crn_ann_train_device produces, for an engine's `-w <file>` (ce_args:
 * src/crts.cpp:43-81): '#' comments, then WeightIH[5][6] and WeightHO[6][4] in the reference's array order
 * (CE_Predictive_Node.hpp:66,71; .cpp:78-120), then optionally the decision threshold.  Doubles are written with 17 digits
 * (exact round trip).  load leaves everything else in cfg untouched. */
CRN_API int crn_cfg_save_ann(const crn_cfg *cfg, const char *path);
CRN_API int crn_cfg_load_ann(crn_cfg *cfg, const char *path);

/* Build-side generalisation used by BASELINE.json configs[1] and the headline metric:
 * fft_len N (multiple of 512), K=10, rectangular, ENERGY, the reference's bin ranges scaled by
 * N/512 (same frequency spans at fs = 13 MHz), DECIDE_THRESHOLD relative to the noise-floor band
 * with thresh[b] = lambda * bins_b / bins_NF. */
CRN_API int crn_cfg_energy_scaled(crn_cfg *cfg, int32_t fft_len, float lambda);

/* Welch PSD configuration of BASELINE.json configs[2]: N-point Hann, hop N/2, n_bands equal
 * contiguous bands covering all N bins, absolute thresholds (ref_band = -1) to be filled in by
 * the caller in cfg->thresh. */
CRN_API int crn_cfg_welch(crn_cfg *cfg, int32_t fft_len, int32_t frames_per_epoch, int32_t n_bands);

/* crn_cfg_energy_scaled's channel plan and relative thresholds on a Welch estimate: periodic Hann, hop N/2, K frames. */
CRN_API int crn_cfg_welch_scaled(crn_cfg *cfg, int32_t fft_len, int32_t frames_per_epoch, float lambda);

/* -- lifecycle --------------------------------------------------------------------------- */

/* Replaces the constructor's buffer zeroing + fft_create_plan (CE_Predictive_Node.cpp:36-45):
 * validates cfg, selects cfg->device, builds twiddle/window/band tables in HBM. */
CRN_API int crn_sense_create(const crn_cfg *cfg, crn_handle **out);

/* The reference never destroys its plan (empty destructor, CE_Predictive_Node.cpp:49; no
 * `delete CE` in the ECR); a GPU-backed engine needs an explicit release. */
/* CRN_ERR_STATE while an ingest ring is attached (its launcher thread launches through the handle): crn_ingest_destroy first. */
CRN_API int crn_sense_destroy(crn_handle *h);

/* -- the hot path --------------------------------------------------------------------------
 * Replaces, for n_epochs * K frames in one launch, CE_Predictive_Node.cpp:148-261:
 *   memcpy into the zero-padded FFT buffer (:149), fft_execute (:150), magnitude + /K running
 *   mean (:152-154), band sums + squares (:173-197), feature widening (:200), ANN (:214-235),
 *   decision cascade (:245-261) and the fft_avg reset (:287-288).
 *
 * d_iq: device pointer, interleaved complex fp32.  Epoch e starts at sample
 *       e * epoch_stride; its frame f covers samples [f*hop, f*hop + samples_per_frame) of the
 *       epoch, zero-padded to fft_len.  samples_per_frame (L) must be in 1..fft_len — the
 *       reference does not check (:149) and overruns its buffer when L > 512; this ABI rejects
 *       it.  With hop < fft_len, samples_per_frame must equal fft_len.
 *       epoch_stride <= 0 selects the dense default K * samples_per_frame (hop == fft_len)
 *       or K * hop (overlapped: consecutive epochs share fft_len - hop samples, so the
 *       buffer must hold n_epochs * K * hop + (fft_len - hop) samples).
 * stream: a hipStream_t (NULL = default stream).  The call only enqueues work.
 */
CRN_API int crn_sense_run_device(crn_handle *h, const float *d_iq, int64_t n_epochs,
                         int32_t samples_per_frame, int64_t epoch_stride,
                         const crn_out *d_out, void *stream);

/* Host-buffer convenience used by the engine wrapper: H2D, run, D2H, synchronise. */
CRN_API int crn_sense_run_host(crn_handle *h, const float *iq, int64_t n_epochs,
                       int32_t samples_per_frame, int64_t epoch_stride, const crn_out *out);

/* -- per-bin CA-CFAR detection (cell averaging, constant false-alarm rate) --------------------------------------------------
 * A handle created with mode CRN_MODE_ENERGY and decide CRN_DECIDE_THRESHOLD or CRN_DECIDE_NONE can decide per bin instead of per
 * fixed band.  With P[k] the K-frame mean energy of bin k (the `spectrum` output), guard cells g and training cells W on each side:
 *   Z[k] = (1 / 2W) sum P[(k + i) mod N] over g < |i| <= g + W   (circular: bin N-1 neighbours bin 0)
 *   bin k detected  <=>  P[k] > alpha * Z[k]   (fp32)
 *   band_bins[b] = detected bins in band b's segments (a bin counts once per segment listing, as the band sums count it)
 *   occupancy[b] = band_bins[b] >= min_bins,  decision = number of occupied bands
 * `features` stay the band energy sums and `spectrum` the per-bin means; the stored thresholds are kept but not used while CFAR is on.
 * The threshold follows the local noise floor (filter roll-off, a DC spike), so no calibration is needed.
 * Parameters: 1 <= train <= 64, guard >= 0, 2 (guard + train) + 1 <= fft_len, alpha > 0 and finite, min_bins >= 1, reserved = 0.
 * Suggested (not applied automatically): guard 2, train 16, alpha from crn_cfar_alpha(1e-3, frames_per_epoch, 16, &alpha),
 * min_bins 1.  All windows, hop == fft_len or fft_len / 2, and every fft_len are supported. */
typedef struct crn_cfar_params {
  int32_t guard, train, min_bins, reserved;
  float alpha;
} crn_cfar_params;

/* Switch CFAR on with `params`, or back to the cfg's own rule with NULL; launches enqueued after the call use the new values.
 * CRN_ERR_ARG on a REF_MAG handle or for parameters out of range; CRN_ERR_STATE on an ANN handle or while an ingest ring is attached.
 * Not supported yet (CRN_ERR_ARG): an ingest ring on a CFAR handle (crn_epoch_result has no room for the mask) and wire-format (sc16)
 * launches. */
CRN_API int crn_sense_set_cfar(crn_handle *h, const crn_cfar_params *params);
/* The parameters in force and whether CFAR is on (*on = 0: params holds the last ones set, zeros if none).  Either pointer may be NULL. */
CRN_API int crn_sense_get_cfar(crn_handle *h, crn_cfar_params *params, int32_t *on);
/* crn_sense_run_device with the CFAR outputs (device pointers, either may be NULL):
 *   d_bin_mask   [n_epochs][fft_len / 32] bit k % 32 of word k / 32 = bin k detected
 *   d_band_bins  [n_epochs][n_bands]      detected bins per band
 * CRN_ERR_STATE when CFAR is off.  (crn_sense_run_device on a CFAR handle gives the CFAR occupancy and decision without these two.) */
CRN_API int crn_sense_run_device_cfar(crn_handle *h, const float *d_iq, int64_t n_epochs, int32_t samples_per_frame, int64_t epoch_stride,
                                      const crn_out *d_out, uint32_t *d_bin_mask, int32_t *d_band_bins, void *stream);
/* alpha for a false-alarm probability `pfa` per bin (0 < pfa < 1), frames_per_epoch K >= 1 and train W (1..64), host only.
 * Assumes white complex Gaussian noise, the rectangular window and disjoint frames: P[k] / Z[k] then follows F(2K, 4WK), and
 * pfa = P(F > alpha) is inverted by bisection on the regularised incomplete beta function (K = 1: pfa = (1 + alpha / 2W)^(-2W)).
 * Windowed or overlapped frames correlate neighbouring bins and frames: the real false-alarm rate then differs from `pfa`. */
CRN_API int crn_cfar_alpha(double pfa, int32_t frames_per_epoch, int32_t train, double *alpha);

/* -- the CFAR detector family: greatest-of, smallest-of and ordered-statistic ------------------------------------------------
 * The same P[k], guard and training cells, circular wrap, min_bins, band_bins, occupancy and decision as above; only the noise
 * estimate Z[k] changes.  With L[k] and R[k] the means of the W training cells on each side:
 *   CRN_CFAR_CA  Z = (L + R) / 2            (crn_sense_set_cfar)
 *   CRN_CFAR_GO  Z = max(L, R)              holds the false-alarm rate where the floor steps (a band edge, filter roll-off)
 *   CRN_CFAR_SO  Z = min(L, R)              resolves closely spaced carriers
 *   CRN_CFAR_OS  Z = the rank-th smallest of the 2W cells, 1 <= rank <= 2W: ignores up to 2W - rank interferers in the window
 * bin k detected  <=>  P[k] > alpha * Z[k].  OS is decided exactly by counting: at least `rank` training cells c with
 * fl32(alpha c) < P[k] (both on the K-frame sums), which is P[k] > fl32(alpha X_(rank)), ties included. */
typedef enum crn_cfar_method { CRN_CFAR_CA = 0, CRN_CFAR_GO = 1, CRN_CFAR_SO = 2, CRN_CFAR_OS = 3 } crn_cfar_method;

/* crn_cfar_params plus the method and, for CRN_CFAR_OS only, the rank (0 for the other methods); reserved = 0. */
typedef struct crn_cfar_params_ex {
  int32_t method, guard, train, min_bins, rank, reserved;
  float alpha;
} crn_cfar_params_ex;

/* crn_sense_set_cfar for every method: the same handle checks and parameter ranges, and CRN_ERR_ARG for a method outside 0..3, an OS
 * rank outside 1..2 train, or a nonzero rank with another method.  NULL switches CFAR off.  A refused call leaves the detector as it
 * was.  crn_sense_set_cfar(h, p) is this call with CRN_CFAR_CA and rank 0.  Ring and sc16 refusals apply to every method. */
CRN_API int crn_sense_set_cfar_ex(crn_handle *h, const crn_cfar_params_ex *params);
/* The detector in force, method and rank included, and whether CFAR is on.  Either pointer may be NULL.  (crn_sense_get_cfar fills
 * the fields the two structs share, whichever method was set.) */
CRN_API int crn_sense_get_cfar_ex(crn_handle *h, crn_cfar_params_ex *params, int32_t *on);
/* alpha for a per-bin false-alarm probability `pfa` of `method`, host only, under crn_cfar_alpha's noise model (training cells and
 * P are i.i.d. Gamma(K) in units of the noise power).  rank: 1..2 train for CRN_CFAR_OS, 0 otherwise.
 *   CA  crn_cfar_alpha, exactly
 *   GO  pfa = int Q(K, alpha s / W) 2 F(s) f(s) ds         f, F: the Gamma(WK) density and distribution (one side's sum)
 *   SO  pfa = int Q(K, alpha s / W) 2 (1 - F(s)) f(s) ds
 *   OS  pfa = int_0^1 Beta(u; rank, 2W - rank + 1) Q(K, alpha F_K^-1(u)) du
 * Q(K, .) is the regularised upper incomplete gamma function.  Each is evaluated by quadrature and inverted by bisection in double.
 * CRN_ERR_ARG for arguments out of range and for a pfa too small to reach. */
CRN_API int crn_cfar_alpha_ex(int32_t method, double pfa, int32_t frames_per_epoch, int32_t train, int32_t rank, double *alpha);

/* -- emitter segments from the CFAR bin mask ---------------------------------------------------------------------------------
 * The detector's back end: per epoch, the bit mask d[k] and the `spectrum` row P[k] (k in Z_N, circular like CFAR's training cells)
 * become a short ordered list of segments and a noise estimate, on the device, for the whole batch in one launch.
 *   1. closing   no bit set: no segments.  Otherwise every maximal circular run of zero bits of length <= merge_gap joins the closed
 *                mask c (merge_gap = 0: c = d).
 *   2. segments  the maximal circular runs of ones in c: bins (lo + i) mod N, 0 <= i < width; a segment may cross the wrap
 *                (lo + width > N).  c all ones: one segment, lo = 0, width = N.
 *   3. noise     before any filtering: noise_bins = bins with c = 0, noise_mean = the mean of P over them (0 when there are none).
 *   4. filter    segments with width < min_width are dropped; n_found counts the rest; the first min(n_found, max_segments) by
 *                ascending lo are stored (n_stored), so a wrap-crossing segment comes last.  Slots beyond n_stored are zero-filled:
 *                a batch gives the same bytes however it is cut into launches.
 *   5. stored    n_detected = set bits of d inside the segment; peak_bin = the absolute bin of the largest P (ties: the smallest i),
 *                peak_power = that P; power = sum P; centroid = sum(i P) / sum(P), the power-weighted offset from lo in bins
 *                (0 when the sum is 0).  Sums are accumulated in fp64 and rounded to fp32 once. */
typedef struct crn_segment_params {
  int32_t merge_gap, min_width, max_segments, reserved;
} crn_segment_params;
typedef struct crn_segment {
  int32_t lo, width, peak_bin, n_detected;
  float power, peak_power, centroid, reserved;
} crn_segment; /* 32 bytes */
typedef struct crn_segment_epoch {
  int32_t n_found, n_stored, noise_bins;
  float noise_mean;
} crn_segment_epoch; /* 16 bytes */

/* Enqueue the extraction on `stream` over n_epochs rows (device pointers):
 *   d_bin_mask  [n_epochs][fft_len / 32]   as crn_sense_run_device_cfar writes it (8-byte aligned)
 *   d_spectrum  [n_epochs][fft_len]        the `spectrum` output of the same launch (16-byte aligned)
 *   d_epochs    [n_epochs]                 one header per epoch
 *   d_segments  [n_epochs][max_segments]   or NULL: headers only (the count and the noise estimate)
 * `h` supplies fft_len and the device, nothing else: the mask and rows may come from any source, the handle may be of any mode, with
 * CFAR on or off.  Allocates nothing, keeps no state.  CRN_ERR_ARG for a NULL h, params, d_bin_mask, d_spectrum or d_epochs,
 * merge_gap outside 0 .. fft_len - 1, min_width < 1, max_segments outside 1 .. 256, reserved != 0, n_epochs < 0 or a misaligned
 * pointer.  n_epochs = 0 succeeds and launches nothing. */
CRN_API int crn_segments_device(crn_handle *h, const uint32_t *d_bin_mask, const float *d_spectrum, int64_t n_epochs,
                                const crn_segment_params *params, crn_segment_epoch *d_epochs, crn_segment *d_segments, void *stream);

/* -- tracks: emitter segments linked across epochs ----------------------------------------------------------------------------
 * One record per track, a transmitter's stay in one place of the band, from the two arrays crn_segments_device wrote.  A batch is
 * n_epochs / epochs_per_stream streams of epochs_per_stream consecutive epochs in time order (crn_synth_cfg.n_streams); N = fft_len.
 * Not a sequential tracker: tracks are the connected components of a graph, which every epoch can work on at once.
 *   1. nodes    the stored segments: node (e, s), s < d_epochs[e].n_stored (segments beyond max_segments were never stored and are
 *               not seen).  Epoch e belongs to stream e / epochs_per_stream; t = e % epochs_per_stream is its time in the stream.
 *   2. links    nodes (e, a) and (e + d, b) of the same stream, 1 <= d <= max_miss + 1, are linked when
 *                 ((lo_b - lo_a) mod N) < width_a + slack_bins  or  ((lo_a - lo_b) mod N) < width_b + slack_bins,
 *               that is when, on the circle, the two bin intervals share a bin or the gap between them is smaller than slack_bins
 *               (0: they must share a bin; 1: touching is enough).  Integers only; a wrap-crossing segment and a segment of width N
 *               are no special cases.  Nodes of one epoch are never linked directly.
 *   3. tracks   the connected components.  A component's root is its smallest node index e * max_segments + s: its earliest epoch,
 *               there the lowest slot.  Two emitters that touch in some epoch (both linked to one segment of a neighbouring epoch)
 *               are ONE track; a caller who wants them apart lowers slack_bins here or merge_gap in the extraction.
 *   4. filter   n_epochs_hit = the number of distinct epochs with a member.  Components with n_epochs_hit < min_epochs are dropped
 *               (an M-of-N confirmation: min_epochs = 2 removes single-epoch false alarms).  Per stream n_found counts the rest; they
 *               are numbered 0, 1, ... by ascending root; the first min(n_found, max_tracks) are stored, the other slots zero-filled.
 *   5. stored   first_t, last_t: the first and last time with a member; first_slot, last_slot: the lowest slot among the members in
 *               that epoch (the two segments to look up for a drift); n_segments: members; each member m is placed at
 *               off_m = ((lo_m - lo_root + N / 2) mod N) - N / 2 and covers off_m .. off_m + width_m - 1: lo_off and hi_off are the
 *               smallest and largest offset covered; width_sum = sum of width_m (the mean width is width_sum / n_segments);
 *               power_sum = sum of P_m, the members' power; peak_power = the largest of the members' peak_power (exact);
 *               centre = (lo_root + sum(P_m (off_m + centroid_m)) / sum(P_m)) mod N, in bins (lo_root when the sum is 0; a value
 *               that rounds to N is stored as 0); both sums in fp64, rounded to fp32 once.  flags: bit 0 when first_t <= max_miss
 *               (the track may have begun before the batch), bit 1 when last_t >= epochs_per_stream - 1 - max_miss (it may go on
 *               after it).  Nothing is carried from one call to the next.
 *   6. labels   d_track_of[e][s] = the number of node (e, s)'s track within its stream (numbers >= max_tracks occur when the list was
 *               truncated), -1 for empty slots and for members of dropped components. */
typedef struct crn_track_params {
  int32_t max_segments, epochs_per_stream, slack_bins, max_miss, min_epochs, max_tracks, reserved[2];
} crn_track_params; /* 32 bytes */
typedef struct crn_track {
  int32_t first_t, last_t, first_slot, last_slot, n_epochs_hit, n_segments, lo_off, hi_off;
  int64_t width_sum;
  float power_sum, peak_power, centre;
  int32_t flags, reserved[2];
} crn_track; /* 64 bytes */
typedef struct crn_track_stream {
  int32_t n_found, n_stored, n_nodes, reserved; /* n_nodes: the stored segments of the stream */
} crn_track_stream; /* 16 bytes */

/* Bytes of device scratch crn_tracks_device needs for n_epochs epochs under `params` (of slack_bins only the sign is checked): needs no handle
 * and no device.  Positive for valid arguments (also for n_epochs = 0), -1 for a NULL params, n_epochs < 0 or a parameter outside
 * the ranges below, or when n_epochs x max_segments does not fit 31 bits. */
CRN_API int64_t crn_tracks_workspace_bytes(int64_t n_epochs, const crn_track_params *params);

/* Enqueue the linking on `stream` (device pointers):
 *   d_epochs     [n_epochs]                             as crn_segments_device wrote them (16-byte aligned)
 *   d_segments   [n_epochs][max_segments]               the same call's segments, the same max_segments (16-byte aligned)
 *   d_streams    [n_epochs / epochs_per_stream]         one header per stream (16-byte aligned)
 *   d_tracks     [n_epochs / epochs_per_stream][max_tracks]   (16-byte aligned)
 *   d_track_of   [n_epochs][max_segments] int32, or NULL
 *   d_workspace  workspace_bytes >= crn_tracks_workspace_bytes of scratch (8-byte aligned); its contents before and after mean nothing
 * `h` supplies fft_len and the device, nothing else.  Only enqueues (seven small launches), allocates nothing, keeps no state; integer
 * fields, flags, peak_power and the labels do not depend on the order the work ran in; power_sum and centre are summed with fp64
 * atomic adds and may differ in the last bit between runs.  CRN_ERR_ARG, decided before any device call, for a NULL h, params,
 * d_epochs, d_segments, d_streams, d_tracks or d_workspace; n_epochs < 0; max_segments outside 1 .. 256; epochs_per_stream < 1 or not
 * dividing n_epochs; slack_bins outside 0 .. fft_len - 1; max_miss outside 0 .. 15; min_epochs < 1; max_tracks outside 1 .. 1024;
 * reserved != 0; n_epochs x max_segments >= 2^31; a misaligned pointer; a workspace too small.  n_epochs = 0 succeeds and launches
 * nothing. */
CRN_API int crn_tracks_device(crn_handle *h, const crn_segment_epoch *d_epochs, const crn_segment *d_segments, int64_t n_epochs,
                              const crn_track_params *params, crn_track_stream *d_streams, crn_track *d_tracks, int32_t *d_track_of,
                              void *d_workspace, int64_t workspace_bytes, void *stream);

/* -- tracks carried across batches ---------------------------------------------------------------------------------------------
 * crn_tracks_device knows one batch.  Here a sequence of calls covers, for every stream of the batch, the times
 * t_start .. t_start + epochs_per_stream - 1: global epoch counts per stream since the call with t_start = 0.  T = t_start +
 * epochs_per_stream, H = max_miss + 1, N = fft_len.
 * What the caller sees.  Take the link graph of crn_tracks_device (its steps 1-2) over all epochs 0 .. T - 1 of the stream.  After a call
 * a component is OPEN when last_t >= T - 1 - max_miss and flush == 0, otherwise CLOSED.  Every component is reported exactly once, by
 * the call in which it becomes closed, with the fields crn_tracks_device would give for the whole stream in one batch of T epochs
 * (global first_t / last_t; flag bit 0 when first_t <= max_miss; bit 1 when last_t >= T - 1 - max_miss, which only a record closed by
 * `flush` can have), apart from the two exceptions below.  Within a call the closed components with n_epochs_hit >= min_epochs are
 * numbered by ascending root (first_t, first_slot); the first max_tracks are stored, the other slots zero-filled; n_found counts all.
 * The carry is opaque device memory written by the call, per stream: T; the TAIL, the stored (lo, width) lists of the epochs
 * T - H .. T - 1 (fewer before H epochs were seen), each segment with the position of the open track it belongs to; and the OPEN
 * TRACKS in ascending root order, each with its root (t, slot), lo_root, last (t, slot), hits, n_segments, lo_off, hi_off, width_sum,
 * power and moment in fp64, peak and a `merged` bit.  Every tail segment belongs to an open track and every open track has a tail
 * segment, so at most H x max_segments tracks are open per stream: the carry is sized for that and nothing overflows.
 * One call (the incremental rule):
 *   1. nodes    the open tracks (in carry order), then the tail segments, then the new stored segments by (t, slot).
 *   2. joins    each tail segment is joined to its open track.
 *   3. links    step 2's condition of crn_tracks_device between any tail or new segment and any NEW segment 1 .. H epochs later.
 *   4. tracks   the connected components; the root is the smallest node in the order of item 1, so a component holding carried tracks
 *               keeps the earliest carried root.
 *   5. fresh    a component without a carried track accumulates as in crn_tracks_device.
 *   6. carried  a component rooted at carried track A starts from A's accumulators.  Every further carried track B adds itself re-based
 *               by delta = ((lo_root_B - lo_root_A + N / 2) mod N) - N / 2: lo_off_B + delta and hi_off_B + delta enter the min / max,
 *               moment_B + delta power_B is added, counts and sums add, peak and last (t, lowest slot) take the maximum.
 *   7. new      new segments add with `off` relative to lo_root_A; tail segments add nothing (they are already counted).
 *   8. hits     distinct NEW epochs with a member add to the hits.
 *   9. merged   when two or more carried tracks end in one component the epochs they shared cannot be known: the merged bit is set and
 *               stays set, hits becomes min(sum, last_t - first_t + 1), and the record carries flag bit 2 (n_epochs_hit is an upper
 *               bound).
 *  10. split    open tracks go to the new carry in ascending root order, the new tail is written, closed components are emitted.
 * The two exceptions to whole-batch equality: (a) records with bit 2: n_epochs_hit lies between the true count and the span, and
 * min_epochs is applied to the bound; every other field is the whole-batch value.  (b) Re-basing by delta is exact only while a track
 * covers less than N / 2 bins (hi_off - lo_off < N / 2); wider tracks get the values the rule gives, and the rule is the definition. */
typedef struct crn_track_carry_stream {
  int32_t n_found, n_stored, n_nodes;              /* closed by this call; stored segments of this call's epochs */
  int32_t n_open, n_open_found, n_open_stored;     /* carried on; of those hits >= min_epochs; written to d_open */
  int32_t status, reserved;                        /* bit 0: the carry did not match and was taken as empty */
} crn_track_carry_stream; /* 32 bytes */
#define CRN_TRACK_BEGAN_BEFORE 1     /* crn_track.flags */
#define CRN_TRACK_GOES_ON 2
#define CRN_TRACK_HITS_UPPER_BOUND 4 /* crn_tracks_carry_device only */

/* Bytes of the carry for n_streams streams under `params` (max_segments and max_miss decide; the other fields are only checked): needs
 * no handle and no device.  Positive for valid arguments (also for n_streams = 0), -1 as crn_tracks_workspace_bytes (a NULL params,
 * n_streams < 0, a parameter out of range). */
CRN_API int64_t crn_tracks_carry_bytes(int64_t n_streams, const crn_track_params *params);
/* Bytes of device scratch crn_tracks_carry_device needs for n_epochs epochs under `params`; -1 as crn_tracks_workspace_bytes, or when
 * (n_epochs + 2 (max_miss + 1) n_epochs / epochs_per_stream) x max_segments does not fit 31 bits. */
CRN_API int64_t crn_tracks_carry_workspace_bytes(int64_t n_epochs, const crn_track_params *params);

/* Enqueue one call of the sequence on `stream` (device pointers; d_epochs, d_segments, d_workspace as for crn_tracks_device):
 *   d_carry     carry_bytes >= crn_tracks_carry_bytes(n_epochs / epochs_per_stream, params), 16-byte aligned: read, then rewritten
 *   d_streams   [n_streams]               one crn_track_carry_stream per stream (16-byte aligned)
 *   d_tracks    [n_streams][max_tracks]   the records this call closed (16-byte aligned)
 *   d_open      [n_streams][max_tracks]   or NULL: the open tracks as they stand after the call, flag bit 1 set; only those with
 *               hits >= min_epochs, the first max_tracks by ascending root, the rest zero-filled (n_open_stored is 0 for NULL)
 * t_start = 0 starts afresh: the carry's previous contents mean nothing and the call initialises it; no reset function is needed.  For
 * t_start > 0 each stream's carry holds a mark (max_segments, max_miss, fft_len and T); where it does not equal what the call expects
 * (T = t_start) that stream is treated as having an empty carry and `status` bit 0 is set.  Every index read from the carry is clamped:
 * a foreign buffer cannot cause an access outside the buffers.  slack_bins, min_epochs, max_tracks and epochs_per_stream may differ from
 * call to call.  flush != 0 closes everything and leaves an empty carry with T advanced.  Only enqueues (seven small launches),
 * allocates nothing, keeps no host state.  CRN_ERR_ARG, decided before any device call, for everything crn_tracks_device refuses (with
 * the node count of crn_tracks_carry_workspace_bytes), t_start < 0, t_start + epochs_per_stream > 2^31 - 1, a NULL d_carry, carry_bytes
 * or the workspace too small, a misaligned pointer (16 bytes for the record arrays and d_carry).  n_epochs = 0 succeeds and launches
 * nothing. */
CRN_API int crn_tracks_carry_device(crn_handle *h, const crn_segment_epoch *d_epochs, const crn_segment *d_segments, int64_t n_epochs,
                                    const crn_track_params *params, int64_t t_start, int32_t flush, void *d_carry, int64_t carry_bytes,
                                    crn_track_carry_stream *d_streams, crn_track *d_tracks, crn_track *d_open, void *d_workspace,
                                    int64_t workspace_bytes, void *stream);

/* -- channels: occupancy statistics over time and an idle forecast -------------------------------------------------------------
 * What a cognitive radio senses for: which channel is free, and how likely it is to stay free.  The CFAR bin mask (and, optionally, the
 * `spectrum` rows) of a batch become one small record per stream and channel: busy fraction, the 2 x 2 transition counts of the
 * two-state chain idle / busy, run statistics and idle / busy power.  The record lives in the caller's device memory and is its own
 * carry from call to call.  A batch is laid out as for crn_tracks_device: n_epochs / epochs_per_stream streams of epochs_per_stream
 * consecutive epochs in time order; N = fft_len.
 *   Per epoch and channel   n_det = set mask bits inside the span; busy = n_det >= min_bins (a min_bins larger than the width: never
 *                           busy); power = the sum of P over the span's bins, accumulated in fp64 and rounded to fp32 once (0 when
 *                           d_spectrum is NULL).  Sums are direct: no bin outside the span ever enters one.
 *   Per stream and channel  the epochs in time order, s the busy bit and p the fp32 power of each:
 *       if first: R = all zero
 *       for each epoch of the stream:
 *           if R.n_epochs > 0:
 *               a = R.state & 1
 *               R.n_trans[a][s] += 1
 *               if s != a:                          the run (a, R.run) is complete
 *                   R.n_runs[a] += 1; R.run_sum[a] += R.run; R.run_max[a] = max(R.run_max[a], R.run)
 *                   if a == 0: R.idle_hist[clamp(floor(log2(max(R.run, 1))), 0, 15)] += 1
 *                   R.run = 0
 *           R.state = s; R.run += 1; R.n_epochs += 1; R.n_busy += s; R.power[s] += (double)p
 *     The first run starts with the first observed epoch (it is left-censored) and is counted when it ends; the run in progress is in
 *     no completed count.  A record is all zero or what an earlier call wrote; nothing else is told apart from these.
 *     No index is ever read from a record, so a foreign buffer cannot cause an access outside the buffers.  The four n_trans sum to
 *     n_epochs - 1, and run_sum[0] + run_sum[1] + run = n_epochs.
 *   Cut independence        a sequence given in one call and the same sequence cut into several calls (first = 1, then 0) give
 *                           identical integer fields; d_busy and d_power are the same bytes however the batch is cut.  power[] is an
 *                           fp64 sum of the fp32 values whose order depends on the cut. */
#define CRN_MAX_CHANNELS 64
typedef struct crn_channel_span {
  int32_t lo, width;
} crn_channel_span; /* bins (lo + i) mod N, 0 <= i < width; 0 <= lo < N, 1 <= width <= N.  A span may cross the wrap (the reference's
                     * CH1 does).  Spans may overlap. */
typedef struct crn_channel_params {
  int32_t n_channels;        /* 1..64 */
  int32_t epochs_per_stream; /* >= 1, divides n_epochs */
  int32_t min_bins;          /* >= 1 */
  int32_t first;             /* != 0: the records' contents mean nothing, start afresh */
  int32_t reserved[4];       /* 0 */
  crn_channel_span span[CRN_MAX_CHANNELS];
} crn_channel_params; /* 544 bytes */
typedef struct crn_channel_stats {
  int64_t n_epochs, n_busy;
  int64_t n_trans[2][2];                     /* [previous][current], 0 idle, 1 busy */
  int64_t n_runs[2], run_sum[2], run_max[2]; /* completed runs only */
  int64_t run;                               /* length so far of the run in progress */
  int32_t state, reserved;
  double power[2];                           /* sum of the channel's power over idle / busy epochs */
  int32_t idle_hist[16];                     /* completed idle runs with floor(log2(length)) = b; bin 15 also takes everything longer */
} crn_channel_stats; /* 192 bytes */

/* Bytes of device scratch crn_channels_device needs for n_epochs epochs under `params`: needs no handle and no device.  Positive for
 * valid arguments (also for n_epochs = 0), -1 for a NULL params, n_epochs < 0, n_channels outside 1..64, epochs_per_stream < 1 or not
 * dividing n_epochs, min_bins < 1, a nonzero reserved field, or a span with lo < 0 or width < 1 or either beyond the largest fft_len. */
CRN_API int64_t crn_channels_workspace_bytes(int64_t n_epochs, const crn_channel_params *params);

/* Enqueue the reduction on `stream` (device pointers):
 *   d_bin_mask   [n_epochs][fft_len / 32]      as crn_sense_run_device_cfar writes it (8-byte aligned)
 *   d_spectrum   [n_epochs][fft_len]           the `spectrum` output of the same launch (16-byte aligned), or NULL: every power is 0
 *   d_stats      [n_streams][n_channels]       the records (16-byte aligned): read (unless first != 0), then rewritten
 *   d_busy       [n_epochs] uint64, or NULL    bit c = channel c busy in that epoch (8-byte aligned)
 *   d_power      [n_epochs][n_channels] fp32, or NULL   (16-byte aligned; refused without d_spectrum)
 *   d_workspace  workspace_bytes >= crn_channels_workspace_bytes of scratch (8-byte aligned); its contents before and after mean nothing
 * `h` supplies fft_len and the device, nothing else: the mask and rows may come from any source, the handle may be of any mode, with
 * CFAR on or off.  Only enqueues (three small launches), allocates nothing, keeps no host state; integer fields do not depend on the
 * order the work ran in.  CRN_ERR_ARG, decided before any device call, for a NULL h, params, d_bin_mask, d_stats or d_workspace;
 * n_epochs < 0; n_channels outside 1..64; a span with lo outside 0 .. fft_len - 1 or width outside 1 .. fft_len; min_bins < 1;
 * epochs_per_stream < 1 or not dividing n_epochs; a nonzero reserved field; d_power without d_spectrum; a misaligned pointer; a
 * workspace too small.  n_epochs = 0 succeeds and launches nothing, with first != 0 too (the records are then left as they are). */
CRN_API int crn_channels_device(crn_handle *h, const uint32_t *d_bin_mask, const float *d_spectrum, int64_t n_epochs,
                                const crn_channel_params *params, crn_channel_stats *d_stats, uint64_t *d_busy, float *d_power,
                                void *d_workspace, int64_t workspace_bytes, void *stream);

/* A record as a two-state Markov chain, host only (`s` is a host copy of one record):
 *   p01 = (n_trans[0][1] + prior) / (n_trans[0][0] + n_trans[0][1] + 2 prior), p10 likewise from n_trans[1][.]; a 0 / 0 gives 0.5
 *   p_idle = the probability that every one of the next `horizon` epochs is idle: (1 - p01)^horizon from an idle state (state & 1 = 0),
 *            p10 (1 - p01)^(horizon - 1) from a busy one
 * prior = 1 is Laplace's rule, 0 the plain frequencies.  Any output pointer may be NULL.  CRN_ERR_ARG for a NULL s, horizon < 1, or a
 * negative or non-finite prior. */
CRN_API int crn_channel_forecast(const crn_channel_stats *s, int32_t horizon, double prior, double *p01, double *p10, double *p_idle);

/* -- cooperative sensing: the masks and spectra of a group of sensors fused into one ------------------------------------------
 * Every stage above works on one stream, one node's receiver.  This one combines what a group of sensors on the same band, aligned in
 * time, saw: M rows in, one row out.  A batch is laid out as for crn_tracks_device: n_epochs = S T, S streams of T = epochs_per_stream
 * epochs in time order; M = group_size, S = G M, and group j is the streams j M .. j M + M - 1.  Fused row r = j T + t is formed from
 * the member epochs (j M + m) T + t, m = 0 .. M - 1; N = fft_len.  The outputs have the layout of a batch of G streams, so they feed
 * crn_segments_device, crn_tracks_device, crn_tracks_carry_device and crn_channels_device unchanged, with n_epochs = G T.
 *   Active members   member m is active when weight[m] > 0; at least one must be.  An inactive member takes no part in anything: its
 *                    rows and mask words are never read, so whatever they hold (a NaN, say) reaches no output.
 *   Fused row        written whenever d_spectrum and d_fused_spectrum are given, under either rule:
 *                      F[k] = fl32( sum (double)w_m (double)P_m[k] ), over the active m in ascending order, accumulated in fp64 and
 *                    rounded to fp32 once.  (A product of two fp32 values is exact in fp64: a fused multiply-add and a separate
 *                    multiply and add give the same bits.)  The weights are not normalised: equal-gain combining is w_m = 1 / M, and
 *                    a caller who knows the members' noise floors passes their reciprocals.
 *   CRN_FUSE_VOTE    hard decision: fused bit k is set when at least `votes` active members have bit k set.  OR is votes = 1, AND is
 *                    votes = n_active, majority is votes = ceil(n_active / 2).  Needs d_bin_mask; the spectrum is optional.
 *   CRN_FUSE_SOFT    CA-CFAR on the fused row, every sum direct and in a fixed order.  With g = guard, W = train:
 *                      L = sum over i = g + 1 .. g + W, ascending, of (double)F[(k - i) mod N];  R the same with k + i;  T = L + R
 *                      bin k detected  <=>  (double)F[k] 2W > (double)alpha T   (fp64)
 *                    No sliding sum and no difference of prefix sums: a strong bin that enters and leaves such a sum leaves a residue
 *                    behind.  Needs d_spectrum; d_fused_spectrum may be NULL (the fused row then never leaves the chip); d_bin_mask
 *                    is optional.
 *                    alpha = crn_cfar_alpha(pfa, n_active K, W) holds the false-alarm rate at `pfa` under that function's noise model
 *                    with equal weights and equal noise power at every member: the mean of n_active independent K-frame means is
 *                    Gamma(n_active K).  Sensors with unequal floors, or correlated sensors, move the real rate.
 *   Row header       n_detected = set bits of the fused mask; n_any = bins set in at least one active member's mask, n_all = bins set
 *                    in all of them (both 0 without d_bin_mask: together they show how much the sensors disagree); n_active.
 *   Cut independence a batch gives the same bytes however it is cut along time or along groups. */
#define CRN_MAX_FUSE_MEMBERS 32
typedef enum crn_fuse_rule { CRN_FUSE_VOTE = 0, CRN_FUSE_SOFT = 1 } crn_fuse_rule;
typedef struct crn_fuse_params {
  int32_t rule, group_size, epochs_per_stream;
  int32_t votes;                      /* VOTE: k in 1..n_active.  SOFT: 0 */
  int32_t guard, train;               /* SOFT: crn_cfar_params' ranges: 1 <= train <= 64, guard >= 0, 2 (guard + train) + 1 <= fft_len.  VOTE: 0 */
  int32_t reserved[3];                /* 0 */
  float alpha;                        /* SOFT: > 0, finite.  VOTE: 0 */
  float weight[CRN_MAX_FUSE_MEMBERS]; /* w_m >= 0, finite; entries at m >= group_size must be 0 */
} crn_fuse_params; /* 168 bytes */
typedef struct crn_fuse_row {
  int32_t n_detected, n_any, n_all, n_active;
} crn_fuse_row; /* 16 bytes */

/* Enqueue the fusion on `stream`, one launch (device pointers):
 *   d_bin_mask        [n_epochs][fft_len / 32]        the members' masks (8-byte aligned); NULL under SOFT: n_any = n_all = 0
 *   d_spectrum        [n_epochs][fft_len]             the members' `spectrum` rows (16-byte aligned); NULL under VOTE: no fused row
 *   d_fused_mask      [n_epochs / M][fft_len / 32]    or NULL (8-byte aligned)
 *   d_fused_spectrum  [n_epochs / M][fft_len]         or NULL (16-byte aligned; refused without d_spectrum)
 *   d_rows            [n_epochs / M]                  or NULL (16-byte aligned)
 * `h` supplies fft_len and the device, nothing else: the arrays may come from any source, the handle may be of any mode.  Only
 * enqueues; allocates nothing, keeps no state, needs no workspace.  CRN_ERR_ARG, decided before any device call, for a NULL h or
 * params; all three outputs NULL; rule outside 0..1; group_size outside 1..32; epochs_per_stream < 1, or group_size epochs_per_stream
 * not dividing n_epochs; n_epochs < 0; a negative or non-finite weight; a nonzero weight at m >= group_size; no active member; a
 * nonzero reserved field; VOTE: NULL d_bin_mask, votes outside 1..n_active, or a nonzero guard, train or alpha; SOFT: NULL d_spectrum,
 * votes != 0, or guard, train or alpha outside the ranges above; d_fused_spectrum without d_spectrum; a misaligned pointer.
 * n_epochs = 0 succeeds and launches nothing. */
CRN_API int crn_fuse_device(crn_handle *h, const uint32_t *d_bin_mask, const float *d_spectrum, int64_t n_epochs,
                            const crn_fuse_params *params, uint32_t *d_fused_mask, float *d_fused_spectrum, crn_fuse_row *d_rows,
                            void *stream);

/* The per-sensor false-alarm probability p at which votes-of-n voting of independent sensors gives pfa_fused, host only:
 *   sum over j = k .. n of C(n, j) p^j (1 - p)^(n - j) = pfa_fused, solved by bisection in double.
 * The result goes into crn_cfar_alpha(p, K, W).  CRN_ERR_ARG for n outside 1..32, k outside 1..n, pfa_fused outside (0, 1) or a NULL
 * pfa_member. */
CRN_API int crn_fuse_member_pfa(double pfa_fused, int32_t n, int32_t k, double *pfa_member);

/* -- spectrum holes: which parts of the band are free now, how wide, for how long, how quiet -----------------------------------
 * crn_channels_device answers for spans the caller named in advance.  This stage answers for a user bound to no channel plan: the
 * maximal spans whose every bin has been clear for at least min_age epochs, the latest included (the intersection of the idle bins
 * over time, not their union).  A batch is laid out as for crn_tracks_device: n_epochs = S T, S streams of T = epochs_per_stream
 * epochs in time order; N = fft_len; bins are circular.  d_t[k] is bit k of epoch t's mask.
 *   1. blocked   b_t[k] = OR of d_t[(k + i) mod N] over |i| <= guard: a circular dilation of the epoch's mask.
 *   2. age       one int32 per stream and bin in the caller's d_age [S][N], its own carry; it holds values only, no index is ever
 *                read from it.  a = first ? 0 : max(d_age[k], 0); then for each epoch of the stream in time order
 *                a = b_t[k] ? 0 : min(a + 1, 2^31 - 1); the result is written back.  Equivalently: when the bin was blocked in the
 *                batch and the last such epoch is t*, a = T - 1 - t*; otherwise a = min(a_start + T, 2^31 - 1).  It is the number of
 *                consecutive epochs, ending with the latest, in which the bin was clear, left-censored at the first call.
 *   3. free      f[k] = age[k] >= min_age.  free_bins counts them before any width filter; d_free_mask [S][N / 32] has the bit
 *                layout of the bin mask.
 *   4. holes     the maximal circular runs of ones in f: bins (lo + i) mod N, 0 <= i < width.  f all ones: one hole, lo = 0,
 *                width = N; f all zero: none.  Runs with width < min_width are dropped, n_found counts the rest, the first
 *                min(n_found, max_holes) by ascending lo are stored (n_stored): a hole that crosses the wrap comes last.  Slots
 *                beyond n_stored are zero-filled.  widest_lo, widest_width and widest_age (that hole's `age`) describe the widest of
 *                all found holes, stored or not; ties go to the smallest lo; all three are 0 when there is none.
 *   5. fields    per stored hole, age is the smallest and age_max the largest age[k] inside it.  With d_spectrum,
 *                A = min(avg_epochs, T) and Pbar[k] = fl32(S_k / (double)A), S_k the fp64 sum of (double)P_t[k] over
 *                t = T - A .. T - 1 in ascending t; peak_bin is the absolute bin of the largest Pbar in the hole (ties: the smallest
 *                i) and peak_power that value; power = the sum of Pbar over the hole, accumulated in fp64 and rounded to fp32 once
 *                (direct: no bin outside the hole enters it); floor_mean = the fp64 sum of Pbar over all free bins divided by
 *                free_bins, rounded once, 0 when there are none.  Without d_spectrum power = peak_power = floor_mean = 0 and
 *                peak_bin = lo.
 *   6. cuts      a stream given in one call, and the same stream cut into several calls (first = 1, then 0), give identical d_age,
 *                d_free_mask and integer fields; the fields that come from Pbar (power, peak_power, floor_mean, and peak_bin with
 *                them) too when the last call of each cut has T >= avg_epochs, so that Pbar is the mean of the same rows. */
typedef struct crn_hole_params {
  int32_t epochs_per_stream; /* >= 1, divides n_epochs */
  int32_t first;             /* != 0: d_age's contents mean nothing, start afresh */
  int32_t guard;             /* 0..32: a detected bin also blocks its `guard` neighbours on each side */
  int32_t min_age;           /* 1..2^31-1: epochs a bin must have been idle, the latest included */
  int32_t min_width;         /* 1..fft_len */
  int32_t max_holes;         /* 1..256 */
  int32_t avg_epochs;        /* 1..64: rows averaged for the power fields */
  int32_t reserved;          /* 0 */
} crn_hole_params; /* 32 bytes */
typedef struct crn_hole {
  int32_t lo, width, age, age_max, peak_bin, reserved;
  float power, peak_power;
} crn_hole; /* 32 bytes */
typedef struct crn_hole_stream {
  int32_t n_found, n_stored, free_bins, widest_lo, widest_width, widest_age;
  float floor_mean;
  int32_t reserved;
} crn_hole_stream; /* 32 bytes */

/* Bytes of device scratch crn_holes_device needs for n_epochs epochs under `params`: needs no handle and no device (it is sized for
 * the largest fft_len).  Positive for valid arguments (also for n_epochs = 0), -1 for a NULL params, n_epochs < 0, epochs_per_stream
 * < 1 or not dividing n_epochs, guard outside 0..32, min_age < 1, min_width outside 1 .. the largest fft_len, max_holes outside
 * 1..256, avg_epochs outside 1..64, or a nonzero reserved. */
CRN_API int64_t crn_holes_workspace_bytes(int64_t n_epochs, const crn_hole_params *params);

/* Enqueue the stage on `stream`, two launches (device pointers):
 *   d_bin_mask   [n_epochs][fft_len / 32]      as crn_sense_run_device_cfar writes it (8-byte aligned)
 *   d_spectrum   [n_epochs][fft_len]           the `spectrum` output of the same launch (16-byte aligned), or NULL
 *   d_age        [n_streams][fft_len] int32    the carry (16-byte aligned): read (unless first != 0), then rewritten
 *   d_streams    [n_streams]                   the headers (16-byte aligned)
 *   d_holes      [n_streams][max_holes]        or NULL: headers only (16-byte aligned)
 *   d_free_mask  [n_streams][fft_len / 32]     or NULL (8-byte aligned)
 *   d_workspace  workspace_bytes >= crn_holes_workspace_bytes of scratch (8-byte aligned); its contents before and after mean nothing
 * `h` supplies fft_len and the device, nothing else.  Only enqueues, allocates nothing, keeps no host state.  CRN_ERR_ARG, decided
 * before any device call, for a NULL h, params, d_bin_mask, d_age, d_streams or d_workspace; n_epochs < 0; any parameter outside the
 * ranges above (min_width against the handle's fft_len); a nonzero reserved; a misaligned pointer; a workspace too small.
 * n_epochs = 0 succeeds and launches nothing, with first != 0 too (d_age is then left as it is). */
CRN_API int crn_holes_device(crn_handle *h, const uint32_t *d_bin_mask, const float *d_spectrum, int64_t n_epochs,
                             const crn_hole_params *params, int32_t *d_age, crn_hole_stream *d_streams, crn_hole *d_holes,
                             uint32_t *d_free_mask, void *d_workspace, int64_t workspace_bytes, void *stream);

/* -- wideband detection against an excised noise floor (LAD, localisation by double thresholding) -------------------------------
 * The CFAR detectors compare a bin with its neighbours and are blind to an emitter wider than the training window: its interior
 * bins have the emitter on both sides.  This stage finds the noise floor of the row itself by forward consecutive mean excision
 * (FCME), thresholds every bin against it, and accepts a run of bins over a lower threshold only where it holds a bin over an upper
 * one.  Per epoch, no state, no calibrated noise power.  Its output has the layout of the CFAR mask, so every stage above takes it.
 * One row is P[0..N), N = fft_len, the `spectrum` output of one epoch; the values are taken as non-negative finite fp32 (for a row
 * that holds anything else that row's outputs are unspecified, and nothing outside them is touched).  The row is cut into n_blocks
 * blocks of M = N / n_blocks >= 256 bins, block b the bins [b M, (b + 1) M), each with a floor of its own (the receiver's floor is
 * not flat: filter roll-off).
 *   1. floor       x_(1) <= .. <= x_(M) the block's values ascending, C_n = sum of (double)x_(i) over i <= n,
 *                  n0 = max(1, M init_percent / 100) (integer division).  n* is the smallest n in n0 .. M with n == M or
 *                  (double)x_(n+1) n > (double)t_cme C_n.  floor_b = C_n* / n* in fp64; d_floor[row][b] is that rounded to fp32 once.
 *   2. thresholds  lower[k]  <=>  (double)P[k] n* > (double)t_lower C_n*, with n* and C_n* of k's block; upper[k] the same with
 *                  t_upper.  t_lower <= t_upper: upper is a subset of lower.
 *   3. clusters    the maximal circular runs of ones in `lower` (lower all ones: one cluster of width N).  A cluster is kept when
 *                  it holds at least one `upper` bin; det is the union of the kept clusters.  A cluster may cross block edges and
 *                  the wrap.
 *   4. output      out = det | or_mask, or_mask an optional input in the mask layout (the CFAR mask of the same launch, so that
 *                  one mask carries both detectors); it may be the same address as d_bin_mask.
 *   5. header      n_lower, n_upper: the set bits of lower and upper; n_detected: the set bits of out; n_clusters: kept clusters;
 *                  n_rejected: clusters without an upper bin; n_clean: the sum of n* over the blocks; floor_min, floor_max: the
 *                  smallest and the largest d_floor of the row.
 *   6. arithmetic  the fp64 sums may be added in any order.  A row is decided when every comparison of steps 1-2 that the
 *                  ascending-order evaluation makes has |lhs / rhs - 1| > 2^-36 (or both sides 0); decided rows have exactly the
 *                  outputs of that evaluation (x n is exact in fp64, and C_n in another order moves by at most M 2^-53 relative).
 *   Limits         the floor needs noise to stand on: a block that an emitter fills, or a row occupied beyond about 80 %, puts the
 *                  floor on the emitter.  Rows are independent: a batch gives the same bytes however it is cut. */
typedef struct crn_lad_params {
  int32_t n_blocks;       /* 1, 2, 4, 8; fft_len / n_blocks >= 256 */
  int32_t init_percent;   /* 1..50: the share of a block taken as surely noise */
  float t_cme;            /* > 0, finite: crn_lad_factor(pfa_cme, K, 0) */
  float t_lower, t_upper; /* > 0, finite, t_lower <= t_upper: crn_lad_factor(pfa, K, t_cme) */
  int32_t reserved[3];    /* 0 */
} crn_lad_params; /* 32 bytes */
typedef struct crn_lad_row {
  int32_t n_lower, n_upper, n_detected, n_clusters, n_rejected, n_clean;
  float floor_min, floor_max;
} crn_lad_row; /* 32 bytes */

/* Enqueue the stage on `stream`, one launch (device pointers):
 *   d_spectrum  [n_epochs][fft_len]            `spectrum` rows (16-byte aligned)
 *   d_or_mask   [n_epochs][fft_len / 32]       or NULL (8-byte aligned); may be d_bin_mask itself
 *   d_bin_mask  [n_epochs][fft_len / 32]       or NULL (8-byte aligned)
 *   d_rows      [n_epochs]                     or NULL (16-byte aligned)
 *   d_floor     [n_epochs][n_blocks] float     or NULL (4-byte aligned)
 * `h` supplies fft_len and the device, nothing else.  Only enqueues; allocates nothing, keeps no state, needs no workspace.
 * CRN_ERR_ARG, decided before any device call, for a NULL h, params or d_spectrum; all three outputs NULL; n_blocks outside
 * {1, 2, 4, 8} or fft_len / n_blocks < 256; init_percent outside 1..50; t_cme, t_lower or t_upper not finite or <= 0;
 * t_lower > t_upper; a nonzero reserved; n_epochs < 0; a misaligned pointer.  n_epochs = 0 succeeds and launches nothing. */
CRN_API int crn_lad_device(crn_handle *h, const float *d_spectrum, int64_t n_epochs, const crn_lad_params *params,
                           const uint32_t *d_or_mask, uint32_t *d_bin_mask, crn_lad_row *d_rows, float *d_floor, void *stream);

/* The factors of crn_lad_params from false-alarm rates, host only, under crn_cfar_alpha's noise model (P is Gamma(K), mean 1,
 * K = frames_per_epoch):
 *   t_cme == 0   factor = G_K^-1(1 - pfa) / K, the plain quantile: this gives t_cme itself.
 *   t_cme > 0    that quantile divided by m, the mean FCME converges to in noise: the fixed point of
 *                m = P(K + 1, K t_cme m) / P(K, K t_cme m), iterated from m = 1 (P the regularised lower incomplete gamma).  The
 *                excised floor sits below the true mean, and an uncorrected threshold runs high.
 * Blocks much smaller than 256 bins bias the floor further down (the n0 smallest of few values): hence M >= 256.
 * CRN_ERR_ARG for pfa outside (0, 1), frames_per_epoch < 1, a negative or non-finite t_cme, or a NULL factor. */
CRN_API int crn_lad_factor(double pfa, int32_t frames_per_epoch, double t_cme, double *factor);

/* -- ordered-statistic CFAR along time, per bin (the radar "clutter-map" CFAR) -----------------------------------------------------
 * The CFAR detectors and crn_lad_device take their noise reference from the other bins of the same row.  This stage takes it from the
 * same bin's own past: a floor of any shape in frequency, a fixed spur and a DC spike are constant in time and therefore floor, and an
 * emitter of any width is seen whole.  Its output has the layout of the CFAR mask, so every stage above takes it.  A batch is laid out
 * as for crn_tracks_device: n_epochs = S T, S streams of T = epochs_per_stream epochs in time order; N = fft_len; P_n[k] is bin k of
 * the `spectrum` row of the stream's epoch n.  Per stream, `seen` is the number of epochs given in earlier calls: 0 when first != 0,
 * otherwise d_seen[stream] read as a value and clamped to 0 .. 2^62.  Epoch t of the call has the global index n = seen + t.
 * D = cells, g = guard_epochs, H = D + g.
 *   1. cells     for n >= H the cells of (n, k) are c_i = P_(n-g-i)[k], i = 1..D: the bin's own D epochs before the g guard epochs.  A
 *                row comes from the batch where it lies inside the batch and from the history otherwise.  For n < H there are no
 *                cells: the bin is not detected and n_cells = 0 (the warm-up).
 *   2. test      det  <=>  at least `rank` cells satisfy fl32(alpha c_i) < P_n[k]: an fp32 product and an fp32 compare, strict, a tie
 *                counts as "not below".  It is the counting form of CRN_CFAR_OS on K-frame means, so
 *                crn_cfar_alpha_ex(CRN_CFAR_OS, pfa, K, cells / 2, rank) gives alpha (K-frame means of disjoint epochs are independent).
 *   3. output    out = det | or_mask, or_mask an optional input in the mask layout (the CFAR or LAD mask of the same rows, so that
 *                one mask carries every detector); it may be the same address as d_bin_mask.
 *   4. header    n_detected: the set bits of out; n_new: the bits of det not in or_mask; n_cells: 0 in the warm-up, D after it.
 *   5. history   the caller owns d_hist [S][H][N] fp32 and d_seen [S] int64.  The row of global epoch n lives in slot n mod H.  After
 *                the call the slots of the last min(H, seen + T) epochs hold those rows and d_seen = seen + T.  Slots of epochs never
 *                seen are never read.  No index is read from either array (n mod H is in range whatever d_seen holds): a foreign
 *                buffer costs wrong bits and nothing else.
 *   6. cuts      a stream given in one call, and the same stream cut anywhere into several calls (first = 1, then 0), give identical
 *                masks, headers, d_seen and written history slots.
 *   7. values    taken as non-negative finite fp32.  For a bin whose test value or cells hold anything else that bin's outputs are
 *                unspecified, and nothing outside the outputs is touched.
 *   Limits       a bin that is busy in more than D - rank of its D cells raises its own threshold, and an always-on emitter is floor:
 *                the blind spot is the complement of the other detectors', hence the OR.  The first H epochs of a stream yield
 *                nothing.  alpha assumes that cells and test are independent: true of disjoint epochs whatever the window, not of
 *                Welch epochs that share fft_len - hop samples with their neighbour (guard_epochs >= 1 keeps the test clear of it;
 *                neighbouring cells stay correlated). */
typedef struct crn_tcfar_params {
  int32_t epochs_per_stream; /* >= 1, divides n_epochs */
  int32_t first;             /* != 0: d_hist's and d_seen's contents mean nothing, start afresh */
  int32_t cells;             /* D: even, 2..128 (train = cells / 2 is within crn_cfar_alpha_ex's 1..64) */
  int32_t guard_epochs;      /* g: 0..16 */
  int32_t rank;              /* 1..cells */
  float alpha;               /* > 0, finite: crn_cfar_alpha_ex(CRN_CFAR_OS, pfa, K, cells / 2, rank) */
  int32_t reserved[2];       /* 0 */
} crn_tcfar_params; /* 32 bytes */
typedef struct crn_tcfar_row {
  int32_t n_detected, n_new, n_cells, reserved;
} crn_tcfar_row; /* 16 bytes */

/* Bytes of d_hist for n_streams streams of fft_len bins under `params`, n_streams (cells + guard_epochs) fft_len 4: needs no handle and
 * no device.  -1 for a NULL params, n_streams < 1, an fft_len other than 512, 1024, 2048 or 4096, epochs_per_stream < 1, cells odd or
 * outside 2..128, guard_epochs outside 0..16, rank outside 1..cells, an alpha that is not finite or <= 0, or a nonzero reserved. */
CRN_API int64_t crn_tcfar_hist_bytes(int64_t n_streams, int32_t fft_len, const crn_tcfar_params *params);

/* Enqueue the stage on `stream`, at most three launches (device pointers):
 *   d_spectrum  [n_epochs][fft_len]                `spectrum` rows (16-byte aligned)
 *   d_or_mask   [n_epochs][fft_len / 32]           or NULL (8-byte aligned); may be d_bin_mask itself
 *   d_bin_mask  [n_epochs][fft_len / 32]           or NULL (8-byte aligned)
 *   d_rows      [n_epochs]                         or NULL (16-byte aligned)
 *   d_hist      [n_streams][cells + guard_epochs][fft_len] float, crn_tcfar_hist_bytes of them (16-byte aligned): read (unless
 *               first != 0), then the batch's last rows are written
 *   d_seen      [n_streams] int64 (8-byte aligned): read (unless first != 0), then rewritten
 * d_bin_mask and d_rows both NULL is allowed: the call then only feeds the history.  `h` supplies fft_len and the device, nothing
 * else.  Only enqueues, allocates nothing, keeps no host state.  CRN_ERR_ARG, decided before any device call, for a NULL h, params,
 * d_spectrum, d_hist or d_seen; n_epochs < 0; any parameter outside the ranges above; a nonzero reserved; a misaligned pointer.
 * n_epochs = 0 succeeds, launches nothing and leaves d_hist and d_seen as they are, with first != 0 too. */
CRN_API int crn_tcfar_device(crn_handle *h, const float *d_spectrum, int64_t n_epochs, const crn_tcfar_params *params,
                             const uint32_t *d_or_mask, uint32_t *d_bin_mask, crn_tcfar_row *d_rows, float *d_hist, int64_t *d_seen,
                             void *stream);

/* -- what a segment is: occupied bandwidth, x-dB bandwidth and shape --------------------------------------------------------------
 * crn_segments_device gives the mask's idea of an emitter; its width is the width of the detected bits plus what merge_gap closed and
 * moves with the false-alarm rate.  This stage measures each stored segment on its own `spectrum` row with the two widths spectrum
 * monitoring quotes: the occupied bandwidth, the span that holds all but a small share of the power (ITU-R SM.443's beta / 2 rule), and
 * the x-dB bandwidth, the outermost points that still rise above peak - x dB.  With the crest they tell a carrier from a flat wideband
 * signal from a multicarrier.  The powers of a segment are turned into integers once and every sum is an integer sum, so the result
 * has no rounding freedom: it is the same in any order of addition.  N = fft_len, fl32(.) is one fp32 operation.
 * Per epoch e, for each slot s < min(max(d_epochs[e].n_stored, 0), max_segments) of d_segments[e], with row P and lo, width = w and
 * peak_power from the record:
 *   1. noise     nm = the epoch's noise_mean if subtract_noise is set and it is finite and > 0, otherwise 0.
 *   2. net bins  Q[i] = fl32(P[(lo + i) mod N] - nm), 0 <= i < w; Q[i] counts as 0 unless Q[i] > 0 (NaN included).
 *                pq = fl32(peak_power - nm).
 *   3. integers  e = the binary exponent of peak_power (2^e <= peak_power < 2^(e+1), subnormals included: frexp's, less one).
 *                q[i] = min(trunc(Q[i] 2^(30 - e)), 2^31 - 1): a scaling by a power of two, exact.  q[i] < 2^31, S0 = sum q < 2^43 and
 *                S0 tail_ppm < 2^62: every sum is an exact integer in int64 (and in fp64).
 *   4. occupied  T = (S0 tail_ppm) div 10^6, C[i] = q[0] + .. + q[i], C[-1] = 0.  obw_lo = the smallest i with C[i] > T; the last bin
 *                is the largest i with S0 - C[i-1] > T; obw_width = last - obw_lo + 1, >= 1 whenever S0 > 0 (T < S0 / 2).
 *   5. x dB      thr = fl32(xdb_ratio pq).  A bin is above when Q[i] > thr, strictly.  xdb_lo = the first such i, xdb_width spans to
 *                the last one, n_above = their count (none above: all three are 0).  n_above / xdb_width is the fill: 1 for a solid
 *                emitter, less for a multicarrier.
 *   6. floats    net_power = fl32(S0 2^(e - 30)); crest = fl32((double) max q w / (double) S0), one fp64 division rounded to fp32: near
 *                w for a carrier, near 1 for a flat emitter.
 *   7. nothing   the whole record is zero bytes when lo is outside 0 .. N - 1, width outside 1 .. N, peak_power not finite or not > 0,
 *                pq not > 0, or S0 = 0.  Slots at and beyond n_stored are zero-filled, as crn_segments_device does: a batch gives
 *                the same bytes however it is cut into launches.  obw_width == 0 is the caller's test for "not measured".
 * Offsets count from the segment's own lo, like centroid: the absolute bin is (lo + obw_lo) mod N.
 *   Limits       the clamp at 0 keeps the half of the noise's fluctuation that lies above noise_mean, so a weak lone carrier's
 *                99 % width is several bins and not 1; a record whose peak_power is not its row's (a foreign array) measures
 *                against that peak_power and costs wrong numbers, nothing else. */
typedef struct crn_measure_params {
  int32_t max_segments;   /* as given to crn_segments_device: 1 .. 256 */
  int32_t tail_ppm;       /* share of the net power left outside on EACH side, in 1e-6: 0 .. 499999 (SM.443's 99 %: 5000) */
  float xdb_ratio;        /* linear power ratio of the x-dB rule, finite, 0 <= r < 1 (26 dB: 10^-2.6) */
  int32_t subtract_noise; /* 0 | 1: take the epoch's noise_mean off every bin first */
  int32_t reserved[4];    /* 0 */
} crn_measure_params; /* 32 bytes */
typedef struct crn_measure {
  int32_t obw_lo, obw_width, xdb_lo, xdb_width; /* offsets count from the segment's own lo */
  int32_t n_above;
  float net_power, crest, reserved;
} crn_measure; /* 32 bytes */

/* Enqueue the measurement on `stream` over n_epochs rows, one launch (device pointers, all 16-byte aligned):
 *   d_spectrum  [n_epochs][fft_len]        the rows the segments were cut from
 *   d_epochs    [n_epochs]                 the headers crn_segments_device wrote (n_stored and noise_mean are read)
 *   d_segments  [n_epochs][max_segments]   its records (lo, width and peak_power are read)
 *   d_measures  [n_epochs][max_segments]   one record per slot, every slot written
 * `h` supplies fft_len and the device, nothing else.  Allocates nothing, keeps no state, needs no workspace.  Whatever bytes d_epochs
 * and d_segments hold, only the epoch's own row and records are read and only its own max_segments slots written.  CRN_ERR_ARG for a
 * NULL h, params, d_spectrum, d_epochs, d_segments or d_measures; max_segments outside 1 .. 256; tail_ppm outside 0 .. 499999; an
 * xdb_ratio that is not finite or outside [0, 1); subtract_noise other than 0 or 1; a nonzero reserved; n_epochs < 0; any of the four
 * arrays not 16-byte aligned.  n_epochs = 0 succeeds and touches nothing. */
CRN_API int crn_measure_device(crn_handle *h, const float *d_spectrum, int64_t n_epochs, const crn_measure_params *params,
                               const crn_segment_epoch *d_epochs, const crn_segment *d_segments, crn_measure *d_measures, void *stream);

/* -- what a segment is: the symbol rate from the cyclic spectrum ---------------------------------------------------------------------
 * Every stage above works on `spectrum` rows, K-frame means of |X|^2: an RRC-QPSK carrier, a band of noise and an OFDM block of the same
 * width give crn_measure_device the same record.  A digitally modulated carrier correlates spectral components that lie one symbol rate
 * apart; stationary noise of any colour does not.  This stage forms that correlation from the per-frame complex spectra, normalised by
 * the power in both components (a spectral coherence: no calibrated noise power is needed), over every stored segment, and reports the
 * strongest cell, hence the symbol rate.  It describes detected segments; it is not a detector below the noise (at 0 dB in-band the
 * feature of a 62-bin segment is lost with 32 frames).
 * N = fft_len; F = params.frames; X_f[k] is bin k of the complex spectrum of frame f of an epoch: d_frames is [n_epochs][F][N]
 * interleaved complex fp32, what crn_fft_forward_device writes for n_epochs F consecutive disjoint frames of N samples (the stage does
 * not care where the array came from).  Per epoch e and slot s < d_epochs[e].n_stored, with lo and width read from d_segments[e][s]:
 *   1. span      every value read from the records is clamped first: n_stored to 0 .. max_segments, lo to lo mod N (0 .. N - 1), width
 *                to 0 .. N.  w = min(width, max_width); lo' = (lo + (width - w) div 2) mod N: the central w bins of the segment.
 *   2. cells     (a, q) for a = a_lo .. a_lo + n_a - 1 and q = 0 .. F - 1.  n_pairs(a) = w - a.  A cell is tested when
 *                n_pairs(a) >= min_pairs.
 *   3. pairs     for i = 0 .. n_pairs - 1, with k = (lo' + i) mod N and k' = (lo' + i + a) mod N:
 *                    C = sum over f of X_f[k'] conj(X_f[k]) e^(-j 2 pi q f / F)        P[k] = sum over f of |X_f[k]|^2
 *                    rho = |C|^2 / (P[k'] P[k]), and rho = 0 when the product is 0
 *                in fp32 throughout; the order of the operations is the implementation's (the kernel divides every column by
 *                sqrt(P) first and takes C from a radix-2 transform over f), so S below is defined to within 8 F 2^-24 absolute of its
 *                exact value and the same build gives the same bytes.  That holds for spectra of any scale whose P[k] are normal
 *                fp32 numbers, about 1e-18 <= |X| <= 1e18: P[k'] P[k] and |C|^2 themselves are never formed.
 *   4. statistic S(a, q) = (sum over i of rho) / n_pairs, the sum in fp64, rounded to fp32 once; 0 <= S <= 1.
 *                z(a, q) = fl32((F S - 1) sqrt(n_pairs (F + 1) / (F - 1))), formed in fp64 from the fp32 S.  Under white Gaussian noise,
 *                a rectangular window and disjoint frames rho follows Beta(1, F - 1): z has mean 0 and variance 1.
 *   5. record    (a, q) = the tested cell of largest z, ties to the smallest a and then the smallest q; n_pairs = n_pairs(a); stat = S
 *                there; stat_lo and stat_hi = S at (a - 1, q) and (a + 1, q), each 0 where that cell lies outside a_lo .. a_lo + n_a - 1
 *                or is not tested; n_over = the tested cells with z >= z_min.  With no tested cell the record is all zero bytes, and so
 *                are the slots at and beyond n_stored: a batch gives the same bytes however it is cut into launches.
 *   6. profile   d_profile, optional, [n_epochs][max_segments][n_a][F] fp32: S, with 0 for cells not tested and for empty slots.
 * The feature's cyclic frequency is congruent to q / F modulo one bin and the nearest separation is a: the symbol rate in bins is the
 * value congruent to q / F that lies nearest a.  A carrier between two separations answers in (a, q) and (a + 1, q), hence the two
 * neighbour values (crnsense.cyclo_bins interpolates over them).
 *   Limits       an off-grid CW carrier under the rectangular window gives S ~ 0.99 at q = 0 for every a (its leakage is coherent):
 *                such segments are recognised by `crest` of crn_measure_device, not here.  The leakage skirt around a strong
 *                modulated carrier is coherent in the same way: a segment that reaches well into it (80 bins around a 60-bin carrier
 *                38 dB over the noise) has its largest z at q = 0.  Keep the span to the occupied band, by a detection threshold
 *                above the skirt or by max_width = the channel's width.  Only the non-conjugate cyclic spectrum is
 *                formed: the carrier-frequency features of BPSK and MSK are not.  The feature lives where the two shifted copies of
 *                the pulse overlap, about roll-off x symbol rate bins, so a narrow segment at N = 512 has few pairs.  Disjoint frames
 *                under the rectangular window leak between adjacent a. */
typedef struct crn_cyclo_params {
  int32_t max_segments; /* as given to crn_segments_device: 1 .. 256 */
  int32_t frames;       /* F: 8, 16, 32 or 64 */
  int32_t a_lo;         /* the first separation in bins, >= 1 */
  int32_t n_a;          /* separations: 1 .. 128, a_lo + n_a - 1 <= fft_len / 2 */
  int32_t max_width;    /* bins of a segment that are looked at, the central ones: 2 .. 1024 */
  int32_t min_pairs;    /* a cell needs this many pairs: 1 .. max_width */
  int32_t reserved[2];  /* 0 */
  float z_min;          /* finite: crn_cyclo_zmin */
} crn_cyclo_params; /* 36 bytes */
typedef struct crn_cyclo {
  int32_t a, q, n_pairs, n_over;
  float stat, stat_lo, stat_hi, z;
} crn_cyclo; /* 32 bytes */

/* Enqueue the stage on `stream` over n_epochs epochs, one launch (device pointers, all 16-byte aligned):
 *   d_frames    [n_epochs][frames][fft_len] complex fp32   the per-frame spectra
 *   d_epochs    [n_epochs]                                 the headers crn_segments_device wrote (n_stored is read)
 *   d_segments  [n_epochs][max_segments]                   its records (lo and width are read)
 *   d_cyclo     [n_epochs][max_segments]                   one record per slot, every slot written
 *   d_profile   [n_epochs][max_segments][n_a][frames] fp32, or NULL
 * `h` supplies fft_len and the device, nothing else.  Only enqueues; allocates nothing, keeps no state, needs no workspace.  Whatever
 * bytes d_epochs and d_segments hold, only the epoch's own frames and records are read and only its own slots written.  Fixed
 * reduction orders and no floating-point atomics: the same call repeated gives the same bytes.  CRN_ERR_ARG, decided before any device
 * call, for a NULL h, params, d_frames, d_epochs, d_segments or d_cyclo; n_epochs < 0; any parameter outside the ranges above; a z_min
 * that is not finite; a nonzero reserved; any of the five arrays not 16-byte aligned.  n_epochs = 0 succeeds and launches nothing. */
CRN_API int crn_cyclo_device(crn_handle *h, const float *d_frames, int64_t n_epochs, const crn_cyclo_params *params,
                             const crn_segment_epoch *d_epochs, const crn_segment *d_segments, crn_cyclo *d_cyclo, float *d_profile,
                             void *stream);

/* z_min for a false-alarm probability pfa per tested cell, host only.  An approximation: the sum of n_pairs Beta(1, F - 1) values is
 * matched in mean and variance by a Gamma law of shape g = n_pairs (F + 1) / (F - 1), whose upper tail Q(g, g + z sqrt(g)) is inverted
 * by bisection.  (The rho of neighbouring pairs share a column and the true tail is not Gamma's: in simulated noise the realised rate
 * at pfa = 1e-2 lay between 0.8 and 1.05 times the nominal one for 23 to 54 pairs.)  Cells of different n_pairs have different thresholds: pass the
 * smallest n_pairs in use, min_pairs, which is the conservative choice.  CRN_ERR_ARG for pfa outside (0, 1), frames other than 8, 16,
 * 32 or 64, n_pairs < 1 or a NULL z_min. */
CRN_API int crn_cyclo_zmin(double pfa, int32_t frames, int32_t n_pairs, double *z_min);

/* -- occupancy map: what every bin did over time -------------------------------------------------------------------------------
 * The occupancy survey of spectrum monitoring (ITU-R SM.2256), per bin: how often each frequency is occupied, how often it changes
 * state and how long it stays busy or idle, the highest and lowest level seen there (max hold, min hold), and the mean level while
 * idle and while busy.  The mean level while idle, power[0] / (n_epochs - n_busy), is the receiver's noise floor bin by bin: its shape,
 * which noise_mean of the segment stage and the floor of crn_lad_device, one number per row or block, cannot show.
 * crn_channels_device keeps such a record for at most 64 spans named in advance and crn_holes_device one number per bin; this stage
 * keeps one record per stream and bin, in the caller's device memory, its own carry from call to call.  A batch is laid out as for
 * crn_tracks_device: S = n_epochs / epochs_per_stream streams of T = epochs_per_stream epochs in time order; N = fft_len.
 * For stream j, bin k and epoch t: s = bit k of the mask row; P = the `spectrum` value (0 when d_spectrum is NULL); u = the bit pattern
 * of P as uint32 (0 when d_spectrum is NULL).  For the non-negative values a power row holds, unsigned order of u is numeric order,
 * +inf lies above every finite value and NaN above that; umax and umin below compare u, so a negative value, which no power row
 * holds, counts as above every positive one.  sat(x) = min(x, 2^31 - 1).  The sequential rule is the definition:
 *       R = the carried record; taken as all zero when params.first != 0 or R.n_epochs <= 0
 *       R.run = max(R.run, 0)
 *       for each epoch of the stream in time order:
 *           if R.n_epochs > 0:
 *               a = R.state & 1
 *               if s != a:
 *                   if a == 0: R.n_rise = sat(R.n_rise + 1)
 *                   else:      R.n_fall = sat(R.n_fall + 1)
 *                   R.run_max[a] = max(R.run_max[a], R.run); R.run = 0
 *               R.max_hold = umax(R.max_hold, u); R.min_hold = umin(R.min_hold, u)
 *           else:
 *               R.max_hold = R.min_hold = u
 *           R.state = s; R.run = sat(R.run + 1); R.n_epochs = sat(R.n_epochs + 1)
 *           R.n_busy = sat(R.n_busy + s); R.power[s] += (double)P
 *       R.reserved = 0
 *     The first run starts with the first observed epoch (it is left-censored) and is counted when it ends, as in crn_channel_stats;
 *     the run in progress is in no completed figure.  No index is ever read from a record: whatever bytes the carry holds, the call
 *     reads and writes only its own arrays.
 *   Usual mask     d_usual_mask [S][N / 32], optional, in the bit layout of the bin mask: bit k is set when n_epochs > 0 and
 *                  (int64)n_busy 10^6 >= (int64)duty_ppm n_epochs, on the record as the call leaves it.  It is the band plan of the
 *                  emitters that are usually there, and feeds crn_segments_device, crn_holes_device and crn_channels_device unchanged.
 *   Header         one crn_occmap_stream per stream: busy_sum = the sum of n_busy over the bins; n_epochs = that of bin 0;
 *                  usual_bins = the bits of the usual mask, counted whether or not the mask is asked for; clear_bins = bins with
 *                  n_busy == 0; busy_now = bins with state & 1 set.
 *   Cut independence   a stream given in one call and the same stream cut into several calls (first = 1, then 0) give identical
 *                  integer fields, state, max_hold and min_hold, an identical usual mask and identical headers.  power[] is an fp64
 *                  sum whose order depends on the cut and on the kernels' chunks of 64 epochs: within n_epochs 2^-52 relative of the
 *                  exact sum for non-negative rows.  Within one build the same call repeated gives the same bytes, power[] included
 *                  (a fixed order, no floating-point atomics). */
typedef struct crn_occmap_params {
  int32_t epochs_per_stream; /* >= 1, divides n_epochs */
  int32_t first;             /* != 0: the records' contents mean nothing, start afresh */
  int32_t duty_ppm;          /* 1 .. 1000000: the busy fraction, in 1e-6, from which a bin is in the usual mask */
  int32_t reserved[5];       /* 0 */
} crn_occmap_params; /* 32 bytes */
typedef struct crn_occmap_bin {
  int32_t n_epochs, n_busy;
  int32_t n_rise, n_fall;    /* idle->busy, busy->idle transitions */
  int32_t run, state;        /* length of the run in progress; bit 0 of state = the last epoch's s */
  int32_t run_max[2];        /* longest COMPLETED idle / busy run */
  float max_hold, min_hold;  /* compared as uint32 bit patterns */
  int32_t reserved[2];       /* written as 0 */
  double power[2];           /* fp64 sum of P over idle / busy epochs */
} crn_occmap_bin; /* 64 bytes */
typedef struct crn_occmap_stream {
  int64_t busy_sum;
  int32_t n_epochs, usual_bins, clear_bins, busy_now;
  int32_t reserved[2];       /* written as 0 */
} crn_occmap_stream; /* 32 bytes */

/* Bytes of device scratch crn_occmap_device needs for n_epochs epochs under `params`: needs no handle and no device (it is sized for
 * the largest fft_len).  Positive for valid arguments (also for n_epochs = 0), -1 for a NULL params, n_epochs < 0, epochs_per_stream
 * < 1 or not dividing n_epochs, duty_ppm outside 1 .. 1000000, or a nonzero reserved. */
CRN_API int64_t crn_occmap_workspace_bytes(int64_t n_epochs, const crn_occmap_params *params);

/* Enqueue the stage on `stream`, three launches (device pointers):
 *   d_bin_mask    [n_epochs][fft_len / 32]     as crn_sense_run_device_cfar writes it (8-byte aligned)
 *   d_spectrum    [n_epochs][fft_len]          the `spectrum` output of the same launch (16-byte aligned), or NULL: P = 0 and u = 0
 *   d_bins        [n_streams][fft_len]         the records (16-byte aligned): read (unless first != 0), then rewritten
 *   d_streams     [n_streams]                  the headers (16-byte aligned)
 *   d_usual_mask  [n_streams][fft_len / 32]    or NULL (8-byte aligned)
 *   d_workspace   workspace_bytes >= crn_occmap_workspace_bytes of scratch (16-byte aligned); its contents before and after mean nothing
 * `h` supplies fft_len and the device, nothing else: the mask and rows may come from any source, the handle may be of any mode, with
 * CFAR on or off.  Only enqueues, allocates nothing, keeps no host state.  CRN_ERR_ARG, decided before any device call, for a NULL h,
 * params, d_bin_mask, d_bins, d_streams or d_workspace; n_epochs < 0; epochs_per_stream < 1 or not dividing n_epochs; duty_ppm outside
 * 1 .. 1000000; a nonzero reserved field; a misaligned pointer; a workspace too small.  n_epochs = 0 succeeds and touches nothing,
 * with first != 0 too (the records are then left as they are). */
CRN_API int crn_occmap_device(crn_handle *h, const uint32_t *d_bin_mask, const float *d_spectrum, int64_t n_epochs,
                              const crn_occmap_params *params, crn_occmap_bin *d_bins, crn_occmap_stream *d_streams,
                              uint32_t *d_usual_mask, void *d_workspace, int64_t workspace_bytes, void *stream);

/* -- hops: how the channels move together -----------------------------------------------------------------------------------------
 * crn_channels_device keeps one two-state record per channel, each channel on its own.  A primary user that hops between channels (the
 * reference's CE_Random_Behaviour_PU and CE_PU_MARKOV_Chain_Tx, the interferer's TX_FREQ_BEHAVIOR_SWEEP) is one emitter whose next
 * channel depends on the one it is on: this stage counts, per stream, which channel was busy d epochs after which, for up to 8 lags d,
 * and the moves from one channel to another.  Its input is d_busy of crn_channels_device, one 64-bit busy word per epoch.  A batch is
 * laid out as for crn_channels_device: n_epochs / epochs_per_stream streams of epochs_per_stream consecutive epochs in time order.
 *   States     C = n_channels, 1..63.  The augmented word of an epoch is a = w & ((1 << C) - 1), and a = 1 << 63 when that is 0: index 63
 *              is the virtual channel "nothing busy", bits C..62 are never set, and the bits of d_busy at or above C, bit 63 included,
 *              are ignored.
 *   Lags       n_lags in 1..8, lag[m] strictly ascending, each in 1..64.
 *   Record     one per stream, in the caller's device memory, its own carry from call to call, 64 + 512 + 16384 + n_lags * 16896 bytes:
 *                int64 n_epochs (epochs seen so far); int32 n_channels, n_lags, lag[8] (unused entries 0), reserved[4] (0)   64 bytes
 *                uint64 hist[64]    bit k of hist[c] = bit c of the augmented word of epoch n_epochs - 1 - k, for k < min(n_epochs, 64);
 *                                   every other bit is 0
 *                int32 hop[64][64]
 *                per lag m: int32 from[64], to[64], pair[64][64]
 *   Rule       sequential, and the definition.  Per epoch, T = the stream's n_epochs before it, cur = its augmented word:
 *                for each lag m with T >= lag[m]:  prev = the augmented word of epoch T - lag[m] (from hist)
 *                    from[m][i] += 1 for every set bit i of prev;  to[m][j] += 1 for every set bit j of cur
 *                    pair[m][i][j] += 1 for every such i and j
 *                if T >= 1:  prev = the word of epoch T - 1;  fall = prev & ~cur;  rise = cur & ~prev
 *                    hop[i][j] += 1 for every i in fall and j in rise          (the moves; stays are left out)
 *                cur is shifted into hist;  n_epochs += 1
 *              Every int32 count saturates at 2^31 - 1.
 *   Carry      the record is taken as empty (all zero) when first != 0, when its n_epochs <= 0, or when its n_channels, n_lags or any
 *              lag[] differs from the call's (the call's lag[] entries at and above n_lags are not looked at and count as 0).  On
 *              reading, hist words are masked to k < min(n_epochs, 64) and to the channel positions c < C and c = 63, and a negative
 *              count is read as 0.  No index is ever read from a record, so a foreign buffer cannot cause an access outside the buffers.
 *   Cut independence   a stream given in one call and the same stream cut into several calls (first = 1, then 0) give identical bytes:
 *              everything is an integer, and saturating sums of non-negative terms do not depend on the order. */
typedef struct crn_hop_params {
  int32_t n_channels;        /* 1..63 */
  int32_t epochs_per_stream; /* >= 1, divides n_epochs */
  int32_t n_lags;            /* 1..8 */
  int32_t first;             /* != 0: the records' contents mean nothing, start afresh */
  int32_t lag[8];            /* lag[0 .. n_lags - 1] strictly ascending, each in 1..64 */
  int32_t reserved[4];       /* 0 */
} crn_hop_params; /* 64 bytes */

/* Bytes of n_streams records, and bytes of device scratch crn_hops_device needs for n_epochs epochs, under `params`: neither needs a
 * handle or a device.  -1 for a NULL params, a negative count, n_channels outside 1..63, n_lags outside 1..8, a lag outside 1..64 or
 * not above the one before it, epochs_per_stream < 1 (for the workspace: or not dividing n_epochs), or a nonzero reserved field;
 * otherwise the size (the workspace's is positive for n_epochs = 0 too). */
CRN_API int64_t crn_hops_bytes(int64_t n_streams, const crn_hop_params *params);
CRN_API int64_t crn_hops_workspace_bytes(int64_t n_epochs, const crn_hop_params *params);

/* Enqueue the stage on `stream`, two launches (device pointers):
 *   d_busy       [n_epochs] uint64                  one busy word per epoch (8-byte aligned)
 *   d_records    record_bytes >= crn_hops_bytes of the batch's streams (16-byte aligned): read (unless first != 0), then rewritten
 *   d_workspace  workspace_bytes >= crn_hops_workspace_bytes of scratch (8-byte aligned); its contents before and after mean nothing
 * `h` supplies the device and nothing else: the words may come from crn_channels_device, from the same stage run after
 * crn_fuse_device or on a mask of crn_lad_device, or from anywhere else.  Only enqueues, allocates nothing, keeps no host state; the
 * same call gives the same bytes.  CRN_ERR_ARG, decided before any device call, for a NULL h, params, d_busy, d_records or d_workspace;
 * n_epochs < 0; everything crn_hops_workspace_bytes refuses; a misaligned pointer; records or a workspace too small.  n_epochs = 0
 * succeeds and launches nothing, with first != 0 too (the records are then left as they are). */
CRN_API int crn_hops_device(crn_handle *h, const uint64_t *d_busy, int64_t n_epochs, const crn_hop_params *params, void *d_records,
                            int64_t record_bytes, void *d_workspace, int64_t workspace_bytes, void *stream);

/* Where the emitters seen now will be lag[m] epochs on, host only (`record` is a host copy of ONE record; `word` the busy word of the
 * epoch at hand, a its augmented word):
 *   p[j] = the largest, over the set bits i of a, of (pair[m][i][j] + prior) / (from[m][i] + 2 prior); a 0 / 0 gives 0.5
 *   p[j] = 0 for C <= j < 63; p[63] is the probability that nothing is busy lag[m] epochs on
 * With several emitters on the air a channel is taken to be as threatened as the most threatening of them makes it: that is the rule,
 * not an approximation of a joint model.  prior = 1 is Laplace's rule, 0 the plain frequencies.  CRN_ERR_ARG for a NULL pointer, m
 * outside 0 .. n_lags - 1, a negative or non-finite prior, or a head whose n_channels or n_lags is out of range. */
CRN_API int crn_hop_forecast(const void *record, int32_t m, uint64_t word, double prior, double p[64]);

/* -- extraction: a detected emitter as a baseband sample stream -------------------------------------------------------------------
 * The stages above find an emitter, follow it and describe it; this one hands out its samples, mixed to baseband, band-limited and
 * decimated, without the raw IQ leaving the device: an overlap-save (fast-convolution) channelizer on per-frame spectra.
 * N = fft_len.  d_spectra is [n_frames][N] interleaved complex fp32, what crn_fft_forward_device writes for samples_per_frame = N and
 * frame_stride = N / 2 (half-overlapped frames under no window; the stage cannot check that, it is the caller's contract).  n_frames
 * = S F: S streams of F = frames_per_stream consecutive frames each.  M = out_len, one of 16, 32, 64, 128, 256, M <= N / 2.  A channel
 * is a 16-byte record in device memory, so that a later stage can write it; kappa = centre mod N, taken into 0 .. N - 1 (also for
 * negative and extreme values).  d_taper[M] is fp32; entry j weights offset i = j - M / 2, so i runs over -M / 2 .. M / 2 - 1.  Per
 * channel c and frame t = 0 .. F - 1 of its stream, X_t that frame's spectrum and H the taper:
 *   1. taper     Z[i] = (fl32(Re X_t[(kappa + i) mod N] H[i]), fl32(Im X_t[(kappa + i) mod N] H[i]))
 *   2. block     y[n] = (1 / N) sum over i of Z[i] e^(+j 2 pi i n / M) for n = M / 4 .. 3 M / 4 - 1, the middle half of the block.  1 / N
 *                is a power of two: a tone of amplitude A on bin kappa comes out with amplitude A H[0].
 *   3. sign      y is negated when kappa (t0 + t) is odd: a hop of N / 2 samples turns the mixer e^(-j 2 pi kappa m / N) by e^(-j pi kappa).
 *                t0 is the index within the stream of the call's first frame; only its parity matters.
 *   4. row       d_out[c][t M / 2 + (n - M / 4)] = y[n], interleaved complex fp32; a row holds F M / 2 samples.
 *   5. timing    the output rate is M / N of the input rate; output sample u of a stream (counted from t0 = 0) sits at input sample
 *                (u + M / 4) N / M of the stream.  The first N / 4 input samples of a stream have no output, nor have the last N / 4 of
 *                its last frame.
 *   6. no stream a channel whose `stream` is outside 0 .. S - 1 gets a row of zero bytes.
 *   7. safety    whatever bytes d_channels holds, only rows of d_spectra inside the batch are read and only the channel's own row written.
 *   8. no state  there is no carry: a stream cut into calls, with t0 advanced by the frames already given, yields the same bytes as one
 *                call, and a call repeated yields the same bytes.
 * Exactness: step 1 is exact as written.  Step 2 is an fp32 radix-2 transform whose order is the implementation's; with u = 2^-24 every
 * sample is within gamma u (sum over i of |Z[i]|) / N of the exact value, gamma = 5 log2(M) + 4 (44 at M = 256): log2(M) butterfly
 * levels, each a rounded difference (u) and a product with a rounded factor ((1 + sqrt 2) u for the product, u / sqrt 2 for the
 * factor), rounded up to 5 u a level, and one more such product between the two passes.  The scale and the sign are exact.  A taper
 * of zeros gives zeros (of either sign).
 *   Limits       the taper's roll-off is the filter: what lies within its flat part comes out unchanged, what lies in the roll-off is
 *                weighted, and the time response of the roll-off must have died within N / 4 samples for the blocks to join.  With
 *                N = 1024, M = 64 and a flat part of +-16 bins an off-grid tone joins over 39 borders within 2.7e-4 of its amplitude;
 *                N = 4096, M = 256, flat +-96: 1.3e-5; N = 512, M = 16, flat +-4, a roll-off of 4 bins: 1.8e-2.  Choose M so that the
 *                roll-off has 16 bins or more.  All channels of a call share M and the taper.  No resampling to a symbol rate. */
typedef struct crn_extract_params {
  int32_t out_len;           /* M: 16, 32, 64, 128 or 256, and <= fft_len / 2 */
  int32_t frames_per_stream; /* F >= 1, divides n_frames */
  int32_t t0;                /* >= 0: frames of each stream given to earlier calls */
  int32_t reserved[5];       /* 0 */
} crn_extract_params; /* 32 bytes */
typedef struct crn_extract_channel {
  int32_t stream;            /* 0 .. S - 1; anything else: a row of zeros */
  int32_t centre;            /* bin; taken mod fft_len */
  int32_t reserved[2];       /* not looked at */
} crn_extract_channel; /* 16 bytes */

/* Enqueue the stage on `stream`, one launch (device pointers, all 16-byte aligned):
 *   d_spectra   [n_frames][fft_len] complex fp32              the spectra of half-overlapped frames
 *   d_channels  [n_chan]                                      the channel records
 *   d_taper     [out_len] fp32                                H
 *   d_out       [n_chan][frames_per_stream out_len / 2] complex fp32, every sample written
 * `h` supplies fft_len and the device, nothing else.  Only enqueues; allocates nothing, keeps no state, needs no workspace.  No atomics:
 * the same call repeated gives the same bytes.  CRN_ERR_ARG, decided before any device call, for a NULL h, params, d_spectra,
 * d_channels, d_taper or d_out; an out_len not in the list or above fft_len / 2; frames_per_stream < 1 or not dividing n_frames;
 * t0 < 0; n_chan outside 0 .. 65536; n_frames < 0; a nonzero reserved in params; any of the four arrays not 16-byte aligned.
 * n_frames = 0 or n_chan = 0 succeeds and launches nothing. */
CRN_API int crn_extract_device(crn_handle *h, const float *d_spectra, int64_t n_frames, const crn_extract_params *params,
                               const crn_extract_channel *d_channels, int32_t n_chan, const float *d_taper, float *d_out, void *stream);

/* -- resampling: an extracted stream at k samples per symbol -----------------------------------------------------------------------
 * The extraction's streams run at fs M / N, whatever the emitter's symbol rate, and keep the offset between the emitter and the whole
 * bin kappa.  This stage takes both away on the device: an arbitrary-ratio polyphase resampler with a fine mixer behind it.  The ratio
 * and the offset are per row and read from device memory, so that a later stage can write them; the carry from call to call lies in
 * the caller's device memory, as for the other stateful stages.
 * T = taps, one of 8, 16, 32.  P = phases, one of 32, 64, 128, 256; s = 32 - log2 P.  d_in is [n_rows][in_len] interleaved complex fp32
 * (the rows of crn_extract_device's d_out fit as they are); row r of the input is row r of d_rows, d_state and d_out.  d_taps is
 * [P + 1][T] fp32, the polyphase table h, supplied by the caller as the extraction's taper is.  A row record holds step, the input
 * samples per output sample in Q32.32 (rho = step / 2^32), and dphi, the mixer's increment per output sample in turns 2^32 (it wraps).
 * A row is LIVE when 2^30 <= step <= 2^34 (rho from 1/4 to 4); any other value gives a row of zero bytes and last_n_out = 0, and the
 * rest of its state stays as it was.  The state of a row is 320 bytes, a 64-byte head and hist[32] complex fp32; it is taken as EMPTY
 * (pos 0, phase 0, a history of zeros, counters 0) when `first` is set or when its `taps` is not the call's T; a negative counter is
 * read as 0.  No index is ever formed from a state's bytes except through pos, which enters the arithmetic of steps 1 and 6 only.
 * For a live row, L = in_len 2^32, and x[i] for i < 0 is the history, x[i] = hist[T - 1 + i]:
 *   1. count     n = 0 if pos >= L, else floor((L - 1 - pos) / step) + 1: the outputs whose position falls inside this call's input.
 *                w = min(n, out_cap).
 *   2. position  for u = 0 .. w - 1: p = pos + u step (no overflow: p < L <= 2^56); j = p >> 32; f = p mod 2^32; phi = f >> s;
 *                mu = ((f mod 2^s) >> max(s - 24, 0)) 2^-min(s, 24), which fp32 holds exactly.
 *   3. filter    y = sum over k = 0 .. T - 1 of ((1 - mu) h[phi][k] + mu h[phi + 1][k]) x[j - k].  Causal: with h from the rule below the
 *                output sits T / 2 input samples behind position p.
 *   4. mixer     z = y e^(+j 2 pi theta / 2^32), theta = phase + u dphi mod 2^32.
 *   5. row       d_out[r][u] = z for u < w; every other sample of the row, up to out_cap, is zero bytes: every byte is written.
 *   6. carry     pos <- pos + n step - L (pos - L when n = 0); phase <- phase + n dphi; n_in += in_len; n_out += w; n_dropped += n - w;
 *                last_n_out = w; taps = T; hist <- the last T - 1 samples of (old history ++ this call's row), also for in_len < T - 1;
 *                hist[T - 1 .. 31] and the reserved words are written as 0.  pos and phase advance by n, not w: outputs that did not fit
 *                are lost, the stream's timing is not.
 *   7. safety    whatever bytes the rows and the states hold, only d_in rows inside the batch, the table and the row's own state are
 *                read, and only the row's own output and state written.
 *   8. cutting   a row fed in one call, and the same row cut into calls of any lengths, give the same output samples bit for bit
 *                (concatenated over last_n_out) and the same final state byte for byte (last_n_out apart, which speaks of the last call
 *                alone); so does the same call repeated from the same state.  The arithmetic of one output therefore does not depend
 *                on where the call begins: the history and the row are read through one path, and the sum over k runs in one order.
 * Exactness: steps 1, 2, 5 and 6 are integers and exact.  For steps 3 and 4, with u = 2^-24, every output is within
 * gamma u sum over k of max(|h[phi][k]|, |h[phi + 1][k]|) |x[j - k]| of the exact value, gamma = T + 12: 3 u for the interpolated
 * coefficient (a rounded difference and one fma, mu exact), T u for the T-term sum, 5.7 u for the mixer factor (each component within
 * 4 u of exact) and 2.4 u for the complex product.  theta is an integer, so its reduction to a quadrant is exact; what is left has 29
 * bits and a sign, which fp32 holds to 0.8 u in the angle.
 *   Table        crnsense.resample_taps(taps, phases, cutoff, beta), in float64, rounded once: h[phi][k] = g(k - T / 2 + phi / P) for
 *                phi = 0 .. P, g(t) = 2 fc sinc(2 fc t) I0(beta sqrt(1 - (2 t / T)^2)) / I0(beta) for |t| < T / 2 and 0 beyond, fc =
 *                cutoff in cycles per input sample, the whole scaled once so that rows 0 .. P - 1 sum to P (unit gain at 0).
 *   Limits       the filter is short.  16 taps have a transition band of about +-0.16 cycles per sample around the cutoff (8 taps
 *                +-0.18, 32 taps +-0.10): the signal must lie that far inside `cutoff`, and for rho > 1 `cutoff` must lie that far
 *                inside 0.5 / rho.  With T 16, P 128, beta 8, cutoff 0.40 tones out to 0.22 come out within 1.1e-4 of their amplitude
 *                sum, tones at 0.30 are 2 % off.  rho within 1/4 .. 4.  One table per call: rows of very different rho want separate
 *                calls.  The delay is T / 2 input samples.  No timing recovery, no matched filter. */
typedef struct crn_resample_params {
  int32_t in_len;            /* 1 .. 2^24 samples of a row */
  int32_t out_cap;           /* 1 .. 2^26 samples of an output row */
  int32_t taps;              /* T: 8, 16 or 32 */
  int32_t phases;            /* P: 32, 64, 128 or 256 */
  int32_t first;             /* != 0: the states' contents mean nothing, start afresh */
  int32_t reserved[3];       /* 0 */
} crn_resample_params; /* 32 bytes */
typedef struct crn_resample_row {
  uint64_t step;             /* input samples per output sample, Q32.32; live in 2^30 .. 2^34 */
  int32_t dphi;              /* mixer increment per output sample, turns 2^32 */
  int32_t reserved;          /* not looked at */
} crn_resample_row; /* 16 bytes */
typedef struct crn_resample_state {
  uint64_t pos;              /* Q32.32 position of the next output, relative to the first sample of the next call's input */
  uint32_t phase;            /* mixer phase, turns 2^32 */
  int32_t taps;              /* the T this history belongs to */
  int64_t n_in;              /* input samples taken so far */
  int64_t n_out;             /* output samples produced so far */
  int64_t n_dropped;         /* outputs that did not fit */
  int32_t last_n_out;        /* outputs written by the last call */
  int32_t reserved[5];       /* written as 0 */
  float hist[64];            /* hist[32] complex: the last T - 1 input samples in [0 .. T - 2], the rest written as 0 */
} crn_resample_state; /* 320 bytes */

/* Bytes of n_rows states: 320 n_rows, -1 for n_rows outside 0 .. 65536.  Needs no handle and no device. */
CRN_API int64_t crn_resample_state_bytes(int64_t n_rows);

/* Enqueue the stage on `stream`, two launches (device pointers, all 16-byte aligned):
 *   d_in     [n_rows][in_len] complex fp32
 *   d_rows   [n_rows]                        the row records
 *   d_taps   [phases + 1][taps] fp32         h
 *   d_state  [n_rows]                        the states: read (unless first != 0), then rewritten by the second launch
 *   d_out    [n_rows][out_cap] complex fp32, every sample written
 * `h` supplies the device only.  Only enqueues; allocates nothing, needs no workspace.  No atomics: the same call from the same state
 * gives the same bytes.  CRN_ERR_ARG, decided before any device call, for a NULL h, params, d_in, d_rows, d_taps, d_state or d_out;
 * taps or phases not in the list; in_len outside 1 .. 2^24; out_cap outside 1 .. 2^26; n_rows outside 0 .. 65536; a nonzero reserved
 * in params; any of the five arrays not 16-byte aligned.  n_rows = 0 succeeds and launches nothing. */
CRN_API int crn_resample_device(crn_handle *h, const float *d_in, int32_t n_rows, const crn_resample_params *params,
                                const crn_resample_row *d_rows, const float *d_taps, crn_resample_state *d_state, float *d_out,
                                void *stream);

/* Allocate, now, the device scratch and pinned staging that crn_sense_run_host needs for up to
 * max_epochs dense epochs of full-length frames (and their per-bin spectra when want_spectrum != 0),
 * and load the kernels: a later crn_sense_run_host within that size allocates nothing.  An engine
 * calls this from its constructor so that no allocation ever runs inside execute(), where CE_mutex
 * is held (src/extensible_cognitive_radio.cpp:1792-1803). */
CRN_API int crn_sense_reserve_host(crn_handle *h, int64_t max_epochs, int32_t want_spectrum);

/* -- ingest ring: the rx-worker side of the boundary --------------------------------------------
 * The ECR's rx worker hands the engine one USRP packet at a time (memcpy into ce_usrp_rx_buffer +
 * condition signal, src/extensible_cognitive_radio.cpp:1310-1324) and the engine must return
 * quickly because CE_mutex is held (:1792-1803).  The ring coalesces packets of many streams into
 * K-packet epochs — each packet is copied once, straight into its place in a pinned batch buffer —
 * ships batches to the GPU asynchronously on a private stream (H2D -> kernel -> D2H, two buffers)
 * and hands decisions back through a non-blocking poll.  crn_ingest_push and crn_ingest_poll never
 * wait for the GPU and never allocate: `execute()` only copies one packet and checks an event.
 * The ring owns a launcher thread that makes every HIP call (it calls crn_sense_run_device on the
 * handle: do not use crn_sense_run_host / crn_sense_reserve_host on that handle from another
 * thread while batches are in flight; crn_sense_run_device is safe to call concurrently).
 * Environment, read at creation: $CRN_INGEST_ZEROCOPY_BYTES (524288: batches up to this size are read from and written to the
 * pinned buffers by the kernel itself, no copies), $CRN_INGEST_SPIN_US (150: how long after a small batch's hand-off the launcher
 * polls its event before sleeping), $CRN_INGEST_PREWAKE_US (600; 0 = off: ten packets before a small batch's hand-off the pushing
 * thread tells the launcher — one condition-variable signal, no wait — and the launcher polls for the work for at most this long
 * instead of sleeping: a sleeping thread comes back tens of microseconds late; when the ring's stream has sat idle for more than
 * 2 ms the launcher also queues one empty launch at that moment — the HIP calls of the first launch on an idle queue take several
 * times longer than back to back, and this way the empty one pays for it; $CRN_INGEST_WARM_GPU=0 leaves it out), $CRN_INGEST_TRACE (1: crn_ingest_destroy prints to
 * stderr where the hand-off-to-results time went: the launcher's wake-up, the HIP calls, device time + noticing the event). */
typedef struct crn_ingest crn_ingest;

typedef struct crn_epoch_result {
  int32_t stream;                    /* as given to crn_ingest_push                         */
  int32_t decision;                  /* crn_out.decision                                    */
  int64_t epoch_seq;                 /* 0, 1, 2, .. per stream                              */
  double ann_out[3];                 /* DECIDE_ANN only                                     */
  float features[CRN_MAX_BANDS];
  uint8_t occupancy[CRN_MAX_BANDS];
  int32_t flags;                     /* CRN_EPOCH_* bits                                    */
  float noise_floor;                 /* the estimate the epoch's thresholds came from (crn_ingest_calibrate); 0 without one */
} crn_epoch_result;
/* The epoch was launched while a calibration was collecting, or before the thresholds it produced were in place: its features are
 * measurements, its decision / occupancy were taken against the thresholds of before — not to be acted on. */
#define CRN_EPOCH_CALIBRATION 1

/* samples_per_packet: L of every pushed packet (1..fft_len) — also the largest
 * L crn_ingest_set_packet_len may select later (buffers are sized for it here, once).
 * Disjoint frames (hop == fft_len, the reference's shape): a packet is a frame, zero-padded to fft_len by the kernel; K packets
 * make an epoch.  Overlapped frames (hop < fft_len, the Welch plans): the packets of an epoch are consecutive pieces of ONE
 * contiguous run of samples, ceil(((K - 1) hop + fft_len) / L) of them (crn_ingest_packets_per_epoch), from which the kernel
 * cuts its K overlapped frames.
 * epochs_per_batch: completed epochs that trigger a launch.  All device, pinned and host memory the
 * ring will ever use is allocated by this call. */
CRN_API int crn_ingest_create(crn_handle *h, int32_t n_streams, int32_t samples_per_packet,
                              int32_t epochs_per_batch, crn_ingest **out);
/* Threshold plans whose thresholds are lambda x a measured noise floor (the scan engine's start-up): the next
 * n_epochs epochs that come back only feed the estimate — crn_noise_floor_device's median of medians over their features — and with
 * the last of them the ring's launcher thread uploads them, reduces them and puts lambda x the estimate in as every band's
 * threshold, ordered on the ring's stream.  Every epoch launched before that update comes out of crn_ingest_poll marked
 * CRN_EPOCH_CALIBRATION; the first unmarked one carries the estimate in `noise_floor`.  The call itself only posts the request
 * (no HIP call, no allocation: the buffers were made by crn_ingest_create), so an engine may issue it from execute();
 * CRN_ERR_STATE while an earlier request is still collecting, or on a handle that does not decide by thresholds. */
CRN_API int crn_ingest_calibrate(crn_ingest *g, int32_t n_epochs, float lambda);
/* The estimate in force (0 before the first calibration has finished) and whether one is collecting now.  Never blocks. */
CRN_API int crn_ingest_noise_floor(crn_ingest *g, float *nf_out, int32_t *calibrating);
/* Packets of a different length (<= the creation length) from now on: the rx worker learns the UHD
 * packet size only when it starts (src/extensible_cognitive_radio.cpp:1263-1265), after the engine
 * was constructed.  CRN_ERR_STATE while epochs are staged. */
CRN_API int crn_ingest_set_packet_len(crn_ingest *g, int32_t samples_per_packet);
/* Copy one packet of stream `stream` (L interleaved complex samples) into its epoch's pinned slot;
 * the K-th packet of the last missing epoch of a batch also enqueues the batch.  Never blocks: when
 * both batch buffers are on the GPU the packet is refused with CRN_ERR_BUSY (counted by
 * crn_ingest_dropped) — the caller may drop it, as the reference's hand-off does with frames the CE
 * thread is not ready for, or call crn_ingest_wait and push again. */
CRN_API int crn_ingest_push(crn_ingest *g, int32_t stream, const float *iq_packet);
/* Launch the completed epochs staged so far, even if fewer than epochs_per_batch (may wait for the
 * older batch when open epochs have to move to the other buffer). */
CRN_API int crn_ingest_flush(crn_ingest *g);
/* Block until the buffer being filled is free again (back-pressure for callers that must not drop). */
CRN_API int crn_ingest_wait(crn_ingest *g);
/* Non-blocking: results of finished batches, oldest first.  *n_out <= max_results. */
CRN_API int crn_ingest_poll(crn_ingest *g, crn_epoch_result *out, int32_t max_results, int32_t *n_out);
/* flush + wait for everything in flight (results stay queued for crn_ingest_poll). */
CRN_API int crn_ingest_drain(crn_ingest *g);
/* Packets that complete an epoch at the current packet length: K for disjoint frames, see crn_ingest_create for overlapped ones. */
CRN_API int crn_ingest_packets_per_epoch(crn_ingest *g, int32_t *n_packets);
/* Packets refused with CRN_ERR_BUSY so far (a caller that waits and pushes again has each such packet counted once per refusal). */
CRN_API int crn_ingest_dropped(crn_ingest *g, int64_t *n_packets);
/* Counters of a ring since its creation (the operational view the reference has only as printf lines: SURVEY.md §8b proposed
 * `crn_sense_stats`).  Never blocks; call from the thread that pushes. */
typedef struct crn_ingest_stats {
  int64_t packets;           /* packets accepted */
  int64_t dropped;           /* packets refused with CRN_ERR_BUSY */
  int64_t batches;           /* launches (H2D + kernel + D2H) handed to the GPU */
  int64_t batches_failed;    /* launches that failed (their epochs are lost; the error is reported once by the next call) */
  int64_t epochs_launched;   /* epochs those batches carried */
  int64_t epochs_ready;      /* epochs whose results came back */
  int64_t epochs_polled;     /* of which crn_ingest_poll has handed out */
  double latency_us_sum;     /* per batch: hand-off by the pushing thread -> results readable, summed over `batches` that came back */
  double latency_us_max;
} crn_ingest_stats;
CRN_API int crn_ingest_get_stats(crn_ingest *g, crn_ingest_stats *out);
CRN_API int crn_ingest_destroy(crn_ingest *g);

/* -- multi-GPU: the occupancy exchange ----------------------------------------------------------
 * The path shards by stream: every (stream, epoch) is independent — the only state that crosses
 * frames is the K-frame mean inside one epoch of one stream (fft_avg[], CE_Predictive_Node.hpp:51) —
 * so each GPU (one process per GPU, one crn_handle each) runs crn_sense_run_device on its own
 * streams' batch with no data-path collective.  The one exchange: every node's engine needs the whole
 * occupancy picture to pick a free channel, so each rank contributes its [epochs][n_bands] uint8
 * block to an all-gather over RCCL (xGMI inside a node).  Latency-bound (KiB per rank): one
 * collective per batch, queued on a side stream behind an event so that it overlaps the next launch;
 * `depth` slots so that step i + 1's kernel can write while step i's gather is in flight.
 *
 *   rank 0: crn_comm_unique_id(id), handed to the other ranks out of band (any launcher's store)
 *   all:    crn_comm_create(device, rank, world, id, epochs * n_bands, 2, &c)        (collective)
 *   step i: crn_comm_local(c, i, stream, &occ)   -> crn_out.occupancy = occ; crn_sense_run_device(.., stream)
 *           crn_comm_allgather(c, i, stream)     -> returns at once; the gather runs on the side stream
 *           ... crn_comm_gathered(c, i, &all)    valid once `stream` has passed crn_comm_finish / the
 *                                                crn_comm_local of step i + depth
 * RCCL is loaded at run time by crn_comm_unique_id / crn_comm_create — librccl.so.1, or exactly the library $CRN_RCCL_LIB names
 * (if that does not load the calls fail: no other RCCL is tried) — so single-GPU users of libcrnsense do not need it. */
typedef struct crn_comm crn_comm;
#define CRN_COMM_ID_BYTES 128   /* sizeof(ncclUniqueId) */

CRN_API int crn_comm_unique_id(uint8_t id[CRN_COMM_ID_BYTES]);
/* Collective over all `world` ranks (blocks until every rank has called it).  Allocates, once, the
 * `depth` local and gathered slots on `device` and a private side stream.  Like ncclCommInitRank itself it cannot tell the
 * other ranks about a local failure: if this call fails on one rank (bad argument, no memory, RCCL missing) the others stay
 * inside the collective, so the launcher must take the job down — torch.distributed.run does; a caller with a control
 * plane of its own should first agree that every rank can load RCCL (crn_comm_unique_id into a scratch id is a
 * non-collective probe: bench.py / sharding.py do exactly that). */
CRN_API int crn_comm_create(int32_t device, int32_t rank, int32_t world, const uint8_t id[CRN_COMM_ID_BYTES],
                            int64_t bytes_per_rank, int32_t depth, crn_comm **out);
/* What the communicator is, asked of RCCL itself (ncclCommCount / ncclCommUserRank / ncclCommCuDevice / ncclGetVersion on the
 * communicator crn_comm_create built — not an echo of its arguments), so that a caller can state, and a reader of its output can
 * check, that the collective really spans `nranks` ranks on `nranks` different GPUs: bench.py puts every rank's answer into its N > 1
 * JSON line and refuses to report a real-RCCL run whose ranks do not name N distinct PCI devices.  Fields RCCL cannot answer (a library
 * without the query) read -1.  Not collective; never blocks. */
typedef struct crn_comm_info_t {
  int32_t nranks;         /* ncclCommCount */
  int32_t rank;           /* ncclCommUserRank */
  int32_t rccl_device;    /* ncclCommCuDevice: the HIP device RCCL bound this rank to */
  int32_t rccl_version;   /* ncclGetVersion (e.g. 22203) */
  int32_t device;         /* the device crn_comm_create was given */
  int32_t depth;
  int64_t bytes_per_rank;
  int64_t gathers;        /* all-gathers queued through crn_comm_allgather so far */
  char library[128];      /* the name the RCCL library was loaded under (librccl.so.1, or $CRN_RCCL_LIB) */
  char pci_bus_id[32];    /* hipDeviceGetPCIBusId of rccl_device (of `device` when RCCL cannot say): "0000:05:00.0" — the physical GPU, whatever
                             ordinal a launcher's device isolation gave it in this process (ABI version 4) */
} crn_comm_info_t;
CRN_API int crn_comm_info(crn_comm *c, crn_comm_info_t *out);
/* Device address of the block step `step` writes (slot step % depth).  If that slot's previous gather
 * is still in flight, `stream` is made to wait for it (on the device; the host does not block). */
CRN_API int crn_comm_local(crn_comm *c, int64_t step, void *stream, uint8_t **d_local);
/* The same address without touching the slot's state or any stream (for reading the block back, say). */
CRN_API int crn_comm_local_addr(crn_comm *c, int64_t step, uint8_t **d_local);
/* Queue the all-gather of step `step`'s block behind everything enqueued on `stream` so far.  Only enqueues. */
CRN_API int crn_comm_allgather(crn_comm *c, int64_t step, void *stream);
/* Device address of step `step`'s gathered vector, [world][bytes_per_rank], rank order. */
CRN_API int crn_comm_gathered(crn_comm *c, int64_t step, const uint8_t **d_all);
/* Make `stream` wait for step `step`'s gather alone (work queued on `stream` after the call may read crn_comm_gathered(step)).
 * The slot stays marked in flight: whichever stream later takes it through crn_comm_local, or calls crn_comm_finish, still waits. */
CRN_API int crn_comm_wait(crn_comm *c, int64_t step, void *stream);
/* Make `stream` wait for every gather queued so far (call before the final synchronise). */
CRN_API int crn_comm_finish(crn_comm *c, void *stream);
CRN_API int crn_comm_destroy(crn_comm *c);

/* -- the transform on its own ------------------------------------------------------------------
 * Unnormalised forward DFT X[k] = sum_n x[n] exp(-j 2 pi k n / N) (the contract of liquid-dsp's
 * fft_execute with LIQUID_FFT_FORWARD, CE_Predictive_Node.cpp:42-45,150) of n_frames frames:
 * frame i takes samples_per_frame (<= fft_len, zero-padded) interleaved complex fp32 samples starting
 * frame_stride samples (0 = samples_per_frame) after frame i-1, and yields fft_len complex bins at
 * d_out + 2 * fft_len * i.  Same passes as the sensing kernel, complex output instead of the fused
 * accumulate.  include/crn_liquid_fft.h puts liquid's three entry points on top of this. */
CRN_API int crn_fft_forward_device(crn_handle *h, const float *d_in, int64_t n_frames, int32_t samples_per_frame,
                                   int64_t frame_stride, float *d_out, void *stream);

/* -- monitor rows -----------------------------------------------------------
 * The display side of the reference's GNU Radio monitor — qtgui.freq_sink_c(fft_size 1024,
 * firdes.WIN_BLACKMAN_hARRIS), set_fft_average(0.1), and the waterfall sink (spectrum_analyzer.py:262-275) —
 * over rows of the `spectrum` output of crn_sense_run_device (window CRN_WINDOW_BLACKMAN_HARRIS, mode
 * CRN_MODE_ENERGY; frames_per_epoch frames per row, 1 for the sink's one-FFT-per-update):
 *   d_waterfall_db[r][j]  10 log10(P_r[(j + N/2) mod N] / norm)         fftshifted, like the sinks draw it
 *   d_average_db[r][j]    the single-pole IIR over rows, a = alpha:  y <- (1 - a) y + a x
 *   d_state[j]            the IIR state, carried between calls (first != 0: seeded with row 0)
 * CRN_MONITOR_GNURADIO: norm = N^2 and the IIR runs on the dB values (gr-qtgui 3.7 freq_sink_c_impl.cc: volk
 *   power_spectral_density then d_magbuf = (1 - a) d_magbuf + a new — GNU Radio is third-party and absent from
 *   the reference tree; this is its published algorithm).
 * CRN_MONITOR_PSD: norm = N * sum(w^2) and the IIR runs on linear power (a Welch-style averaged PSD), dB after. */
typedef enum crn_monitor_kind { CRN_MONITOR_GNURADIO = 0, CRN_MONITOR_PSD = 1 } crn_monitor_kind;
CRN_API int crn_monitor_rows_device(crn_handle *h, const float *d_spectrum, int64_t n_rows, int32_t kind, float alpha,
                                    int32_t first, float *d_state, float *d_waterfall_db, float *d_average_db, void *stream);

/* -- training -------------------------------------------------------------
 * The reference ships weights for one FFT size and one receiver gain (CE_Predictive_Node.cpp:78-120)
 * and no way to make others.  crn_ann_train_device fits the same 4-5-3 sigmoid network
 * (CE_Predictive_Node.hpp:20-22,62-73) to labelled features that are already on the device — e.g.
 * the `features` output of crn_sense_run_device over crn_synth_fill_device traffic with its d_truth —
 * by full-batch backpropagation (squared error, momentum), `restarts` independent initialisations in
 * parallel (one workgroup each), and returns the best in the reference's array layout, ready for
 * crn_cfg.ann_w_ih / ann_w_ho.  With `normalise`, feature i is scaled by 1/mean_i during training and
 * the gains are folded back into W_IH, so inference stays exactly the reference's forward pass. */
typedef struct crn_train_cfg {
  uint64_t seed;
  int32_t iterations;  /* gradient steps */
  int32_t restarts;    /* >= 1 */
  float eta;           /* learning rate */
  float alpha;         /* momentum */
  int32_t normalise;   /* 0 / 1 */
  int32_t reserved;
} crn_train_cfg;

/* d_features: [n][4] float32 in ANN input order {NOISE_FLOOR, CH1, CH2, CH3}; d_labels: [n] int32,
 * 0 = no channel occupied, k = channel k.  w_ih / w_ho / final_loss are host pointers.  Blocking. */
CRN_API int crn_ann_train_device(crn_handle *h, const crn_train_cfg *tc, const float *d_features,
                                 const int32_t *d_labels, int64_t n, double w_ih[5][6], double w_ho[6][4],
                                 double *final_loss, void *stream);

/* -- measurement / test aids ------------------------------------------------------------- */

/* Fill d_iq with n_epochs * samples_per_epoch seeded synthetic samples on the device:
 * complex AWGN with E|x|^2 = noise_power, plus — for the band the per-epoch occupancy pattern
 * selects (a seeded uniform pick among {none, band 1, .., band n_active}, mirroring the PU of
 * cognitive_engines/CE_Random_Behaviour_PU/CE_Random_Behaviour_PU.cpp:41-53) — tones_per_band
 * on-grid tones of total RMS amplitude signal_rms.  d_truth (nullable) receives the picked band
 * per epoch (0 = none).  The FFT grid is the handle's fft_len; "active" bands are the handle's
 * bands 1..min(3, n_bands-1) (for Welch cfgs: all bands, pick in 0..n_bands). */
CRN_API int crn_synth_fill_device(crn_handle *h, float *d_iq, int64_t n_epochs,
                          int64_t samples_per_epoch, uint64_t seed, float noise_power,
                          float signal_rms, int32_t tones_per_band, int32_t *d_truth,
                          void *stream);

/* Traffic models of the driven primary user (which band an epoch's signal occupies):
 *  CRN_PU_UNIFORM           seeded uniform pick among {idle, band 1 .. band n_active}, independent per
 *                           epoch — cognitive_engines/CE_Random_Behaviour_PU/CE_Random_Behaviour_PU.cpp:41-53
 *                           (rand() % 3 over the channels) plus an idle state.
 *  CRN_PU_MARKOV_AS_WRITTEN the chain of CE_PU_MARKOV_Chain_Tx.cpp:88-128 exactly as its conditions
 *                           evaluate: outcome = rand() % 10; 0 -> CH1, anything else -> CH2 (the
 *                           `>= 1 || < 4` tests are always true), CH3 unreachable, never idle.
 *  CRN_PU_MARKOV_INTENDED   the same chain with the thresholds its comments intend (`&&`): from
 *                           CH1/CH3: 0 -> CH1, 1..3 -> CH2, 4..9 -> CH3; from CH2: 0 -> CH1,
 *                           1..5 -> CH2, 6..9 -> CH3.  Never idle.
 *  CRN_PU_SWEEP            the interferer's TX_FREQ_BEHAVIOR_SWEEP (src/interferer.cpp:339-345: step up by one
 *                           resolution per dwell, reverse at either end) with one band per epoch:
 *                           1, 2, .., n_active, n_active - 1, .., 1, 2, ..  Never idle.
 * Markov and sweep models run per stream: the batch is n_streams consecutive runs of n_epochs / n_streams
 * epochs, each started in CH1 (the Markov chains independent; d_truth is required for them). */
typedef enum crn_pu_model { CRN_PU_UNIFORM = 0, CRN_PU_MARKOV_AS_WRITTEN = 1, CRN_PU_MARKOV_INTENDED = 2, CRN_PU_SWEEP = 3 } crn_pu_model;

/* What the occupied band carries (src/interferer.cpp:128-140 CW / NOISE, :160-215 GMSK, :221-248 RRC, :254-282 OFDM):
 *  CRN_SIG_TONES      tones_per_band on-grid tones spread over the band, fixed random phases per epoch
 *  CRN_SIG_CW         one carrier at the band's centre bin
 *  CRN_SIG_BAND_NOISE every bin of the band, fresh random phases every fft_len samples (a
 *                     frame-synchronous multicarrier burst: flat in-band spectrum)
 * The three below are continuous modulated carriers at the band's centre frequency (midway between its lowest and
 * highest bin, bins >= fft_len / 2 counted as negative frequencies), NOT aligned to the FFT grid or to frames (they
 * leak like a real transmitter); "band width" is the band's number of bins:
 *  CRN_SIG_RRC_QPSK   random QPSK symbols through a root-raised-cosine pulse, roll-off 0.35 (RRC_BETA,
 *                     include/interferer.hpp:21), truncated at +-8 symbols; symbol rate such that the occupied
 *                     bandwidth (1 + beta) Rs is the band's width
 *  CRN_SIG_GMSK       constant-envelope GMSK, BT = 0.5, modulation index 1/2 (the gmskframegen the interferer
 *                     drives); symbol rate = band width / 1.5 (>= 99.9 % of the power inside the band)
 *  CRN_SIG_OFDM       QPSK subcarriers 15 kHz apart at the 13 MHz sample rate of CE_Predictive_Node.hpp:42-43
 *                     (the interferer's tx_rate / num_subcarriers, src/interferer.cpp:255), i.e.
 *                     fft_len * 15e3 / 13e6 bins, filling the band; cyclic prefix 1/4 of the useful symbol, no taper
 * All kinds have total power signal_rms^2. */
typedef enum crn_signal_kind {
  CRN_SIG_TONES = 0, CRN_SIG_CW = 1, CRN_SIG_BAND_NOISE = 2, CRN_SIG_RRC_QPSK = 3, CRN_SIG_GMSK = 4, CRN_SIG_OFDM = 5
} crn_signal_kind;

typedef struct crn_synth_cfg {
  uint64_t seed;
  float noise_power;      /* E|x|^2 of the complex AWGN */
  float signal_rms;       /* RMS amplitude of the PU signal */
  int32_t tones_per_band; /* CRN_SIG_TONES only */
  int32_t pu_model;       /* crn_pu_model */
  int32_t signal_kind;    /* crn_signal_kind */
  int32_t n_streams;      /* >= 1; must divide n_epochs for the Markov models */
  int32_t adc_bits;       /* 0: full fp32 samples.  2..24: every component rounded to a multiple of 2^-(adc_bits - 1) and clipped to
                           * [-1, 1): what a radio delivers — the reference's USRPs send 16-bit integers over the wire (4 bytes per
                           * complex sample: the 363-364 samples of a 1500-byte packet, src/extensible_cognitive_radio.cpp:1263-1265),
                           * which UHD converts to the complex floats of recv(.., COMPLEX_FLOAT32, ..) (:1071-1072) with a constant
                           * of its own (1/32767: the values then are not on this power-of-two grid) */
} crn_synth_cfg;

/* crn_synth_fill_device with a traffic model and a signal kind.  crn_synth_fill_device(.., seed,
 * noise_power, signal_rms, tones, ..) == this with {CRN_PU_UNIFORM, CRN_SIG_TONES, n_streams 1}. */
CRN_API int crn_synth_fill_device_ex(crn_handle *h, const crn_synth_cfg *sc, float *d_iq, int64_t n_epochs,
                                     int64_t samples_per_epoch, int32_t *d_truth, void *stream);

/* Noise-floor estimate for threshold plans (thr_b = lambda x NF_est, NF_est = the median band energy): the
 * median over epochs of every epoch's median band energy, from a features matrix [n_epochs][n_bands] on the device (what
 * crn_sense_run_device wrote; at most the first 4096 epochs are used).  "Median" = element (n - 1) / 2 of the sorted values.  With
 * fewer than half of the bands occupied the estimate does not see the signals.  Enqueues on `stream` and waits for the result. */
CRN_API int crn_noise_floor_device(crn_handle *h, const float *d_features, int64_t n_epochs, float *nf_out, void *stream);
/* Replace the per-band thresholds of a handle (cfg.thresh; CRN_DECIDE_THRESHOLD): ordered on `stream` — launches enqueued on it
 * after the call see the new values, launches before it the old ones.  `thresh` is read before the call returns (it is staged in
 * pinned memory of the handle's own, one slot per update: the asynchronous copy never reads memory a later call rewrites).
 * Updates (this call, crn_sense_set_ann, crn_sense_calibrate_thresholds) cannot be captured into a hipGraph — a replay would upload
 * whatever the reused staging slot holds by then: on a stream that is capturing they return CRN_ERR_STATE and enqueue nothing.
 * Launches capture fine.  With all eight staging slots still in flight an update waits for the oldest with the handle's lock released
 * (a launch on another thread never waits for an update's copy); if a crn_sense_set_bands on another thread changed the number of
 * bands (or the decision rule) in that window the update returns CRN_ERR_STATE and writes nothing. */
CRN_API int crn_sense_set_thresholds(crn_handle *h, const float *thresh, int32_t n_bands, void *stream);

/* Allocate, now, what crn_noise_floor_host and crn_sense_calibrate_thresholds need (pinned + device upload buffers for 4096 epochs
 * of CRN_MAX_BANDS features, the reduction scratch): after it neither allocates.  An engine calls it from its constructor. */
CRN_API int crn_sense_reserve_noise_floor(crn_handle *h);
/* Calibration in one call, for callers that hold the features on the host (the engine's synchronous form; the ingest ring's launcher
 * thread): upload features [n_epochs][n_bands] (n_epochs <= 4096), crn_noise_floor_device, then every band's threshold = lambda x
 * the estimate, set on `stream` like crn_sense_set_thresholds.  Blocks for the reduction; allocates nothing (CRN_ERR_STATE unless
 * crn_sense_reserve_noise_floor ran). */
CRN_API int crn_sense_calibrate_thresholds(crn_handle *h, const float *features, int64_t n_epochs, float lambda, float *nf_out, void *stream);
/* The same estimate from a features matrix in host memory (an engine that keeps no device buffers of its own): uploaded, then
 * crn_noise_floor_device.  Blocking; not for the packet path.  Allocates its upload buffers on the first call unless
 * crn_sense_reserve_noise_floor did. */
CRN_API int crn_noise_floor_host(crn_handle *h, const float *features, int64_t n_epochs, float *nf_out);
/* Replace the network of a DECIDE_ANN handle (cfg.ann_w_ih / ann_w_ho / ann_threshold; the reference has its weights as
 * literals, CE_Predictive_Node.cpp:78-120): ordered on `stream` like crn_sense_set_thresholds.  The threshold rides in the launch
 * parameters: launches made after the call use it. */
CRN_API int crn_sense_set_ann(crn_handle *h, const double w_ih[5][6], const double w_ho[6][4], double threshold, void *stream);
/* Replace the band plan of a live handle (cfg.segs / n_segs / n_bands; the reference's is the five loops of
 * CE_Predictive_Node.cpp:173-191).  thresh: n_bands new thresholds, or NULL to keep the current ones (then n_bands must not
 * change).  Same validation as crn_sense_create.  Every table derived from the plan is rebuilt into a fresh allocation and the
 * call waits for launches in flight on the device before it frees the old one: not for the packet path.  Safe against an attached
 * ingest ring's launcher thread: the swap and the release of the old tables happen under the handle's lock, which every launch
 * holds from its first read of the plan until its kernel is enqueued.  Ingest rings size their result buffers for the n_bands they
 * were created with: a call that changes n_bands is refused (CRN_ERR_STATE) while one is attached. */
CRN_API int crn_sense_set_bands(crn_handle *h, const crn_band_seg *segs, int32_t n_segs, int32_t n_bands, const float *thresh);

/* Wait until everything queued on `stream` (NULL = the default stream) of the handle's device has completed: for callers that are
 * pure host code against this ABI (the engine) and need an asynchronous update to have landed before they go on. */
CRN_API int crn_sense_synchronize(crn_handle *h, void *stream);

/* Counters of a sensing handle since its creation.  `samples` counts every input sample a launch covers once (8 bytes each: the
 * algorithmic read of the path), so samples * 8 / kernel seconds is the same figure bench.py's roofline reports.  Durations are
 * measured only while crn_sense_set_timing(h, 1) is in effect (two HIP events per launch on the launch stream, a ring of 16 pairs;
 * leave it off while capturing launches into a hipGraph); crn_sense_get_stats collects those that have finished and never blocks. */
typedef struct crn_sense_stats {
  int64_t launches;          /* crn_sense_run_device calls that launched (run_host and the ingest ring go through it) */
  int64_t epochs;
  int64_t samples;
  int64_t timed_launches;    /* launches whose duration is in kernel_ms */
  double kernel_ms;          /* sum of their durations */
  double kernel_ms_last;
  double kernel_ms_min, kernel_ms_max;
} crn_sense_stats;
CRN_API int crn_sense_set_timing(crn_handle *h, int32_t on);
CRN_API int crn_sense_get_stats(crn_handle *h, crn_sense_stats *out);

/* Launches of a few epochs — up to one per compute unit; the engine's launch is ONE — at fft_len 512 / 1024 (any window, disjoint or
 * overlapped frames) run the sensing kernel in its dealt-frame form: one epoch per workgroup, its frames_per_epoch frames spread over the workgroup's lane
 * groups (8 at 512 points, 4 at 1024) instead of run one after the other by one of them, the K-frame accumulate replayed in frame
 * order afterwards: the same operations in the same order, so every output is bit for bit what the streaming form gives, in about
 * ceil(K / groups) frame latencies instead of K.  Chosen per launch from n_epochs; *n = how many launches of this handle RAN that
 * form (a launch the device refused the dealt form's LDS for runs the streaming form and is not counted).  (crn_sense_set_variant 400 / 401 / 402: automatic / never / at any batch size — for measurements and the equality test.) */
CRN_API int crn_sense_dealt_launches(crn_handle *h, int64_t *n);

/* Name, registers and LDS of the sensing kernel selected for this handle. */
CRN_API int crn_sense_kernel_info(crn_handle *h, char *name, int32_t name_len, int32_t *threads_per_block,
                          int32_t *lds_bytes, int32_t *epochs_per_block);

/* Which form of the sensing kernel a handle launches (set before running).  The shipped library carries the forms that are sensing
 * results: 0 (= 13) the default; 2 without the pruning of pass 3 to the registers the reference channel plan reaches (what any band
 * table outside that plan runs anyway); 23 every twiddle in registers at three workgroups per CU.  100 + n / 200 + n / 300 + n
 * override the launch geometry (epochs per big workgroup; x 256 epochs in tail workgroups; epochs per tail workgroup) and change
 * no result.  The measurement forms (7, 17, 19-22, 26, 27: the same flags in other combinations, and a build with in-kernel time
 * stamps) are compiled only into libcrnsense_ab.so (make -C csrc ab) and refused here with CRN_ERR_ARG; every other number is refused
 * by both. */
CRN_API int crn_sense_set_variant(crn_handle *h, int32_t variant);

/* (Optional, not in this library: samples kept in the radio's wire format, int16 pairs — include/crn_sense_sc16.h, libcrnsense_sc16.so.) */

CRN_API const char *crn_last_error(void);
CRN_API int crn_abi_version(void);
/* Toolchain contract.  built_hip: HIP_VERSION of the headers the library was compiled with (major * 10^7 + minor * 10^5 + patch);
 * runtime_hip: what hipRuntimeGetVersion reports on this machine (0 when no runtime answers).  The library links libamdhip64.so.<major>
 * and carries a gfx950 code object only: it runs on any ROCm whose HIP runtime has the SAME MAJOR version as built_hip and is not
 * older than ROCm 7.0 (the first release with gfx950).  Returns CRN_OK when that holds, CRN_ERR_STATE (with the two versions in
 * crn_last_error) when it does not.  Either pointer may be NULL. */
CRN_API int crn_build_info(int32_t *built_hip, int32_t *runtime_hip);

#ifdef __cplusplus
}
#endif
#endif /* CRN_SENSE_H */
