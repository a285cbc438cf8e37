// crn_handle.h — struct crn_handle and what the host translation units that implement the C ABI on it share (internal: csrc/ only).
#ifndef CRN_HANDLE_H
#define CRN_HANDLE_H
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>

#include "crn_internal.h"

struct crn_handle {
  explicit crn_handle(int dev) : device(dev) {}
  // The HIP device, fixed at creation: what every entry point makes current, readable without a lock (cfg.device is the same number,
  // but cfg as a whole is rewritten under tables_mu by crn_sense_set_bands while an ingest ring's launcher thread may be in here).
  const int device;
  crn_cfg cfg;
  int variant = 0;
  int groups_per_wg = 0;        // 0 = automatic
  int64_t tail_groups = -1;     // < 0 = automatic; epoch groups handed to the short tail workgroups at the end
  int tail_groups_per_wg = 0;   // 0 = automatic; epoch groups per tail workgroup
  std::atomic<int64_t> n_dealt{0};   // launches that ran the dealt-frame kernel (crn_sense_dealt_launches)
  int64_t deal_max_epochs = -1; // launches of up to this many epochs run the dealt-frame kernel where it exists (< 0: automatic, from n_cus)
  int n_row_entries = 0;        // > 0: the band plan qualifies for register-resident band sums
  int aligned_shift = 0;        // N = 4096, equal contiguous bands of 64 / 128 / 256 bins in order: log2 of the width
  std::atomic<int> n_rings{0};  // ingest rings created on this handle (they size their result buffers for cfg.n_bands)
  int n_cus = 256;              // compute units of the device (workgroup slots = n_cus x workgroups per CU): read at creation
  size_t lds_budget = 64 * 1024;   // LDS a workgroup may ask for on this device (hipDeviceAttributeMaxSharedMemoryPerBlock: 160 KiB on gfx950)
  unsigned acc_mask = 0xFFFFu;  // accumulator registers (bit j R3 + d) that hold a bin of some band (N = 4096: the 256-bin rows)
  // the plan as the plain 4096-point kernels see it (register rows 7 bins early: crn_kernels.h, bin_of): their row entries and mask
  int n_row_entries_shift = 0;
  unsigned acc_mask_shift = 0xFFFFu;
  bool cfar_on = false;         // crn_sense_set_cfar[_ex]: per-bin CFAR decides instead of the cfg's rule (under tables_mu)
  crn_cfar_params_ex cfar{};    // the detector last set (crn_sense_set_cfar: method CA, rank 0)
  // one device slab holding every table
  void *d_tables = nullptr;
  const float2 *d_tw1 = nullptr, *d_tw2 = nullptr;
  const float *d_window = nullptr, *d_thresh = nullptr;
  const int *d_band_seg_begin = nullptr, *d_seg_lo = nullptr, *d_seg_hi = nullptr;
  const int *d_band_bins_begin = nullptr, *d_band_bins = nullptr, *d_band_tab = nullptr, *d_band_c2 = nullptr, *d_row_entries_shift = nullptr;
  const double *d_wih = nullptr, *d_who = nullptr;
  // scratch of crn_sense_run_host
  void *d_scratch = nullptr;
  size_t scratch_bytes = 0;
  double window_power = 0.0;   // sum of the squared fp32 window values (crn_monitor_rows_device)
  double wire_full_scale = 32768.0;   // crn_sense_set_wire_full_scale
  float *d_nf_scratch = nullptr;   // crn_noise_floor_device: per-epoch medians + the result
  void *h_small = nullptr;     // pinned in-place buffer of run_host's small batches (samples | results)
  size_t h_small_bytes = 0;
  void *h_results = nullptr;   // pinned staging for the per-epoch results of run_host (one D2H)
  size_t h_results_bytes = 0;
  // Live updates against launches from other threads (an ingest ring's launcher thread calls run_device_impl while the thread that
  // owns the handle calls crn_sense_set_bands / _set_thresholds / _set_ann): `tables_mu` covers cfg, every table pointer and the
  // plan-derived fields above.  A launch holds it from the first read of cfg until the kernel is enqueued, an update from its
  // first write until its copies are enqueued (set_bands: until the old slab is freed) — so a launch sees one plan, whole, and no
  // launch can pick up a slab after the update that frees it has started.
  std::mutex tables_mu;
  // The noise-floor scratch and upload buffers (d_nf_scratch, h_nf_features, d_nf_features) and the blocking reductions that use them:
  // a lock of their own, so that a calibration waiting for the device never holds tables_mu — launches on other threads go on.
  // Order: nf_mu before tables_mu.
  std::mutex nf_mu;
  // Pinned staging of the small asynchronous updates (thresholds, weights): hipMemcpyAsync reads its source when the stream gets
  // there, so each update copies from a slot of its own that is not rewritten until the event behind its copies has completed.
  struct UpdateSlot {
    float thresh[CRN_MAX_BANDS];
    double w_ih[CRN_ANN_IN + 1][CRN_ANN_HID + 1];
    double w_ho[CRN_ANN_HID + 1][CRN_ANN_OUT + 1];
  };
  static constexpr int kUpdateSlots = 8;
  UpdateSlot *upd = nullptr;                 // pinned [kUpdateSlots]
  hipEvent_t upd_done[kUpdateSlots] = {};
  bool upd_used[kUpdateSlots] = {};
  int64_t upd_next = 0;
  float *h_nf_features = nullptr;            // pinned upload buffer of crn_noise_floor_host (crn_sense_reserve_noise_floor)
  float *d_nf_features = nullptr;
  // counters (crn_sense_get_stats): launches come from the caller's thread or from an ingest ring's launcher thread
  std::atomic<int64_t> n_launches{0}, n_epochs{0}, n_samples{0};
  std::mutex timing_mu;        // everything below
  bool timing = false;
  static constexpr int kTimedSlots = 16;
  hipEvent_t t_start[kTimedSlots] = {}, t_stop[kTimedSlots] = {};
  int64_t t_issued = 0, t_collected = 0, t_dropped = 0;   // slots [t_collected, t_issued) are in flight (mod kTimedSlots)
  double kernel_ms = 0.0, kernel_ms_last = 0.0, kernel_ms_min = 0.0, kernel_ms_max = 0.0;
};

namespace crn {
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// crn_tables.cpp: the rules of crn_sense_create on a configuration, and everything a handle keeps in HBM for one
int validate(const crn_cfg *c);
int build_tables(crn_handle *h, const crn_cfg &next);
}  // namespace crn
#endif
