// crn_updates.cpp — changes to a live handle (thresholds, ANN weights, the band plan) against launches from other threads, and the
// noise-floor estimate that calibrates the thresholds.  (The entry points take their C linkage from include/crn_sense.h.)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "crn_handle.h"
#include "crn_kernels.h"

namespace {
// Updates copy from pinned staging with hipMemcpyAsync and mark their slot with an event; a stream that is being captured into a
// hipGraph would record both into the graph, where the event never completes for the host and every replay would upload whatever the
// slot holds by then.  Refused: make the update outside the capture (launches capture fine: tests/test_graph.py).
int refuse_capture(hipStream_t st, const char *what) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (st != nullptr && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return crn::fail(CRN_ERR_STATE, std::string(what) + ": the stream is being captured into a hipGraph; updates cannot be captured (their pinned "
                                                       "staging slot is reused) — make them outside the capture");
  return CRN_OK;
}

// A pinned staging slot whose last copy has completed (`lk` = tables_mu, held).  Normally the first one tried; when all eight are still in
// flight the lock is RELEASED while this thread waits for the oldest — a launch on another thread never waits for an update's copy.
// *waited says that happened: whatever the caller checked under the lock before (the number of bands, the decision rule) may have been
// changed by a crn_sense_set_bands on another thread in that window, and the caller checks it again before it writes anything.
// (The event waited for may be re-recorded by another updater meanwhile: the wait is only a hint, the loop queries every slot afresh.)
int take_update_slot(crn_handle *h, std::unique_lock<std::mutex> &lk, int *slot, bool *waited) {
  *waited = false;
  for (;;) {
    for (int k = 0; k < crn_handle::kUpdateSlots; k++) {
      const int i = (int)((h->upd_next + k) % crn_handle::kUpdateSlots);
      if (h->upd_used[i]) {
        const hipError_t q = hipEventQuery(h->upd_done[i]);
        if (q == hipErrorNotReady) continue;
        if (q != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("hipEventQuery(update slot): ") + hipGetErrorString(q));
      }
      h->upd_used[i] = true;
      h->upd_next = i + 1;
      *slot = i;
      return CRN_OK;
    }
    const hipEvent_t oldest = h->upd_done[h->upd_next % crn_handle::kUpdateSlots];
    lk.unlock();
    const hipError_t e = hipEventSynchronize(oldest);
    lk.lock();
    *waited = true;
    if (e != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("hipEventSynchronize(update slot): ") + hipGetErrorString(e));
  }
}

// The reduction + its read-back (nf_mu held, tables_mu NOT held: the wait stalls nobody's launch).
int noise_floor_run(crn_handle *h, const float *d_features, int64_t n_epochs, int n_bands, float *nf_out, hipStream_t st) {
  if (!h->d_nf_scratch) HIP_TRY(hipMalloc(&h->d_nf_scratch, (crn::kNoiseFloorMaxEpochs + 1) * sizeof(float)));
  const int n = (int)std::min<int64_t>(n_epochs, crn::kNoiseFloorMaxEpochs);
  HIP_TRY(crn::launch_noise_floor(d_features, n, n_bands, h->d_nf_scratch, st));
  HIP_TRY(hipMemcpyAsync(nf_out, h->d_nf_scratch + crn::kNoiseFloorMaxEpochs, sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CRN_OK;
}

int bands_of(crn_handle *h) {
  std::lock_guard<std::mutex> lk(h->tables_mu);
  return h->cfg.n_bands;
}

int set_thresholds_locked(crn_handle *h, std::unique_lock<std::mutex> &lk, const float *thresh, int32_t n_bands, hipStream_t st) {
  int slot = 0;
  bool waited = false;
  if (int rc = take_update_slot(h, lk, &slot, &waited)) return rc;
  // (the slot taken stays marked used with its last, completed, event: the next update takes it)
  if (waited && n_bands != h->cfg.n_bands)
    return crn::fail(CRN_ERR_STATE, "the band plan changed while this update waited for a staging slot: nothing was written (set the thresholds of the new plan)");
  std::memcpy(h->cfg.thresh, thresh, sizeof(float) * (size_t)n_bands);
  float *src = h->upd[slot].thresh;
  std::memcpy(src, h->cfg.thresh, sizeof(float) * CRN_MAX_BANDS);
  // the two device copies the kernels read: the table and the packed band table's threshold words (layout: crn_kernels.h)
  HIP_TRY(hipMemcpyAsync(const_cast<float *>(h->d_thresh), src, sizeof(float) * CRN_MAX_BANDS, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(const_cast<int *>(h->d_band_tab) + crn::kTabThresh, src, sizeof(float) * CRN_MAX_BANDS, hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(h->upd_done[slot], st));
  return CRN_OK;
}
}  // namespace

int crn_noise_floor_device(crn_handle *h, const float *d_features, int64_t n_epochs, float *nf_out, void *stream) {
  if (!h || !d_features || !nf_out) return crn::fail(CRN_ERR_ARG, "null handle / features / result");
  if (n_epochs < 1) return crn::fail(CRN_ERR_ARG, "n_epochs < 1");
  std::lock_guard<std::mutex> nf(h->nf_mu);
  HIP_TRY(hipSetDevice(h->device));
  return noise_floor_run(h, d_features, n_epochs, bands_of(h), nf_out, static_cast<hipStream_t>(stream));
}

int crn_sense_reserve_noise_floor(crn_handle *h) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> nf(h->nf_mu);
  HIP_TRY(hipSetDevice(h->device));
  const size_t bytes = (size_t)crn::kNoiseFloorMaxEpochs * CRN_MAX_BANDS * sizeof(float);   // any band plan the handle may get later
  if (!h->d_nf_scratch) HIP_TRY(hipMalloc(&h->d_nf_scratch, (crn::kNoiseFloorMaxEpochs + 1) * sizeof(float)));
  if (!h->h_nf_features) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h->h_nf_features), bytes, hipHostMallocDefault));
  if (!h->d_nf_features) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&h->d_nf_features), bytes));
  return CRN_OK;
}

int crn_sense_set_thresholds(crn_handle *h, const float *thresh, int32_t n_bands, void *stream) {
  if (!h || !thresh) return crn::fail(CRN_ERR_ARG, "null handle / thresholds");
  if (int rc = refuse_capture(static_cast<hipStream_t>(stream), "crn_sense_set_thresholds")) return rc;
  std::unique_lock<std::mutex> lk(h->tables_mu);
  if (n_bands != h->cfg.n_bands) return crn::fail(CRN_ERR_ARG, "n_bands differs from the handle's");
  HIP_TRY(hipSetDevice(h->device));
  return set_thresholds_locked(h, lk, thresh, n_bands, static_cast<hipStream_t>(stream));
}

int crn_sense_calibrate_thresholds(crn_handle *h, const float *features, int64_t n_epochs, float lambda, float *nf_out, void *stream) {
  if (!h || !features || !nf_out) return crn::fail(CRN_ERR_ARG, "null handle / features / result");
  if (n_epochs < 1 || n_epochs > crn::kNoiseFloorMaxEpochs) return crn::fail(CRN_ERR_ARG, "n_epochs must be in 1..4096");
  if (!(lambda > 0.f)) return crn::fail(CRN_ERR_ARG, "lambda must be positive");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = refuse_capture(st, "crn_sense_calibrate_thresholds")) return rc;
  int n_bands = 0;
  {
    // upload + reduction + the wait for its result under the noise-floor buffers' own lock: launches on other threads (an ingest ring's
    // launcher calls this between batches; the owner of the handle may be launching) are not held up by a stream drain
    std::lock_guard<std::mutex> nf(h->nf_mu);
    if (!h->h_nf_features || !h->d_nf_features || !h->d_nf_scratch)
      return crn::fail(CRN_ERR_STATE, "crn_sense_calibrate_thresholds: call crn_sense_reserve_noise_floor first (this call allocates nothing)");
    HIP_TRY(hipSetDevice(h->device));
    n_bands = bands_of(h);
    const size_t bytes = (size_t)n_epochs * n_bands * sizeof(float);
    std::memcpy(h->h_nf_features, features, bytes);
    HIP_TRY(hipMemcpyAsync(h->d_nf_features, h->h_nf_features, bytes, hipMemcpyHostToDevice, st));
    if (int rc = noise_floor_run(h, h->d_nf_features, n_epochs, n_bands, nf_out, st)) return rc;
  }
  float thr[CRN_MAX_BANDS];
  for (int b = 0; b < n_bands; b++) thr[b] = lambda * *nf_out;
  std::unique_lock<std::mutex> lk(h->tables_mu);
  if (n_bands != h->cfg.n_bands) return crn::fail(CRN_ERR_STATE, "crn_sense_calibrate_thresholds: the band plan changed while the noise floor was being estimated");
  return set_thresholds_locked(h, lk, thr, n_bands, st);
}

int crn_sense_set_ann(crn_handle *h, const double w_ih[5][6], const double w_ho[6][4], double threshold, void *stream) {
  if (!h || !w_ih || !w_ho) return crn::fail(CRN_ERR_ARG, "null handle / weights");
  if (int rc = refuse_capture(static_cast<hipStream_t>(stream), "crn_sense_set_ann")) return rc;
  std::unique_lock<std::mutex> lk(h->tables_mu);
  if (h->cfg.decide != CRN_DECIDE_ANN) return crn::fail(CRN_ERR_STATE, "crn_sense_set_ann: the handle does not decide with the network");
  if (!(threshold > 0.0 && threshold < 1.0)) return crn::fail(CRN_ERR_ARG, "threshold must be in (0, 1)");
  for (int i = 0; i < 5; i++)
    for (int j = 0; j < 6; j++)
      if (!std::isfinite(w_ih[i][j])) return crn::fail(CRN_ERR_ARG, "non-finite weight");
  for (int j = 0; j < 6; j++)
    for (int k = 0; k < 4; k++)
      if (!std::isfinite(w_ho[j][k])) return crn::fail(CRN_ERR_ARG, "non-finite weight");
  HIP_TRY(hipSetDevice(h->device));
  int slot = 0;
  bool waited = false;
  if (int rc = take_update_slot(h, lk, &slot, &waited)) return rc;
  if (waited && h->cfg.decide != CRN_DECIDE_ANN)
    return crn::fail(CRN_ERR_STATE, "crn_sense_set_ann: the handle's plan changed while this update waited for a staging slot: nothing was written");
  std::memcpy(h->cfg.ann_w_ih, w_ih, sizeof(h->cfg.ann_w_ih));
  std::memcpy(h->cfg.ann_w_ho, w_ho, sizeof(h->cfg.ann_w_ho));
  h->cfg.ann_threshold = threshold;   // rides in the launch parameters
  crn_handle::UpdateSlot &u = h->upd[slot];
  std::memcpy(u.w_ih, w_ih, sizeof(u.w_ih));
  std::memcpy(u.w_ho, w_ho, sizeof(u.w_ho));
  // the device copies the kernels read: the two tables and the packed band table's weight words (layout: crn_kernels.h)
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(const_cast<double *>(h->d_wih), u.w_ih, sizeof(u.w_ih), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(const_cast<double *>(h->d_who), u.w_ho, sizeof(u.w_ho), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(const_cast<int *>(h->d_band_tab) + crn::kTabWih, u.w_ih, sizeof(u.w_ih), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(const_cast<int *>(h->d_band_tab) + crn::kTabWho, u.w_ho, sizeof(u.w_ho), hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(h->upd_done[slot], st));
  return CRN_OK;
}

int crn_sense_set_bands(crn_handle *h, const crn_band_seg *segs, int32_t n_segs, int32_t n_bands, const float *thresh) {
  if (!h || !segs) return crn::fail(CRN_ERR_ARG, "null handle / segments");
  if (n_segs < 1 || n_segs > CRN_MAX_SEGS) return crn::fail(CRN_ERR_ARG, "n_segs out of range");
  // held across the rebuild AND the release of the old slab: a launch on another thread (an ingest ring's launcher) either was
  // enqueued before — hipFree inside build_tables waits for it — or starts after, with the new plan, whole
  std::lock_guard<std::mutex> lk(h->tables_mu);
  crn_cfg next = h->cfg;
  next.n_segs = n_segs;
  next.n_bands = n_bands;
  std::memcpy(next.segs, segs, sizeof(crn_band_seg) * (size_t)n_segs);
  if (thresh) {
    if (n_bands >= 1 && n_bands <= CRN_MAX_BANDS) std::memcpy(next.thresh, thresh, sizeof(float) * (size_t)n_bands);
  } else if (n_bands != h->cfg.n_bands) {
    return crn::fail(CRN_ERR_ARG, "crn_sense_set_bands: a different number of bands needs its thresholds");
  }
  if (int rc = crn::validate(&next)) return rc;   // same rules as crn_sense_create (DECIDE_ANN keeps its 4 bands, ref_band stays inside)
  if (n_bands != h->cfg.n_bands && h->n_rings.load(std::memory_order_acquire) > 0)
    return crn::fail(CRN_ERR_STATE, "crn_sense_set_bands: an ingest ring on this handle was sized for the current number of bands "
                                    "(destroy it, change the plan, create it again)");
  HIP_TRY(hipSetDevice(h->device));
  return crn::build_tables(h, next);   // a fresh slab; the old one is freed once the device is idle; on failure the old plan stays
}

int crn_noise_floor_host(crn_handle *h, const float *features, int64_t n_epochs, float *nf_out) {
  if (!h || !features || !nf_out) return crn::fail(CRN_ERR_ARG, "null handle / features / result");
  if (n_epochs < 1) return crn::fail(CRN_ERR_ARG, "n_epochs < 1");
  if (int rc = crn_sense_reserve_noise_floor(h)) return rc;   // allocates on the first call only
  std::lock_guard<std::mutex> nf(h->nf_mu);
  HIP_TRY(hipSetDevice(h->device));
  const int n_bands = bands_of(h);
  const int64_t n = std::min<int64_t>(n_epochs, crn::kNoiseFloorMaxEpochs);
  const size_t bytes = (size_t)n * n_bands * sizeof(float);
  std::memcpy(h->h_nf_features, features, bytes);
  HIP_TRY(hipMemcpyAsync(h->d_nf_features, h->h_nf_features, bytes, hipMemcpyHostToDevice, nullptr));
  return noise_floor_run(h, h->d_nf_features, n, n_bands, nf_out, nullptr);
}
