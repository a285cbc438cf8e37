// crn_api.cpp — the C ABI of libcrnsense (include/crn_sense.h): the handle's life, launches, counters.  Beside it: crn_tables.cpp (the
// device tables), crn_updates.cpp (live updates, noise floor), crn_cfar.cpp (the CFAR detector), crn_api_sc16.cpp (wire-format input).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "crn_forms.h"
#include "crn_handle.h"
#include "crn_segments.h"

namespace crn {
static thread_local std::string g_err;
int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
}  // namespace crn

// crn_segments_device (crn_segments.hip) reads nothing else of a handle
void crn::handle_geometry(crn_handle *h, int *fft_len, int *device) {
  std::lock_guard<std::mutex> lk(h->tables_mu);
  *fft_len = h->cfg.fft_len;
  *device = h->device;
}

using crn::align_up;
constexpr size_t kInPlaceBytes = 512 * 1024;   // run_host batches up to this size are read and written in place by the kernel

extern "C" {

const char *crn_last_error(void) { return crn::g_err.c_str(); }
int crn_abi_version(void) { return CRN_ABI_VERSION; }

int crn_build_info(int32_t *built_hip, int32_t *runtime_hip) {
  const int built = HIP_VERSION;   // hip/hip_version.h of the toolchain that compiled this file
  int rt = 0;
  if (hipRuntimeGetVersion(&rt) != hipSuccess) rt = 0;
  if (built_hip) *built_hip = built;
  if (runtime_hip) *runtime_hip = rt;
  if (rt == 0) return crn::fail(CRN_ERR_STATE, "crn_build_info: no HIP runtime answers");
  if (rt / 10000000 != built / 10000000 || rt < 70000000)
    return crn::fail(CRN_ERR_STATE, "libcrnsense was built with HIP " + std::to_string(built) + " and needs a HIP runtime of the same major "
                                    "version, ROCm 7.0 or newer (gfx950); this machine's reports " + std::to_string(rt));
  return CRN_OK;
}

int crn_sense_create(const crn_cfg *cfg, crn_handle **out) {
  if (!out) return crn::fail(CRN_ERR_ARG, "crn_sense_create: null out");
  *out = nullptr;
  if (int rc = crn::validate(cfg)) return rc;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev < 1) return crn::fail(CRN_ERR_DEVICE, "no HIP device visible (libcrnsense has no CPU path)");
  if (cfg->device < 0 || cfg->device >= ndev) return crn::fail(CRN_ERR_ARG, "cfg.device out of range");
  HIP_TRY(hipSetDevice(cfg->device));

  crn_handle *h = new (std::nothrow) crn_handle(cfg->device);
  if (!h) return crn::fail(CRN_ERR_NOMEM, "out of host memory");
  {
    int cus = 0, lds = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0) h->n_cus = cus;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg->device) == hipSuccess && lds > 0) h->lds_budget = (size_t)lds;
  }
  if (int rc = crn::build_tables(h, *cfg)) {
    delete h;
    return rc;
  }
  hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&h->upd), sizeof(crn_handle::UpdateSlot) * crn_handle::kUpdateSlots, hipHostMallocDefault);
  for (int i = 0; i < crn_handle::kUpdateSlots && e == hipSuccess; i++) e = hipEventCreateWithFlags(&h->upd_done[i], hipEventDisableTiming);
  if (e != hipSuccess) {
    (void)crn_sense_destroy(h);
    return crn::fail(CRN_ERR_NOMEM, std::string("crn_sense_create(update staging): ") + hipGetErrorString(e));
  }
  *out = h;
  return CRN_OK;
}

int crn_sense_destroy(crn_handle *h) {
  if (!h) return CRN_OK;
  // a ring's launcher thread launches through this handle and crn_ingest_destroy detaches from it: rings go first
  if (h->n_rings.load(std::memory_order_acquire) > 0)
    return crn::fail(CRN_ERR_STATE, "crn_sense_destroy: " + std::to_string(h->n_rings.load()) + " ingest ring(s) are still attached to this "
                                    "handle (crn_ingest_destroy them first)");
  (void)hipSetDevice(h->device);
  if (h->upd) (void)hipHostFree(h->upd);
  for (int i = 0; i < crn_handle::kUpdateSlots; i++)
    if (h->upd_done[i]) (void)hipEventDestroy(h->upd_done[i]);
  if (h->h_nf_features) (void)hipHostFree(h->h_nf_features);
  if (h->d_nf_features) (void)hipFree(h->d_nf_features);
  if (h->d_scratch) (void)hipFree(h->d_scratch);
  if (h->h_results) (void)hipHostFree(h->h_results);
  if (h->h_small) (void)hipHostFree(h->h_small);
  if (h->d_tables) (void)hipFree(h->d_tables);
  if (h->d_nf_scratch) (void)hipFree(h->d_nf_scratch);
  for (int i = 0; i < crn_handle::kTimedSlots; i++) {
    if (h->t_start[i]) (void)hipEventDestroy(h->t_start[i]);
    if (h->t_stop[i]) (void)hipEventDestroy(h->t_stop[i]);
  }
  delete h;
  return CRN_OK;
}

// internal (crn_ingest.cpp): a ring attaches to / detaches from its handle
int crn_sense_ring_count(crn_handle *h, int delta) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  if (delta > 0) {   // attaching: refused on a CFAR handle, checked and claimed under the lock crn_sense_set_cfar holds
    std::lock_guard<std::mutex> lk(h->tables_mu);
    if (h->cfar_on)
      return crn::fail(CRN_ERR_ARG, "crn_ingest_create: a ring on a CFAR handle is not supported yet (crn_epoch_result has no room for "
                                    "the bin mask)");
    h->n_rings.fetch_add(delta, std::memory_order_acq_rel);
    return CRN_OK;
  }
  h->n_rings.fetch_add(delta, std::memory_order_acq_rel);
  return CRN_OK;
}

// internal (crn_ingest.cpp): an empty launch on the ring's stream, queued at the pre-wake of a batch that follows an idle stretch —
// the HIP calls of the first launch on a queue that sat idle for 100 ms take 20 us instead of 5 (tools/engine_idle_gap.py)
int crn_sense_warm_stream(crn_handle *h, void *stream) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  HIP_TRY(hipSetDevice(h->device));   // (the launcher thread, at every pre-wake: no lock, nothing of cfg)
  HIP_TRY(crn::launch_nop(static_cast<hipStream_t>(stream)));
  return CRN_OK;
}

// internal (crn_ingest.cpp): the configuration a handle was created with
int crn_sense_cfg_of(crn_handle *h, crn_cfg *out) {
  if (!h || !out) return crn::fail(CRN_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->tables_mu);
  *out = h->cfg;
  return CRN_OK;
}

int crn_sense_dealt_launches(crn_handle *h, int64_t *n) {
  if (!h || !n) return crn::fail(CRN_ERR_ARG, "null handle / counter");
  *n = h->n_dealt.load(std::memory_order_relaxed);
  return CRN_OK;
}

int crn_sense_set_variant(crn_handle *h, int32_t variant) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->tables_mu);
  if (variant >= 100 && variant <= 164) {  // A/B: 100 + n = n epoch groups per workgroup (100 = automatic)
    h->groups_per_wg = variant - 100;
    return CRN_OK;
  }
  if (variant >= 200 && variant <= 264) {  // A/B: 200 + n = n x 256 epoch groups in the short tail workgroups
    h->tail_groups = (int64_t)(variant - 200) * 256;
    return CRN_OK;
  }
  if (variant >= 300 && variant <= 364) {  // A/B: 300 + n = n epoch groups per tail workgroup (300 = automatic)
    h->tail_groups_per_wg = variant - 300;
    return CRN_OK;
  }
  if (variant >= 400 && variant <= 402) {  // A/B: the dealt-frame kernel of small launches: 400 automatic, 401 never, 402 at any batch size
    h->deal_max_epochs = variant == 400 ? -1 : variant == 401 ? 0 : (int64_t)0x7fffffff;
    return CRN_OK;
  }
  if (variant < 0 || variant > crn::sense_num_variants()) return crn::fail(CRN_ERR_ARG, "variant out of range");
  if (!crn::sense_variant_available(variant))
    return crn::fail(CRN_ERR_ARG, "variant " + std::to_string(variant) + " is not a form of this library: the measurement variants (7, 17, 19-22, 26, 27) "
                                  "are compiled into libcrnsense_ab.so (make -C csrc ab), not into the shipped library; any other number names "
                                  "a form that no longer exists");
  h->variant = variant;
  return CRN_OK;
}

// What select_form needs to know of the handle's band plan, window and CFAR state: the same for a launch and for crn_sense_kernel_info.
static void fill_plan_facts(const crn_handle *h, bool spectrum, crn::SenseParams &p) {
  p.hann_sym = h->cfg.window == CRN_WINDOW_HANN;
  p.aligned_shift = spectrum ? 0 : h->aligned_shift;
  p.acc_mask = h->variant == 2 ? 0xFFFFu : h->acc_mask;   // variant 2: no pruning at any size
  p.n_row_entries = h->n_row_entries;
  p.n_row_entries_shift = h->n_row_entries_shift;
  p.acc_mask_shift = h->variant == 2 ? 0xFFFFu : h->acc_mask_shift;
  p.cfar_on = h->cfar_on ? 1 : 0;
}

int crn_sense_kernel_info(crn_handle *h, char *name, int32_t name_len, int32_t *threads_per_block,
                          int32_t *lds_bytes, int32_t *epochs_per_block) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->tables_mu);
  // the form a streaming launch of whole frames without a spectrum output runs (a spectrum request falls back to full rows / the LDS close)
  crn::SenseParams p{};
  p.L = h->cfg.fft_len;
  fill_plan_facts(h, false, p);
  const std::optional<crn::FormKey> k = crn::select_form(
      crn::make_form_query(p, h->cfg.fft_len, h->cfg.mode == CRN_MODE_REF_MAG, h->cfg.window != CRN_WINDOW_RECT, h->variant, false));
  if (!k) return crn::fail(CRN_ERR_STATE, "no kernel form for this handle");
  const crn::FormGeometry g = crn::form_geometry(*k);
  if (threads_per_block) *threads_per_block = g.threads;
  if (lds_bytes) *lds_bytes = g.lds_bytes;
  if (epochs_per_block) *epochs_per_block = g.epochs_per_block;
  if (name && name_len > 0) crn::form_name(*k, name, (size_t)name_len);
  return CRN_OK;
}

static int resolve_strides(const crn_handle *h, int32_t L, int64_t *epoch_stride, int *frame_stride) {
  const crn_cfg &c = h->cfg;
  if (L < 1 || L > c.fft_len)
    return crn::fail(CRN_ERR_ARG, "samples_per_frame must be in 1..fft_len (the reference's unchecked memcpy, "
                                   "CE_Predictive_Node.cpp:149, is rejected here)");
  if (c.hop != c.fft_len && L != c.fft_len)
    return crn::fail(CRN_ERR_ARG, "overlapped frames (hop < fft_len) need samples_per_frame == fft_len");
  *frame_stride = c.hop == c.fft_len ? L : c.hop;
  if (*epoch_stride <= 0) *epoch_stride = (int64_t)c.frames_per_epoch * *frame_stride;
  return CRN_OK;
}

// Collect the durations of timed launches that have finished (timing_mu held); `wait`: also the one occupying slot `must_free`.
static void collect_timings(crn_handle *h, bool wait_oldest) {
  while (h->t_collected < h->t_issued) {
    const int s = (int)(h->t_collected % crn_handle::kTimedSlots);
    hipError_t q = hipEventQuery(h->t_stop[s]);
    if (q == hipErrorNotReady && wait_oldest) q = hipEventSynchronize(h->t_stop[s]);
    wait_oldest = false;
    if (q == hipErrorNotReady) break;
    float ms = 0.f;
    if (q == hipSuccess && hipEventElapsedTime(&ms, h->t_start[s], h->t_stop[s]) == hipSuccess) {
      const int64_t n = h->t_collected - h->t_dropped;
      h->kernel_ms += ms;
      h->kernel_ms_last = ms;
      h->kernel_ms_min = n == 0 ? ms : std::min(h->kernel_ms_min, (double)ms);
      h->kernel_ms_max = n == 0 ? ms : std::max(h->kernel_ms_max, (double)ms);
    } else {
      h->t_dropped++;   // a launch that failed on the device: no duration
    }
    h->t_collected++;
  }
}

int crn_sense_set_timing(crn_handle *h, int32_t on) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  std::lock_guard<std::mutex> lk(h->timing_mu);
  if (on && !h->t_start[0]) {
    HIP_TRY(hipSetDevice(h->device));
    for (int i = 0; i < crn_handle::kTimedSlots; i++) {
      HIP_TRY(hipEventCreate(&h->t_start[i]));
      HIP_TRY(hipEventCreate(&h->t_stop[i]));
    }
  }
  h->timing = on != 0;
  return CRN_OK;
}

int crn_sense_get_stats(crn_handle *h, crn_sense_stats *out) {
  if (!h || !out) return crn::fail(CRN_ERR_ARG, "null handle / stats");
  std::lock_guard<std::mutex> lk(h->timing_mu);
  collect_timings(h, false);
  out->launches = h->n_launches.load(std::memory_order_relaxed);
  out->epochs = h->n_epochs.load(std::memory_order_relaxed);
  out->samples = h->n_samples.load(std::memory_order_relaxed);
  out->timed_launches = h->t_collected - h->t_dropped;
  out->kernel_ms = h->kernel_ms;
  out->kernel_ms_last = h->kernel_ms_last;
  out->kernel_ms_min = h->kernel_ms_min;
  out->kernel_ms_max = h->kernel_ms_max;
  return CRN_OK;
}

// How a launch of n_epochs is dealt to workgroups (tables_mu held): groups_per_wg, n_big_wgs and tail_groups_per_wg of `p`, for the
// plain streams and the Welch spans, with the A/B overrides of crn_sense_set_variant.
static void launch_geometry(const crn_handle *h, int64_t n_epochs, int64_t epoch_stride, crn::SenseParams &p) {
  const crn_cfg &c = h->cfg;
  // Several epoch groups per workgroup amortise its prologue (twiddles and tables loaded once, the next epoch's first frame in flight
  // across the close); the single-group workgroups at the end keep the drain short, so two rounds of big workgroups over the 256 CUs x 4
  // slots are enough (measured at N = 4096: +0.5-1.5 % on 2048 .. 12288-epoch batches over the earlier n_groups / 4096).
  const int groups = 256 / (c.fft_len / 16);
  const int64_t n_groups = (n_epochs + groups - 1) / groups;
  // workgroup slots of this device: CUs x workgroups per CU (4 for the plain kernels' register budget, 3 for the windowed ones)
  const int64_t slots4 = (int64_t)h->n_cus * 4, slots3 = (int64_t)h->n_cus * 3;
  int64_t epw = n_groups / (2 * slots4);
  epw = epw < 1 ? 1 : epw > 4 ? 4 : epw;
  // the last `tail` groups go to short workgroups (dispatched last): a short drain
  int64_t tail = slots4;      // one single-group workgroup per workgroup slot: +0.9 % at N = 4096
  int64_t tail_epw = 1;
  // The Welch stream (windowed, hop = N/2, dense epochs) reads one half-frame twice per workgroup span — a span's first half-frame is the
  // previous span's last — so its spans are made long: ~256 frames per big workgroup while at least ~2.7 rounds of them remain over the
  // 768 slots (3 workgroups per CU), a quarter of that per tail workgroup, one tail workgroup per slot.  At K = 8 that is 32 epochs /
  // 8 epochs / 6144 epochs: traffic 1.005 x the algorithmic bytes instead of 1.033 x with 4-epoch spans and a single-epoch tail, and
  // 1-2 % less time (profiles/r05_welch_spans.txt).
  if (c.window != CRN_WINDOW_RECT && c.hop * 2 == c.fft_len && epoch_stride == (int64_t)c.frames_per_epoch * c.hop) {
    const int64_t slots = slots3;
    epw = std::min<int64_t>(std::max<int64_t>(256 / c.frames_per_epoch, 1), n_groups * 3 / (8 * slots));   // >= 2.67 rounds of them
    epw = epw < 1 ? 1 : epw > 64 ? 64 : epw;
    tail_epw = epw / 4 < 1 ? 1 : epw / 4 > 8 ? 8 : epw / 4;
    tail = slots * tail_epw;
  }
  p.groups_per_wg = (int)(h->groups_per_wg > 0 ? h->groups_per_wg : epw);
  if (h->tail_groups >= 0) tail = h->tail_groups;
  if (tail > n_groups / 4) tail = n_groups / 4;
  p.tail_groups_per_wg = (int)(h->tail_groups_per_wg > 0 ? h->tail_groups_per_wg : tail_epw);
  p.n_big_wgs = (n_groups - tail) / p.groups_per_wg;
}

static int run_device_impl(crn_handle *h, const void *d_iq, int64_t n_epochs, int32_t samples_per_frame,
                           int64_t epoch_stride, const crn_out *d_out, void *stream, bool sc16,
                           uint32_t *d_cfar_mask = nullptr, int32_t *d_cfar_band_bins = nullptr, bool want_cfar = false) {
  if (!h || !d_out) return crn::fail(CRN_ERR_ARG, "null handle / outputs");
  if (n_epochs < 0) return crn::fail(CRN_ERR_ARG, "n_epochs < 0");
  if (n_epochs == 0) return CRN_OK;
  if (!d_iq) return crn::fail(CRN_ERR_ARG, "null IQ pointer");
  const int64_t sample_bytes = sc16 ? 4 : 8;
  if ((reinterpret_cast<uintptr_t>(d_iq) & (uintptr_t)(sample_bytes - 1)) != 0)
    return crn::fail(CRN_ERR_ARG, sc16 ? "IQ pointer must be 4-byte aligned" : "IQ pointer must be 8-byte aligned");
  // one plan, whole, from here until the kernel is enqueued (live updates from another thread wait; see crn_handle::tables_mu)
  std::lock_guard<std::mutex> tables_lk(h->tables_mu);
  if (want_cfar && !h->cfar_on) return crn::fail(CRN_ERR_STATE, "crn_sense_run_device_cfar: CFAR is off on this handle (crn_sense_set_cfar)");
  if (sc16 && h->cfar_on) return crn::fail(CRN_ERR_ARG, "CFAR on wire-format (sc16) samples is not supported yet");
  int frame_stride = 0;
  if (int rc = resolve_strides(h, samples_per_frame, &epoch_stride, &frame_stride)) return rc;
  if (n_epochs > (int64_t)0x7fffffff) return crn::fail(CRN_ERR_ARG, "n_epochs too large for one launch");
  HIP_TRY(hipSetDevice(h->device));  // a NULL stream / a launch follows the calling thread's current device
  // a workgroup addresses its window with 32-bit byte offsets
  if ((64 * epoch_stride + (int64_t)(h->cfg.frames_per_epoch + 1) * frame_stride + 2 * (int64_t)h->cfg.fft_len) * sample_bytes >= ((int64_t)1 << 31))
    return crn::fail(CRN_ERR_ARG, "epoch_stride too large (a workgroup window must stay below 2 GiB)");
  const crn_cfg &c = h->cfg;
  crn::SenseParams p{};
  p.iq = reinterpret_cast<const float2 *>(d_iq);   // int16 pairs when sc16: the kernel instantiation knows
  p.n_epochs = n_epochs;
  p.epoch_stride = epoch_stride;
  p.total_samples = (n_epochs - 1) * epoch_stride + (int64_t)(c.frames_per_epoch - 1) * frame_stride +
                    (c.hop == c.fft_len ? samples_per_frame : c.fft_len);
  p.frame_stride = frame_stride;
  p.L = samples_per_frame;
  p.K = c.frames_per_epoch;
  launch_geometry(h, n_epochs, epoch_stride, p);
  {
    // A launch of a few epochs (the engine's: one) leaves most of every workgroup idle in the streaming kernel — an epoch is one lane
    // group running its K frames one after the other.  Up to one epoch per compute unit the dealt-frame kernel spreads an epoch's
    // frames over the lane groups of a workgroup of its own instead (csrc/crn_sense_kernel.h: sense_kernel_dealt; same results bit
    // for bit).  Measured (profiles/r05_dealt_frames_ab.txt, us per launch, streaming -> dealt): 1 reference epoch 19.7 -> 10.0 from
    // HBM and 29.4 -> 15.4 from pinned host memory (the ring's launch); 256 epochs 20.3 -> 10.9; from 512 epochs on — two
    // workgroups per CU — the energy forms lose (17.5 -> 20.5), so the switch sits at one per CU.
    const int64_t deal_max = h->deal_max_epochs >= 0 ? h->deal_max_epochs : (int64_t)h->n_cus;
    // (a CFAR handle has no dealt form: the kCfar kernels stream)
    if (!h->cfar_on && n_epochs <= deal_max && (h->variant == 0 || h->variant == 13))
      p.deal_rounds = crn::sense_deal_rounds(c.fft_len, c.mode == CRN_MODE_REF_MAG, c.window != CRN_WINDOW_RECT,
                                             c.window == CRN_WINDOW_HANN && samples_per_frame == c.fft_len, c.frames_per_epoch, h->lds_budget);
  }
  p.tw1 = h->d_tw1;
  p.tw2 = h->d_tw2;
  p.window = h->d_window;
  p.band_tab = h->d_band_tab;
  p.band_seg_begin = h->d_band_seg_begin;
  p.seg_lo = h->d_seg_lo;
  p.seg_hi = h->d_seg_hi;
  p.thresh = h->d_thresh;
  p.ann_w_ih = h->d_wih;
  p.ann_w_ho = h->d_who;
  p.ann_threshold = c.ann_threshold;
  p.n_bands = c.n_bands;
  p.decide = c.decide;
  p.ref_band = c.ref_band;
  fill_plan_facts(h, d_out->spectrum != nullptr, p);
  {  // 1 / full scale for a sum of magnitudes, its square for energies (2^-15 / 2^-30 by default: exact)
    const double u = 1.0 / h->wire_full_scale;
    p.wire_unscale = (float)(c.mode == CRN_MODE_REF_MAG ? u : u * u);
  }
  p.row_entries_shift = h->d_row_entries_shift;
  p.features = d_out->features;
  // (a measurement form that writes time stamps puts them there: libcrnsense_ab.so only)
  p.ann_out = (c.decide == CRN_DECIDE_ANN || crn::sense_variant_traces(h->variant)) ? d_out->ann_out : nullptr;
  p.decision = d_out->decision;
  p.occupancy = d_out->occupancy;
  p.spectrum = d_out->spectrum;
  if (h->cfar_on) {
    p.cfar_guard = h->cfar.guard;
    p.cfar_train = h->cfar.train;
    p.cfar_min_bins = h->cfar.min_bins;
    // the scale on the K-frame sums: CA alpha / 2W on both sides' total, GO / SO alpha / W on one side's sum, OS alpha on one cell
    const double div = h->cfar.method == CRN_CFAR_CA ? 2.0 * h->cfar.train : h->cfar.method == CRN_CFAR_OS ? 1.0 : (double)h->cfar.train;
    p.cfar_scale = (float)((double)h->cfar.alpha / div);
    p.cfar_method = h->cfar.method;
    p.cfar_rank = h->cfar.rank;
    p.cfar_mask = d_cfar_mask;
    p.cfar_band_bins = d_cfar_band_bins;
  }
  int slot = -1;
  {
    std::lock_guard<std::mutex> lk(h->timing_mu);
    if (h->timing) {
      if (h->t_issued - h->t_collected == crn_handle::kTimedSlots) collect_timings(h, true);   // 16 launches behind: wait for the oldest
      slot = (int)(h->t_issued++ % crn_handle::kTimedSlots);
      HIP_TRY(hipEventRecord(h->t_start[slot], static_cast<hipStream_t>(stream)));
    }
  }
  int deal_rounds_run = 0;   // the form really launched: 0 when the device refused the dealt form's LDS and the streaming kernel took it
  const hipError_t le = crn::launch_sense(p, c.fft_len, c.mode == CRN_MODE_REF_MAG, c.window != CRN_WINDOW_RECT, h->variant,
                                          static_cast<hipStream_t>(stream), sc16, &deal_rounds_run);
  if (slot >= 0) (void)hipEventRecord(h->t_stop[slot], static_cast<hipStream_t>(stream));   // also after a failed launch: the slot must complete
  if (le == hipErrorNotSupported && sc16)
    return crn::fail(CRN_ERR_ARG, "this library was built without the wire-format kernels (make -C csrc SC16=1 builds libcrnsense_sc16.so)");
  if (le != hipSuccess) return crn::fail(CRN_ERR_DEVICE, std::string("launch_sense: ") + hipGetErrorString(le));
  // every input sample once: consecutive epochs closer together than an epoch is long (Welch) share their overlap
  const int64_t extent = (int64_t)(c.frames_per_epoch - 1) * frame_stride + (c.hop == c.fft_len ? samples_per_frame : c.fft_len);
  h->n_launches.fetch_add(1, std::memory_order_relaxed);
  if (deal_rounds_run > 0) h->n_dealt.fetch_add(1, std::memory_order_relaxed);
  h->n_epochs.fetch_add(n_epochs, std::memory_order_relaxed);
  h->n_samples.fetch_add((n_epochs - 1) * std::min(epoch_stride, extent) + extent, std::memory_order_relaxed);
  return CRN_OK;
}

int crn_sense_run_device(crn_handle *h, const float *d_iq, int64_t n_epochs, int32_t samples_per_frame,
                         int64_t epoch_stride, const crn_out *d_out, void *stream) {
  return run_device_impl(h, d_iq, n_epochs, samples_per_frame, epoch_stride, d_out, stream, false);
}

int crn_sense_run_device_cfar(crn_handle *h, const float *d_iq, int64_t n_epochs, int32_t samples_per_frame, int64_t epoch_stride,
                              const crn_out *d_out, uint32_t *d_bin_mask, int32_t *d_band_bins, void *stream) {
  return run_device_impl(h, d_iq, n_epochs, samples_per_frame, epoch_stride, d_out, stream, false, d_bin_mask, d_band_bins, true);
}

// internal (crn_ingest.cpp): either sample format through one call — a ring of wire-format packets (bytes_per_sample 4) exists only
// in a library built with the wire-format kernels
int crn_sense_run_device_any(crn_handle *h, const void *d_iq, int32_t bytes_per_sample, int64_t n_epochs, int32_t samples_per_frame,
                             int64_t epoch_stride, const crn_out *d_out, void *stream) {
  return run_device_impl(h, d_iq, n_epochs, samples_per_frame, epoch_stride, d_out, stream, bytes_per_sample == 4);
}

// One of the handle's grow-only buffers, pinned host or device memory: released and allocated anew when `need` exceeds its size.
static int grow(void **buf, size_t *bytes, size_t need, bool pinned, const char *what) {
  if (need <= *bytes) return CRN_OK;
  if (*buf) (void)(pinned ? hipHostFree(*buf) : hipFree(*buf));
  *buf = nullptr;
  *bytes = 0;
  const hipError_t e = pinned ? hipHostMalloc(buf, need, hipHostMallocDefault) : hipMalloc(buf, need);
  if (e != hipSuccess) return crn::fail(CRN_ERR_NOMEM, std::string(what) + hipGetErrorString(e));
  *bytes = need;
  return CRN_OK;
}

int crn_sense_run_host(crn_handle *h, const float *iq, int64_t n_epochs, int32_t samples_per_frame,
                       int64_t epoch_stride, const crn_out *out) {
  if (!h || !out) return crn::fail(CRN_ERR_ARG, "null handle / outputs");
  if (n_epochs < 0) return crn::fail(CRN_ERR_ARG, "n_epochs < 0");
  if (n_epochs == 0) return CRN_OK;
  if (!iq) return crn::fail(CRN_ERR_ARG, "null IQ pointer");
  int frame_stride = 0;
  if (int rc = resolve_strides(h, samples_per_frame, &epoch_stride, &frame_stride)) return rc;
  const crn_cfg &c = h->cfg;
  HIP_TRY(hipSetDevice(h->device));
  // samples touched: last epoch start + (K-1) frame strides + the last frame
  const int64_t last_frame = c.hop == c.fft_len ? samples_per_frame : c.fft_len;
  const size_t n_samples = (size_t)((n_epochs - 1) * epoch_stride + (int64_t)(c.frames_per_epoch - 1) * frame_stride + last_frame);
  const size_t b_iq = align_up(n_samples * 8, 256);
  const size_t b_feat = align_up((size_t)n_epochs * c.n_bands * sizeof(float), 256);
  const size_t b_ann = align_up((size_t)n_epochs * 3 * sizeof(double), 256);
  const size_t b_dec = align_up((size_t)n_epochs * sizeof(int32_t), 256);
  const size_t b_occ = align_up((size_t)n_epochs * c.n_bands, 256);
  const size_t b_spec = out->spectrum ? align_up((size_t)n_epochs * c.fft_len * sizeof(float), 256) : 0;
  const size_t need = b_iq + b_feat + b_ann + b_dec + b_occ + b_spec;
  const size_t res_bytes = b_feat + b_ann + b_dec + b_occ;
  // features | ann_out | decision | occupancy, back to back at `r` (pinned memory), to the caller's arrays
  auto scatter = [&](const char *r) {
    if (out->features) std::memcpy(out->features, r, (size_t)n_epochs * c.n_bands * sizeof(float));
    if (out->ann_out && c.decide == CRN_DECIDE_ANN) std::memcpy(out->ann_out, r + b_feat, (size_t)n_epochs * 3 * sizeof(double));
    if (out->decision) std::memcpy(out->decision, r + b_feat + b_ann, (size_t)n_epochs * sizeof(int32_t));
    if (out->occupancy) std::memcpy(out->occupancy, r + b_feat + b_ann + b_dec, (size_t)n_epochs * c.n_bands);
  };
  if (!out->spectrum && n_samples * 8 <= kInPlaceBytes) {
    // A decision's worth of samples (the engine's synchronous form: one epoch of 10 x 512): staged in pinned memory that the
    // kernel reads, and whose tail it writes the results to, over the bus itself — one launch and one wait instead of upload +
    // launch + download.
    if (int rc = grow(&h->h_small, &h->h_small_bytes, b_iq + res_bytes, true, "hipHostMalloc(in-place staging): ")) return rc;
    char *b = static_cast<char *>(h->h_small);
    std::memcpy(b, iq, n_samples * 8);
    crn_out d{};
    d.features = reinterpret_cast<float *>(b + b_iq);
    d.ann_out = reinterpret_cast<double *>(b + b_iq + b_feat);
    d.decision = reinterpret_cast<int32_t *>(b + b_iq + b_feat + b_ann);
    d.occupancy = reinterpret_cast<uint8_t *>(b + b_iq + b_feat + b_ann + b_dec);
    if (int rc = crn_sense_run_device(h, reinterpret_cast<const float *>(b), n_epochs, samples_per_frame, epoch_stride, &d, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    scatter(b + b_iq);
    return CRN_OK;
  }
  if (int rc = grow(&h->d_scratch, &h->scratch_bytes, need, false, "hipMalloc(scratch): ")) return rc;
  char *b = static_cast<char *>(h->d_scratch);
  float *d_iq = reinterpret_cast<float *>(b);
  crn_out d{};
  d.features = reinterpret_cast<float *>(b + b_iq);
  d.ann_out = reinterpret_cast<double *>(b + b_iq + b_feat);
  d.decision = reinterpret_cast<int32_t *>(b + b_iq + b_feat + b_ann);
  d.occupancy = reinterpret_cast<uint8_t *>(b + b_iq + b_feat + b_ann + b_dec);
  d.spectrum = out->spectrum ? reinterpret_cast<float *>(b + b_iq + b_feat + b_ann + b_dec + b_occ) : nullptr;
  hipStream_t s = nullptr;
  HIP_TRY(hipMemcpyAsync(d_iq, iq, n_samples * 8, hipMemcpyHostToDevice, s));
  if (int rc = crn_sense_run_device(h, d_iq, n_epochs, samples_per_frame, epoch_stride, &d, s)) return rc;
  // features | ann_out | decision | occupancy sit back to back in the scratch slab: one D2H into pinned staging, then scatter on the
  // host (a decision costs one upload, one launch, one download)
  if (int rc = grow(&h->h_results, &h->h_results_bytes, res_bytes, true, "hipHostMalloc(results): ")) return rc;
  HIP_TRY(hipMemcpyAsync(h->h_results, b + b_iq, res_bytes, hipMemcpyDeviceToHost, s));
  if (out->spectrum) HIP_TRY(hipMemcpyAsync(out->spectrum, d.spectrum, (size_t)n_epochs * c.fft_len * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  scatter(static_cast<const char *>(h->h_results));
  return CRN_OK;
}

int crn_sense_reserve_host(crn_handle *h, int64_t max_epochs, int32_t want_spectrum) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  if (max_epochs < 1) return crn::fail(CRN_ERR_ARG, "max_epochs < 1");
  const crn_cfg &c = h->cfg;
  // a run of zeros at the largest size: allocates the scratch slab and the pinned result staging, loads the code object, sets the LDS attribute
  const int64_t stride = (int64_t)c.frames_per_epoch * c.hop;
  const size_t n_samples = (size_t)(max_epochs * stride + (c.fft_len - c.hop));
  std::vector<float> zeros(n_samples * 2, 0.f);
  std::vector<float> feat((size_t)max_epochs * c.n_bands), spec(want_spectrum ? (size_t)max_epochs * c.fft_len : 0);
  crn_out o{};
  o.features = feat.data();
  o.spectrum = want_spectrum ? spec.data() : nullptr;
  return crn_sense_run_host(h, zeros.data(), max_epochs, c.fft_len, 0, &o);
}

int crn_sense_synchronize(crn_handle *h, void *stream) {
  if (!h) return crn::fail(CRN_ERR_ARG, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return CRN_OK;
}

int crn_monitor_rows_device(crn_handle *h, const float *d_spectrum, int64_t n_rows, int32_t kind, float alpha,
                            int32_t first, float *d_state, float *d_waterfall_db, float *d_average_db, void *stream) {
  if (!h || !d_spectrum || !d_state) return crn::fail(CRN_ERR_ARG, "null handle / spectrum / state");
  if (n_rows < 0) return crn::fail(CRN_ERR_ARG, "n_rows < 0");
  if (kind != CRN_MONITOR_GNURADIO && kind != CRN_MONITOR_PSD) return crn::fail(CRN_ERR_ARG, "unknown monitor kind");
  if (!(alpha > 0.f && alpha <= 1.f)) return crn::fail(CRN_ERR_ARG, "alpha must be in (0, 1]");
  std::lock_guard<std::mutex> lk(h->tables_mu);
  HIP_TRY(hipSetDevice(h->device));
  const double N = (double)h->cfg.fft_len;
  crn::MonitorParams p{};
  p.spectrum = d_spectrum;
  p.n_rows = n_rows;
  p.n = h->cfg.fft_len;
  p.alpha = alpha;
  p.scale = (float)(1.0 / (kind == CRN_MONITOR_GNURADIO ? N * N : N * h->window_power));
  p.db_domain = kind == CRN_MONITOR_GNURADIO;
  p.first = first != 0;
  p.state = d_state;
  p.waterfall_db = d_waterfall_db;
  p.average_db = d_average_db;
  HIP_TRY(crn::launch_monitor(p, static_cast<hipStream_t>(stream)));
  return CRN_OK;
}

int crn_fft_forward_device(crn_handle *h, const float *d_in, int64_t n_frames, int32_t samples_per_frame,
                           int64_t frame_stride, float *d_out, void *stream) {
  if (!h || !d_in || !d_out) return crn::fail(CRN_ERR_ARG, "null handle / buffer");
  if (n_frames < 0) return crn::fail(CRN_ERR_ARG, "negative frame count");
  std::lock_guard<std::mutex> lk(h->tables_mu);
  if (samples_per_frame < 1 || samples_per_frame > h->cfg.fft_len)
    return crn::fail(CRN_ERR_ARG, "samples_per_frame must be in 1..fft_len");
  if (frame_stride <= 0) frame_stride = samples_per_frame;
  HIP_TRY(hipSetDevice(h->device));
  crn::FftParams p{};
  p.in = reinterpret_cast<const float2 *>(d_in);
  p.out = reinterpret_cast<float2 *>(d_out);
  p.n_frames = n_frames;
  p.frame_stride = frame_stride;
  p.L = samples_per_frame;
  p.tw1 = h->d_tw1;
  p.tw2 = h->d_tw2;
  HIP_TRY(crn::launch_fft(p, h->cfg.fft_len, static_cast<hipStream_t>(stream)));
  return CRN_OK;
}

int crn_synth_fill_device(crn_handle *h, float *d_iq, int64_t n_epochs, int64_t samples_per_epoch,
                          uint64_t seed, float noise_power, float signal_rms, int32_t tones_per_band,
                          int32_t *d_truth, void *stream) {
  crn_synth_cfg sc{};
  sc.seed = seed;
  sc.noise_power = noise_power;
  sc.signal_rms = signal_rms;
  sc.tones_per_band = tones_per_band;
  sc.pu_model = CRN_PU_UNIFORM;
  sc.signal_kind = CRN_SIG_TONES;
  sc.n_streams = 1;
  sc.adc_bits = 0;
  return crn_synth_fill_device_ex(h, &sc, d_iq, n_epochs, samples_per_epoch, d_truth, stream);
}

int crn_synth_fill_device_ex(crn_handle *h, const crn_synth_cfg *sc, float *d_iq, int64_t n_epochs,
                             int64_t samples_per_epoch, int32_t *d_truth, void *stream) {
  if (!h || !d_iq || !sc) return crn::fail(CRN_ERR_ARG, "null handle / configuration / IQ pointer");
  if (n_epochs < 0 || samples_per_epoch < 1) return crn::fail(CRN_ERR_ARG, "bad sizes");
  if (sc->tones_per_band < 0 || sc->noise_power < 0.f) return crn::fail(CRN_ERR_ARG, "bad signal parameters");
  if (sc->pu_model < CRN_PU_UNIFORM || sc->pu_model > CRN_PU_SWEEP)
    return crn::fail(CRN_ERR_ARG, "unknown pu_model");
  if (sc->signal_kind < CRN_SIG_TONES || sc->signal_kind > CRN_SIG_OFDM)
    return crn::fail(CRN_ERR_ARG, "unknown signal_kind");
  if (sc->n_streams < 1) return crn::fail(CRN_ERR_ARG, "n_streams must be >= 1");
  if (sc->adc_bits != 0 && (sc->adc_bits < 2 || sc->adc_bits > 24)) return crn::fail(CRN_ERR_ARG, "adc_bits must be 0 or 2..24");
  const bool markov = sc->pu_model == CRN_PU_MARKOV_AS_WRITTEN || sc->pu_model == CRN_PU_MARKOV_INTENDED;
  if (sc->pu_model != CRN_PU_UNIFORM) {
    if (markov && !d_truth) return crn::fail(CRN_ERR_ARG, "the Markov traffic models need d_truth");
    if (n_epochs % sc->n_streams != 0) return crn::fail(CRN_ERR_ARG, "n_streams must divide n_epochs");
  }
  std::lock_guard<std::mutex> lk(h->tables_mu);
  const crn_cfg &c = h->cfg;
  HIP_TRY(hipSetDevice(h->device));
  crn::SynthParams p{};
  p.iq = reinterpret_cast<float2 *>(d_iq);
  p.n_epochs = n_epochs;
  p.samples_per_epoch = samples_per_epoch;
  p.seed = sc->seed;
  p.noise_sigma = std::sqrt(sc->noise_power * 0.5f);
  p.tones = sc->tones_per_band;
  p.tone_amp = sc->tones_per_band > 0 ? sc->signal_rms / std::sqrt((float)sc->tones_per_band) : 0.f;
  p.signal_rms = sc->signal_rms;
  p.pu_model = sc->pu_model;
  p.signal_kind = sc->signal_kind;
  p.epochs_per_stream = n_epochs / sc->n_streams;
  p.adc_scale = sc->adc_bits ? (float)(1 << (sc->adc_bits - 1)) : 0.f;
  p.fft_len = c.fft_len;
  if (c.ref_band >= 0 || c.decide == CRN_DECIDE_ANN) {  // {NF, CH1, ..}: band 0 is never driven
    p.active_band0 = 1;
    p.n_active = std::min(3, c.n_bands - 1);
  } else {
    p.active_band0 = 0;
    p.n_active = c.n_bands;
  }
  if (sc->signal_kind == CRN_SIG_TONES && sc->tones_per_band == 0) p.n_active = 0;
  p.band_bins_begin = h->d_band_bins_begin;
  p.band_bins = h->d_band_bins;
  p.band_c2 = h->d_band_c2;
  p.truth = d_truth;
  if (sc->pu_model != CRN_PU_UNIFORM && p.n_active < 1)
    return crn::fail(CRN_ERR_ARG, "the Markov and sweep traffic models need at least one driven band");
  if (markov) HIP_TRY(crn::launch_pu_pattern(p, static_cast<hipStream_t>(stream)));
  HIP_TRY(crn::launch_synth(p, static_cast<hipStream_t>(stream)));
  return CRN_OK;
}

}  // extern "C"
