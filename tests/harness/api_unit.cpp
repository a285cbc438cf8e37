// TEST INFRASTRUCTURE: the host logic of csrc/crn_api.cpp, crn_tables.cpp, crn_updates.cpp, crn_cfar.cpp and crn_api_sc16.cpp without a GPU — table building (twiddles, window, the band plan
// in its packed LDS form, row entries, accumulator mask), launch geometry (every epoch group handed to exactly one workgroup, whatever
// the batch size, FFT size and CU count), argument checks, live updates, counters.  Those files and crn_cfg.cpp are compiled as they
// are against tests/harness/fake_hip (device memory = host memory, so the tables a launch would read can be read back here); the
// kernels' launch functions are stand-ins that record the parameter block they were handed.  Nothing of this is linked into the product.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/crn_sense.h"
#include "../../include/crn_sense_sc16.h"
#include "../../cognitive-radio-network_amd/csrc/crn_forms.h"

std::atomic<long long> g_fake_gpu_latency_ns{0};
extern "C" int crn_sense_ring_count(crn_handle *h, int delta);   // internal (csrc/crn_internal.h; crn_ingest.cpp uses it)

// ---- stand-ins for csrc/crn_kernels.hip (what the host files call) -------------------------------------------------
namespace {
crn::SenseParams g_last;
int g_last_fft = 0, g_last_variant = -1, g_launches = 0;
bool g_last_mag = false, g_last_win = false, g_last_sc16 = false;
bool g_write_pattern = false;
bool g_refuse_dealt = false;   // the device refuses the dealt form's LDS: the real launch_sense falls back to the streaming kernel
float g_iq_first = 0, g_iq_last = 0;
crn::FftParams g_fft;
crn::MonitorParams g_mon;
crn::SynthParams g_synth;
int g_fft_len = 0, g_synth_launches = 0, g_pattern_launches = 0;
long long g_pack_n = 0;
float g_pack_scale = 0;
}  // namespace
namespace crn {
hipError_t launch_sense(const SenseParams &p, int fft_len, bool mag, bool win, int variant, hipStream_t, bool sc16, int *deal_rounds_run) {
  if (deal_rounds_run) *deal_rounds_run = g_refuse_dealt ? 0 : p.deal_rounds;   // (csrc/crn_sense_kernel.h: launch_selected)
  if (g_write_pattern) {
    // what a launch reads and writes, touched at its ends (under AddressSanitizer a slab one byte short is a report) and filled
    // with values the caller can recognise after the copies back
    const float2 first = p.iq[0], last = p.iq[p.total_samples - 1];
    g_iq_first = first.x;
    g_iq_last = last.y;
    for (long long e = 0; e < p.n_epochs; e++) {
      for (int b = 0; b < p.n_bands; b++) {
        if (p.features) p.features[e * p.n_bands + b] = (float)(e * 100 + b);
        if (p.occupancy) p.occupancy[e * p.n_bands + b] = (uint8_t)((e + b) & 1);
      }
      if (p.ann_out) for (int k = 0; k < 3; k++) p.ann_out[e * 3 + k] = (double)e + 0.25 * k;
      if (p.decision) p.decision[e] = (int32_t)(e % 4);
      if (p.spectrum) for (int k = 0; k < fft_len; k++) p.spectrum[e * fft_len + k] = (float)(e + k);
    }
  }
  g_last = p;
  g_last_fft = fft_len;
  g_last_mag = mag;
  g_last_win = win;
  g_last_variant = variant;
  g_last_sc16 = sc16;
  g_launches++;
  return hipSuccess;
}
hipError_t launch_nop(hipStream_t) { return hipSuccess; }
// (the forms, the selection rule, sense_deal_rounds and the variant policy are the library's own: csrc/crn_forms.cpp is linked as it is)
hipError_t launch_fft(const FftParams &p, int fft_len, hipStream_t) { g_fft = p; g_fft_len = fft_len; return hipSuccess; }
hipError_t launch_monitor(const MonitorParams &p, hipStream_t) { g_mon = p; return hipSuccess; }
hipError_t launch_noise_floor(const float *feat, int n_epochs, int nb, float *scratch, hipStream_t) {
  // touches what the kernel touches: the features it was given and the result word behind kNoiseFloorMaxEpochs medians
  float sum = 0;
  for (long long i = 0; i < (long long)n_epochs * nb; i++) sum += feat[i];
  scratch[kNoiseFloorMaxEpochs] = sum;
  return hipSuccess;
}
hipError_t launch_synth(const SynthParams &p, hipStream_t) { g_synth = p; g_synth_launches++; return hipSuccess; }
hipError_t launch_pack_sc16(const float *, long long n, short *, float full_scale, hipStream_t) { g_pack_n = n; g_pack_scale = full_scale; return hipSuccess; }
hipError_t launch_pu_pattern(const SynthParams &, hipStream_t) { g_pattern_launches++; return hipSuccess; }
}  // namespace crn

// ---- checks ---------------------------------------------------------------------------------------------------------
static int g_failed = 0;
#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "api_unit: %s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                                      \
    }                                                                                  \
  } while (0)

static crn_out any_outputs() {
  static float f[4];
  static double a[3];
  static int32_t d[1];
  static uint8_t o[4];
  crn_out out{f, a, d, o, nullptr};   // never written: the launch is a stand-in
  return out;
}
alignas(16) static float g_iq[64];   // an aligned, non-null "device" pointer

static crn::SenseParams launch(crn_handle *h, int64_t n_epochs, int L, int64_t stride = 0) {
  const crn_out o = any_outputs();
  const int before = g_launches;
  const int rc = crn_sense_run_device(h, g_iq, n_epochs, L, stride, &o, nullptr);
  if (rc != CRN_OK) std::fprintf(stderr, "api_unit: run_device failed: %s\n", crn_last_error());
  REQUIRE(rc == CRN_OK);
  REQUIRE(g_launches == before + 1);
  return g_last;
}

// every epoch group handed to exactly one workgroup: the arithmetic of launch_cfg / stream_span (csrc/crn_sense_kernel.h) restated
static void check_coverage(const crn::SenseParams &p, int fft_len, const char *what) {
  const int groups = 256 / (fft_len / 16);
  const long long n_groups = (p.n_epochs + groups - 1) / groups;
  const long long epw = p.groups_per_wg, tail_epw = p.tail_groups_per_wg < 1 ? 1 : p.tail_groups_per_wg;
  REQUIRE(epw >= 1);
  long long n_big = p.n_big_wgs;
  REQUIRE(n_big >= 0);
  if (n_big * epw > n_groups) n_big = n_groups / epw;   // launch_cfg's clamp
  const long long rest = n_groups - n_big * epw;
  const long long grid = n_big + (rest + tail_epw - 1) / tail_epw;
  std::vector<unsigned char> seen((size_t)n_groups, 0);
  bool ok = grid >= 1;
  for (long long b = 0; b < grid && ok; b++) {
    const bool big = b < n_big;
    const long long w = big ? epw : tail_epw;
    const long long g0 = big ? b * epw : n_big * epw + (b - n_big) * tail_epw;
    const long long n_local = (n_groups - g0) < w ? (n_groups - g0) : w;
    if (n_local < 1 || g0 < 0) ok = false;   // no empty workgroup
    for (long long g = g0; ok && g < g0 + n_local; g++) {
      if (g >= n_groups || seen[(size_t)g]) ok = false;
      else seen[(size_t)g] = 1;
    }
  }
  for (long long g = 0; ok && g < n_groups; g++) ok = seen[(size_t)g] != 0;
  if (!ok)
    std::fprintf(stderr, "api_unit: coverage broken (%s): N %d epochs %lld groups %lld big %lld x %lld tail x %lld\n", what, fft_len,
                 (long long)p.n_epochs, n_groups, (long long)p.n_big_wgs, epw, tail_epw);
  REQUIRE(ok);
}

static void test_tables(int N, bool reference_plan) {
  crn_cfg cfg;
  if (reference_plan) REQUIRE(crn_cfg_reference_scaled(&cfg, N) == CRN_OK);
  else REQUIRE(crn_cfg_energy_scaled(&cfg, N, 4.0f) == CRN_OK);
  crn_handle *h = nullptr;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  const crn::SenseParams p = launch(h, 100, N);
  const int T = N / 16, R3 = N / 256;
  REQUIRE(g_last_fft == N);
  REQUIRE(g_last_mag == (cfg.mode == CRN_MODE_REF_MAG));
  // twiddles: W_N^{i t} (rows 0..15), W_N^{16 t} (row 16), W_T^{i m}
  double worst = 0;
  for (int i = 0; i <= 16; i++)
    for (int t = 0; t < T; t++) {
      const long long q = (i < 16 ? (long long)i * t : 16LL * t) % N;
      const long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)q / (long double)N;
      worst = std::fmax(worst, std::fabs((double)p.tw1[(size_t)i * T + t].x - (double)cosl(ang)));
      worst = std::fmax(worst, std::fabs((double)p.tw1[(size_t)i * T + t].y - (double)sinl(ang)));
    }
  for (int i = 0; i < 16; i++)
    for (int m = 0; m < R3; m++) {
      const long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)(((long long)i * m) % T) / (long double)T;
      worst = std::fmax(worst, std::fabs((double)p.tw2[(size_t)i * R3 + m].x - (double)cosl(ang)));
      worst = std::fmax(worst, std::fabs((double)p.tw2[(size_t)i * R3 + m].y - (double)sinl(ang)));
    }
  REQUIRE(worst <= 6.0e-8);   // correctly rounded to fp32: half an ulp of 1
  // packed band table: the plan as cfg states it
  const int *tab = p.band_tab;
  std::vector<std::set<int>> want(cfg.n_bands);
  int n_seg_total = 0;
  for (int b = 0; b < cfg.n_bands; b++) {
    REQUIRE(tab[b] == n_seg_total);
    for (int s = 0; s < cfg.n_segs; s++)
      if (cfg.segs[s].band == b) {
        REQUIRE(tab[96 + n_seg_total] == cfg.segs[s].lo && tab[256 + n_seg_total] == cfg.segs[s].hi);   // table order inside a band
        for (int k = cfg.segs[s].lo; k < cfg.segs[s].hi; k++) want[b].insert(k);
        n_seg_total++;
      }
  }
  REQUIRE(tab[cfg.n_bands] == n_seg_total);
  REQUIRE(std::memcmp(&tab[416], cfg.thresh, sizeof(float) * CRN_MAX_BANDS) == 0);
  REQUIRE(std::memcmp(&tab[544], cfg.ann_w_ih, sizeof(cfg.ann_w_ih)) == 0);
  REQUIRE(std::memcmp(&tab[604], cfg.ann_w_ho, sizeof(cfg.ann_w_ho)) == 0);
  REQUIRE(std::memcmp(p.thresh, cfg.thresh, sizeof(float) * cfg.n_bands) == 0);
  // row entries (register-resident band sums): the pieces of every row rebuild the plan exactly, no bin twice, none missing
  REQUIRE(p.n_row_entries > 0);   // both plans are small
  const int cap = crn::kRowEntryWords / R3;
  std::vector<std::set<int>> got(cfg.n_bands);
  int entries = 0;
  for (int d = 0; d < R3 && d < 16; d++) {
    bool ended = false;
    for (int sl = 0; sl < cap; sl++) {
      const int w = tab[512 + d * cap + sl];
      if (w == 0) { ended = true; continue; }
      REQUIRE(!ended);   // used slots come first
      const int band = w >> 18, lo = (w >> 9) & 511, hi = w & 511;
      REQUIRE(band >= 0 && band < cfg.n_bands && lo < hi && hi <= 256);
      for (int k = lo; k < hi; k++) REQUIRE(got[band].insert(256 * d + k).second);
      entries++;
    }
  }
  REQUIRE(entries == p.n_row_entries);
  for (int b = 0; b < cfg.n_bands; b++) REQUIRE(got[b] == want[b]);
  // accumulator mask: bin k sits in register ((k % 256) / 16 mod J) R3 + k / 256 of its thread
  unsigned mask = 0;
  const int J = 16 / R3;
  for (int b = 0; b < cfg.n_bands; b++)
    for (int k : want[b]) mask |= 1u << ((((k & 255) >> 4) % J) * R3 + (k >> 8));
  REQUIRE(p.acc_mask == mask);
  REQUIRE(mask == crn::sense_ref_acc_mask(N));   // both helpers lay out the reference channel plan scaled by N / 512
  REQUIRE(mask == (N == 512 ? 0x85e1u : N == 1024 ? 0xbf73u : N == 2048 ? 0x9f9bu : 0x8267u));
  // variant 2: no pruning
  REQUIRE(crn_sense_set_variant(h, 2) == CRN_OK);
  REQUIRE(launch(h, 100, N).acc_mask == 0xFFFFu);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
}

static void test_windows() {
  crn_cfg cfg;
  REQUIRE(crn_cfg_welch(&cfg, 4096, 8, 64) == CRN_OK);
  for (int b = 0; b < 64; b++) cfg.thresh[b] = 1.0f;
  crn_handle *h = nullptr;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  const crn::SenseParams p = launch(h, 1000, 4096);
  REQUIRE(g_last_win && !g_last_mag);
  REQUIRE(p.hann_sym == 1 && p.aligned_shift == 6);
  REQUIRE(p.frame_stride == 2048 && p.epoch_stride == 8 * 2048);   // dense Welch epochs: the stream form
  double worst = 0;
  for (int n = 0; n < 4096; n++) worst = std::fmax(worst, std::fabs((double)p.window[n] - (0.5 - 0.5 * std::cos(2.0 * M_PI * n / 4096.0))));
  REQUIRE(worst <= 6.0e-8);
  for (int n = 0; n < 2048; n++) REQUIRE(std::fabs((double)p.window[n] + (double)p.window[n + 2048] - 1.0) <= 1.2e-7);   // what kHannSym relies on
  // a spectrum request turns the aligned close off
  crn_out o = any_outputs();
  static float spec[4096];
  o.spectrum = spec;
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 4096, 0, &o, nullptr) == CRN_OK);
  REQUIRE(g_last.aligned_shift == 0 && g_last.spectrum == spec);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
}

static void test_geometry() {
  const int cus[] = {256, 304, 64, 8, 1};
  const long long epochs[] = {1, 2, 7, 8, 9, 63, 255, 256, 257, 1023, 1024, 1025, 4095, 4097, 6553, 13107, 28672, 65536, 100003, 229376, 1000000};
  for (int n_cus : cus) {
    g_fake_hip_cus = n_cus;
    for (int N : {512, 1024, 2048, 4096})
      for (int K : {1, 3, 10, 32}) {
        crn_cfg cfg;
        REQUIRE(crn_cfg_energy_scaled(&cfg, N, 4.0f) == CRN_OK);
        cfg.frames_per_epoch = K;
        crn_handle *h = nullptr;
        REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
        int64_t dealt_before = 0, dealt_after = 0;
        REQUIRE(crn_sense_dealt_launches(h, &dealt_before) == CRN_OK && dealt_before == 0);
        for (long long E : epochs) {
          const crn::SenseParams p = launch(h, E, N);
          check_coverage(p, N, "plain");
          // the dealt-frame form: launches of up to one epoch per compute unit, 512 / 1024 points, at least two frames
          const int groups = 256 / (N / 16);
          const int fits = crn::sense_deal_rounds(N, false, false, false, K, 160 * 1024);   // 0 when the K frame slots do not fit in LDS (K = 32 here)
          REQUIRE(fits == 0 || fits == (K + groups - 1) / groups);
          REQUIRE((fits > 0) == ((N == 512 || N == 1024) && K >= 2 && K <= 10));
          const bool want_deal = fits > 0 && E <= (long long)n_cus;
          REQUIRE(p.deal_rounds == (want_deal ? fits : 0));
          dealt_before += want_deal;
          // ... switched off and forced (A/B codes 401 / 402), and back to automatic
          REQUIRE(crn_sense_set_variant(h, 401) == CRN_OK);
          REQUIRE(launch(h, E, N).deal_rounds == 0);
          REQUIRE(crn_sense_set_variant(h, 402) == CRN_OK);
          const bool can = fits > 0;
          REQUIRE((launch(h, E, N).deal_rounds > 0) == can);
          dealt_before += can;
          REQUIRE(crn_sense_set_variant(h, 400) == CRN_OK);
          REQUIRE(p.groups_per_wg >= 1 && p.groups_per_wg <= 4 && p.tail_groups_per_wg == 1);
          const long long n_groups = (E + 256 / (N / 16) - 1) / (256 / (N / 16));
          REQUIRE(n_groups - p.n_big_wgs * p.groups_per_wg <= std::max<long long>(n_groups / 4, 0) + p.groups_per_wg);   // the single-group tail is at most a quarter
          REQUIRE(p.total_samples == (E - 1) * (long long)K * N + (long long)K * N);
        }
        REQUIRE(crn_sense_dealt_launches(h, &dealt_after) == CRN_OK && dealt_after == dealt_before);
        // geometry overrides (A/B codes) keep the coverage
        REQUIRE(crn_sense_set_variant(h, 100 + 7) == CRN_OK);
        REQUIRE(crn_sense_set_variant(h, 200 + 3) == CRN_OK);
        REQUIRE(crn_sense_set_variant(h, 300 + 2) == CRN_OK);
        for (long long E : epochs) check_coverage(launch(h, E, N), N, "overrides");
        REQUIRE(crn_sense_destroy(h) == CRN_OK);
      }
    // the Welch stream: long spans, a tail of shorter ones
    for (int K : {1, 8, 32, 100}) {
      crn_cfg cfg;
      REQUIRE(crn_cfg_welch(&cfg, 4096, K, 64) == CRN_OK);
      for (int b = 0; b < 64; b++) cfg.thresh[b] = 1.0f;
      crn_handle *h = nullptr;
      REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
      for (long long E : epochs) {
        const crn::SenseParams p = launch(h, E, 4096);
        check_coverage(p, 4096, "welch stream");
        REQUIRE(p.groups_per_wg >= 1 && p.groups_per_wg <= 64 && p.tail_groups_per_wg >= 1 && p.tail_groups_per_wg <= 8);
        REQUIRE(p.total_samples == (E - 1) * (long long)K * 2048 + (long long)(K - 1) * 2048 + 4096);
      }
      REQUIRE(crn_sense_destroy(h) == CRN_OK);
    }
  }
  g_fake_hip_cus = 256;
}

static void test_arguments_and_counters() {
  crn_cfg cfg;
  REQUIRE(crn_cfg_reference(&cfg) == CRN_OK);
  crn_handle *h = nullptr;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  const crn_out o = any_outputs();
  const int before = g_launches;
  REQUIRE(crn_sense_run_device(nullptr, g_iq, 1, 364, 0, &o, nullptr) == CRN_ERR_ARG);
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 364, 0, nullptr, nullptr) == CRN_ERR_ARG);
  REQUIRE(crn_sense_run_device(h, g_iq, -1, 364, 0, &o, nullptr) == CRN_ERR_ARG);
  REQUIRE(crn_sense_run_device(h, nullptr, 1, 364, 0, &o, nullptr) == CRN_ERR_ARG);
  REQUIRE(crn_sense_run_device(h, reinterpret_cast<const float *>(reinterpret_cast<const char *>(g_iq) + 4), 1, 364, 0, &o, nullptr) == CRN_ERR_ARG);
  REQUIRE(std::strstr(crn_last_error(), "aligned") != nullptr);
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 513, 0, &o, nullptr) == CRN_ERR_ARG);    // a packet longer than the transform (.cpp:149 overruns)
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 0, 0, &o, nullptr) == CRN_ERR_ARG);
  REQUIRE(crn_sense_run_device(h, g_iq, (int64_t)1 << 31, 364, 0, &o, nullptr) == CRN_ERR_ARG);
  REQUIRE(crn_sense_run_device(h, g_iq, 10, 364, (int64_t)1 << 26, &o, nullptr) == CRN_ERR_ARG);   // a workgroup's window past 2 GiB
  REQUIRE(std::strstr(crn_last_error(), "epoch_stride") != nullptr);
  REQUIRE(g_launches == before);                                                      // none of them reached the device
  REQUIRE(crn_sense_run_device(h, g_iq, 0, 364, 0, &o, nullptr) == CRN_OK && g_launches == before);   // an empty batch is not a launch
  // short packets: L samples per frame, K L apart by default
  const crn::SenseParams p = launch(h, 12, 364);
  REQUIRE(p.L == 364 && p.frame_stride == 364 && p.epoch_stride == 3640 && p.K == 10 && p.decide == crn::CRN_DECIDE_ANN_K && p.n_bands == 4);
  REQUIRE(p.total_samples == 11 * 3640 + 9 * 364 + 364);
  REQUIRE(p.ann_out != nullptr && p.ann_threshold == cfg.ann_threshold);
  // counters
  crn_sense_stats st;
  REQUIRE(crn_sense_get_stats(h, &st) == CRN_OK);
  REQUIRE(st.launches == 1 && st.epochs == 12 && st.samples == 12 * 3640);
  // the shipped variant policy
  REQUIRE(crn_sense_set_variant(h, 7) == CRN_ERR_ARG && std::strstr(crn_last_error(), "measurement variant") != nullptr);
  REQUIRE(crn_sense_set_variant(h, 2) == CRN_OK && crn_sense_set_variant(h, 13) == CRN_OK && crn_sense_set_variant(h, 0) == CRN_OK);
  REQUIRE(crn_sense_set_variant(h, 23) == CRN_ERR_ARG);   // (removed in round 5)
  REQUIRE(crn_sense_set_variant(h, 403) == CRN_ERR_ARG && crn_sense_set_variant(h, -1) == CRN_ERR_ARG);
  {
    int64_t n = -1;
    REQUIRE(crn_sense_dealt_launches(nullptr, &n) == CRN_ERR_ARG && crn_sense_dealt_launches(h, nullptr) == CRN_ERR_ARG);
    REQUIRE(crn_sense_dealt_launches(h, &n) == CRN_OK && n >= 0);
  }
  // live updates reach the next launch's tables
  float thr[4] = {9.f, 8.f, 7.f, 6.f};
  REQUIRE(crn_sense_set_thresholds(h, thr, 4, nullptr) == CRN_OK);
  REQUIRE(crn_sense_set_thresholds(h, thr, 5, nullptr) == CRN_ERR_ARG);
  REQUIRE(std::memcmp(launch(h, 1, 364).thresh, thr, sizeof thr) == 0 && std::memcmp(&g_last.band_tab[416], thr, sizeof thr) == 0);
  double wih[5][6], who[6][4];
  for (int i = 0; i < 5; i++) for (int j = 0; j < 6; j++) wih[i][j] = 0.01 * (i * 6 + j);
  for (int i = 0; i < 6; i++) for (int j = 0; j < 4; j++) who[i][j] = -0.02 * (i * 4 + j);
  REQUIRE(crn_sense_set_ann(h, wih, who, 0.7, nullptr) == CRN_OK);
  const crn::SenseParams q = launch(h, 1, 364);
  REQUIRE(q.ann_threshold == 0.7 && std::memcmp(q.ann_w_ih, wih, sizeof wih) == 0 && std::memcmp(q.ann_w_ho, who, sizeof who) == 0);
  REQUIRE(std::memcmp(&q.band_tab[544], wih, sizeof wih) == 0 && std::memcmp(&q.band_tab[604], who, sizeof who) == 0);
  // a new band plan on the live handle; refused when it would change the band count under an attached ring
  crn_band_seg segs[3] = {{10, 20, 0}, {300, 310, 1}, {100, 140, 0}};
  float thr2[2] = {1.f, 2.f};
  REQUIRE(crn_sense_set_bands(h, segs, 3, 2, thr2) == CRN_ERR_ARG);   // the reference network needs its four features
  REQUIRE(crn_sense_destroy(h) == CRN_OK);

  REQUIRE(crn_cfg_energy_scaled(&cfg, 1024, 4.0f) == CRN_OK);
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  REQUIRE(crn_sense_ring_count(h, +1) == CRN_OK);
  REQUIRE(crn_sense_set_bands(h, segs, 3, 2, thr2) == CRN_ERR_STATE);
  REQUIRE(crn_sense_ring_count(h, -1) == CRN_OK);
  REQUIRE(crn_sense_set_bands(h, segs, 3, 2, thr2) == CRN_OK);
  const crn::SenseParams r = launch(h, 5, 1024);
  REQUIRE(r.n_bands == 2 && r.band_tab[0] == 0 && r.band_tab[1] == 2 && r.band_tab[2] == 3);
  REQUIRE(r.band_tab[96] == 10 && r.band_tab[97] == 100 && r.band_tab[98] == 300);   // grouped by band, table order inside a band
  REQUIRE(r.acc_mask != 0xFFFFu);   // 3 short segments touch few registers -> but not the reference plan's: the full kernel runs
  segs[0].hi = 2000;                // beyond the transform
  REQUIRE(crn_sense_set_bands(h, segs, 3, 2, thr2) == CRN_ERR_ARG);
  REQUIRE(launch(h, 5, 1024).band_tab[96] == 10);   // the old plan stays in force
  REQUIRE(crn_sense_destroy(h) == CRN_OK);

  // configuration errors
  REQUIRE(crn_cfg_reference(&cfg) == CRN_OK);
  cfg.fft_len = 768;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_ERR_ARG);
  REQUIRE(crn_cfg_reference(&cfg) == CRN_OK);
  cfg.abi_version++;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_ERR_ARG && std::strstr(crn_last_error(), "abi_version") != nullptr);
  int32_t built = 0, runtime = 0;
  REQUIRE(crn_build_info(&built, &runtime) == CRN_OK && built == runtime && built == HIP_VERSION);
}

// crn_sense_run_host: the staging slabs (pinned in-place form for a decision's worth of samples, device scratch + pinned results
// otherwise) hold exactly what the launch touches, and every output comes back to the caller's arrays
static void run_host_case(crn_cfg cfg, int64_t E, int L, bool want_spectrum) {
  crn_handle *h = nullptr;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  const int N = cfg.fft_len, K = cfg.frames_per_epoch;
  const bool overlapped = cfg.hop != N;
  const int64_t n_samples = overlapped ? (E * K - 1) * (int64_t)cfg.hop + N : E * K * (int64_t)L;
  std::vector<float> iq((size_t)n_samples * 2);
  for (size_t i = 0; i < iq.size(); i++) iq[i] = (float)(i % 8191);
  std::vector<float> feat((size_t)E * cfg.n_bands, -1.f), spec(want_spectrum ? (size_t)E * N : 0, -1.f);
  std::vector<double> ann((size_t)E * 3, -1.0);
  std::vector<int32_t> dec((size_t)E, -1);
  std::vector<uint8_t> occ((size_t)E * cfg.n_bands, 9);
  crn_out o{feat.data(), ann.data(), dec.data(), occ.data(), want_spectrum ? spec.data() : nullptr};
  g_write_pattern = true;
  const int rc = crn_sense_run_host(h, iq.data(), E, L, 0, &o);
  g_write_pattern = false;
  if (rc != CRN_OK) std::fprintf(stderr, "api_unit: run_host failed: %s\n", crn_last_error());
  REQUIRE(rc == CRN_OK);
  REQUIRE(g_last.total_samples == n_samples);
  REQUIRE(g_iq_first == iq[0] && g_iq_last == iq[iq.size() - 1]);   // the launch saw the caller's samples, first to last
  bool ok = true;
  for (int64_t e = 0; e < E && ok; e++) {
    for (int b = 0; b < cfg.n_bands; b++) ok = ok && feat[e * cfg.n_bands + b] == (float)(e * 100 + b) && occ[e * cfg.n_bands + b] == (uint8_t)((e + b) & 1);
    ok = ok && dec[e] == (int32_t)(e % 4);
    if (cfg.decide == CRN_DECIDE_ANN) for (int k = 0; k < 3; k++) ok = ok && ann[e * 3 + k] == (double)e + 0.25 * k;
    else ok = ok && ann[e * 3] == -1.0;   // not the network's mode: left alone
    if (want_spectrum) ok = ok && spec[e * N] == (float)e && spec[e * N + N - 1] == (float)(e + N - 1);
  }
  REQUIRE(ok);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
}

static void test_run_host() {
  crn_cfg cfg;
  REQUIRE(crn_cfg_reference(&cfg) == CRN_OK);
  for (int64_t E : {1, 2, 12, 300, 5000}) {   // in-place pinned form for the small ones, scratch + pinned results for the others
    run_host_case(cfg, E, 364, false);
    run_host_case(cfg, E, 512, false);
  }
  run_host_case(cfg, 1, 512, true);
  run_host_case(cfg, 77, 100, true);
  REQUIRE(crn_cfg_energy_scaled(&cfg, 4096, 4.0f) == CRN_OK);
  for (int64_t E : {1, 3, 200}) run_host_case(cfg, E, 4096, E == 3);
  REQUIRE(crn_cfg_welch(&cfg, 4096, 8, 64) == CRN_OK);
  for (int b = 0; b < 64; b++) cfg.thresh[b] = 1.0f;
  for (int64_t E : {1, 5, 40}) run_host_case(cfg, E, 4096, false);
  REQUIRE(crn_cfg_welch_scaled(&cfg, 1024, 6, 4.0f) == CRN_OK);
  run_host_case(cfg, 9, 1024, true);
  // a handle re-used with growing and shrinking batches keeps its slabs consistent
  REQUIRE(crn_cfg_reference(&cfg) == CRN_OK);
  crn_handle *h = nullptr;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  REQUIRE(crn_sense_reserve_host(h, 64, 1) == CRN_OK);
  g_write_pattern = true;
  for (int64_t E : {1, 500, 3, 2000, 1, 64}) {
    std::vector<float> iq((size_t)E * 3640 * 2, 1.f), feat((size_t)E * 4);
    std::vector<int32_t> dec((size_t)E);
    crn_out o{feat.data(), nullptr, dec.data(), nullptr, nullptr};
    REQUIRE(crn_sense_run_host(h, iq.data(), E, 364, 0, &o) == CRN_OK);
    REQUIRE(feat[(size_t)(E - 1) * 4 + 3] == (float)((E - 1) * 100 + 3) && dec[(size_t)E - 1] == (int32_t)((E - 1) % 4));
  }
  g_write_pattern = false;
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
}

// the calls either side of the sensing launch: what they derive from the handle and what they refuse
static void test_side_paths() {
  crn_cfg cfg;
  REQUIRE(crn_cfg_reference(&cfg) == CRN_OK);
  crn_handle *h = nullptr;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  static float buf[2048], state[512];
  // generator: the band lists the kernel draws tones from, and twice the signed centre of every band (bins >= N/2 are negative
  // frequencies; CH1 = bins -16..-2 and 0..15 of CE_Predictive_Node.cpp:173-179)
  int32_t truth[8];
  REQUIRE(crn_synth_fill_device(h, buf, 8, 128, 7, 1e-6f, 0.02f, 8, truth, nullptr) == CRN_OK);
  REQUIRE(g_synth.n_epochs == 8 && g_synth.samples_per_epoch == 128 && g_synth.fft_len == 512 && g_synth.truth == truth);
  REQUIRE(g_synth.active_band0 == 1 && g_synth.n_active == 3);                 // band 0 (the noise-floor band) is never driven
  REQUIRE(std::fabs(g_synth.noise_sigma - std::sqrt(0.5e-6f)) < 1e-9f && std::fabs(g_synth.tone_amp - 0.02f / std::sqrt(8.f)) < 1e-9f);
  const int *bb = g_synth.band_bins_begin, *bins = g_synth.band_bins, *c2 = g_synth.band_c2;
  REQUIRE(bb[0] == 0 && bb[1] == 10 && bb[2] == 41 && bb[3] == 71 && bb[4] == 104);   // NF 10, CH1 31, CH2 30, CH3 33 bins (.cpp:173-191)
  REQUIRE(bins[0] == 300 && bins[9] == 309 && bins[10] == 0 && bins[25] == 15 && bins[26] == 496 && bins[40] == 510 && bins[41] == 55 && bins[103] == 221);
  REQUIRE(c2[0] == (300 - 512) + (309 - 512) && c2[1] == -16 + 15 && c2[2] == 55 + 84 && c2[3] == 189 + 221);
  crn_synth_cfg sc{};
  sc.seed = 1; sc.noise_power = 1e-6f; sc.signal_rms = 0.02f; sc.tones_per_band = 8; sc.n_streams = 2; sc.adc_bits = 16;
  sc.pu_model = CRN_PU_MARKOV_INTENDED; sc.signal_kind = CRN_SIG_OFDM;
  const int pat = g_pattern_launches;
  REQUIRE(crn_synth_fill_device_ex(h, &sc, buf, 8, 128, truth, nullptr) == CRN_OK);
  REQUIRE(g_pattern_launches == pat + 1 && g_synth.epochs_per_stream == 4 && g_synth.adc_scale == 32768.f && g_synth.signal_kind == CRN_SIG_OFDM);
  REQUIRE(crn_synth_fill_device_ex(h, &sc, buf, 8, 128, nullptr, nullptr) == CRN_ERR_ARG);   // Markov models keep their state in d_truth
  REQUIRE(crn_synth_fill_device_ex(h, &sc, buf, 7, 128, truth, nullptr) == CRN_ERR_ARG);     // streams must divide the epochs
  sc.adc_bits = 1;
  REQUIRE(crn_synth_fill_device_ex(h, &sc, buf, 8, 128, truth, nullptr) == CRN_ERR_ARG);
  sc.adc_bits = 0; sc.signal_kind = 99;
  REQUIRE(crn_synth_fill_device_ex(h, &sc, buf, 8, 128, truth, nullptr) == CRN_ERR_ARG);
  // the transform on its own
  REQUIRE(crn_fft_forward_device(h, buf, 3, 364, 0, buf, nullptr) == CRN_OK);
  REQUIRE(g_fft_len == 512 && g_fft.n_frames == 3 && g_fft.L == 364 && g_fft.frame_stride == 364 && g_fft.tw1 != nullptr && g_fft.tw2 != nullptr);
  REQUIRE(crn_fft_forward_device(h, buf, 3, 513, 0, buf, nullptr) == CRN_ERR_ARG);
  REQUIRE(crn_fft_forward_device(h, buf, -1, 512, 0, buf, nullptr) == CRN_ERR_ARG);
  // display rows: the two normalisations (gr-qtgui's dB of |X|^2 / N^2, a PSD over the window's power)
  REQUIRE(crn_monitor_rows_device(h, buf, 4, CRN_MONITOR_GNURADIO, 0.1f, 1, state, nullptr, buf, nullptr) == CRN_OK);
  REQUIRE(g_mon.n == 512 && g_mon.db_domain == 1 && g_mon.first == 1 && std::fabs(g_mon.scale - 1.0f / (512.f * 512.f)) < 1e-12f);
  REQUIRE(crn_monitor_rows_device(h, buf, 4, CRN_MONITOR_PSD, 1.0f, 0, state, buf, nullptr, nullptr) == CRN_OK);
  REQUIRE(g_mon.db_domain == 0 && std::fabs(g_mon.scale - 1.0f / (512.f * 512.f)) < 1e-12f);   // rectangular window: power N
  REQUIRE(crn_monitor_rows_device(h, buf, 4, CRN_MONITOR_PSD, 0.0f, 0, state, buf, nullptr, nullptr) == CRN_ERR_ARG);
  REQUIRE(crn_monitor_rows_device(h, buf, 4, 7, 0.5f, 0, state, buf, nullptr, nullptr) == CRN_ERR_ARG);
  // noise floor from host features: staged, measured, read back (the stand-in leaves the sum where the kernel leaves its estimate)
  float feats[6 * 4], nf = -1.f;
  for (int i = 0; i < 24; i++) feats[i] = 0.5f;
  REQUIRE(crn_noise_floor_host(h, feats, 6, &nf) == CRN_OK && nf == 12.0f);
  REQUIRE(crn_noise_floor_host(h, feats, 0, &nf) == CRN_ERR_ARG);
  // wire format: full scale, alignment of int16 pairs
  static int16_t wire[64];
  REQUIRE(crn_sense_set_wire_full_scale(h, 8192.0) == CRN_OK && crn_sense_set_wire_full_scale(h, 0.5) == CRN_ERR_ARG);
  REQUIRE(crn_pack_sc16_device(h, buf, 1000, wire, nullptr) == CRN_OK && g_pack_n == 1000 && g_pack_scale == 8192.f);
  const crn_out o = any_outputs();
  REQUIRE(crn_sense_run_device_sc16(h, wire, 3, 364, 0, &o, nullptr) == CRN_OK && g_last_sc16);
  REQUIRE(std::fabs(g_last.wire_unscale - 1.0f / 8192.f) < 1e-12f);   // a sum of magnitudes unscales once, an energy twice
  REQUIRE(crn_sense_run_device_sc16(h, wire + 1, 3, 364, 0, &o, nullptr) == CRN_ERR_ARG);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
  REQUIRE(crn_cfg_energy_scaled(&cfg, 1024, 4.0f) == CRN_OK);
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  REQUIRE(crn_sense_run_device_sc16(h, wire, 1, 1024, 0, &o, nullptr) == CRN_OK && std::fabs(g_last.wire_unscale - 1.0f / (32768.f * 32768.f)) < 1e-18f);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
  // a Hann monitor handle: the PSD normalisation uses the window's power (N x 3/8)
  REQUIRE(crn_cfg_welch(&cfg, 4096, 8, 64) == CRN_OK);
  for (int b = 0; b < 64; b++) cfg.thresh[b] = 1.0f;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  REQUIRE(crn_monitor_rows_device(h, buf, 1, CRN_MONITOR_PSD, 0.5f, 1, state, buf, nullptr, nullptr) == CRN_OK);
  REQUIRE(std::fabs(g_mon.scale * (4096.0 * 4096.0 * 0.375) - 1.0) < 1e-6);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
}

// Round-5 hardening of the handle: the LDS budget comes from the device, updates refuse a capturing stream, more updates
// in flight than staging slots do not corrupt anything, a windowed handle has its one dealt form.
static void test_device_limits_and_updates() {
  crn_cfg cfg;
  crn_handle *h = nullptr;
  const crn_out o = any_outputs();
  // a device (or partition) with 64 KiB of LDS per workgroup: ten 512-point |X| frames need 70 KiB of slots -> no dealt form, the streaming kernel
  g_fake_hip_lds_bytes = 64 * 1024;
  REQUIRE(crn_cfg_reference(&cfg) == CRN_OK && crn_sense_create(&cfg, &h) == CRN_OK);
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 364, 0, &o, nullptr) == CRN_OK);
  REQUIRE(g_last.deal_rounds == 0);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
  // the budget the rule is handed is the device's figure, to the byte: the dealt launch of this handle needs 8 x 16 x 34 x 8 (exchange
  // buffers) + 32 x 8 (pass-2 twiddles) + 3136 (the close's share) + 2 x 8 x 512 x 4 (frame slots) = 70976 bytes
  for (int budget : {70975, 70976}) {
    g_fake_hip_lds_bytes = budget;
    REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
    REQUIRE(crn_sense_run_device(h, g_iq, 1, 364, 0, &o, nullptr) == CRN_OK);
    REQUIRE(g_last.deal_rounds == (budget == 70976 ? 2 : 0));
    REQUIRE(crn_sense_destroy(h) == CRN_OK);
  }
  g_fake_hip_lds_bytes = 160 * 1024;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 364, 0, &o, nullptr) == CRN_OK);
  REQUIRE(g_last.deal_rounds == 2);      // ten frames over eight lane groups
  // crn_sense_dealt_launches counts the form that RAN: a dealt launch the device refuses (hipErrorLaunchOutOfResources inside
  // launch_sense, which then launches the streaming kernel) is a launch, not a dealt launch
  int64_t n_dealt = 0;
  REQUIRE(crn_sense_dealt_launches(h, &n_dealt) == CRN_OK && n_dealt == 1);
  g_refuse_dealt = true;
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 364, 0, &o, nullptr) == CRN_OK && g_last.deal_rounds == 2);   // asked for ...
  g_refuse_dealt = false;
  REQUIRE(crn_sense_dealt_launches(h, &n_dealt) == CRN_OK && n_dealt == 1);                              // ... but not what ran
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 364, 0, &o, nullptr) == CRN_OK);
  REQUIRE(crn_sense_dealt_launches(h, &n_dealt) == CRN_OK && n_dealt == 2);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
  // windowed handles: the periodic Hann in energy mode on whole frames has a dealt form, a table window and |X| mode have none
  REQUIRE(crn_cfg_welch(&cfg, 1024, 8, 64) == CRN_OK && crn_sense_create(&cfg, &h) == CRN_OK);
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 1024, 0, &o, nullptr) == CRN_OK && g_last.deal_rounds == 2);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
  cfg.window = CRN_WINDOW_BLACKMAN_HARRIS;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 1024, 0, &o, nullptr) == CRN_OK && g_last.deal_rounds == 0);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
  cfg.window = CRN_WINDOW_HANN;
  cfg.mode = CRN_MODE_REF_MAG;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  REQUIRE(crn_sense_run_device(h, g_iq, 1, 1024, 0, &o, nullptr) == CRN_OK && g_last.deal_rounds == 0);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
  // updates on a stream that is being captured into a hipGraph are refused before anything is enqueued; launches are not their business
  REQUIRE(crn_cfg_energy_scaled(&cfg, 1024, 4.0f) == CRN_OK && crn_sense_create(&cfg, &h) == CRN_OK);
  hipStream_t cap = nullptr, other = nullptr;
  REQUIRE(hipStreamCreateWithFlags(&cap, 0) == hipSuccess && hipStreamCreateWithFlags(&other, 0) == hipSuccess);
  g_fake_hip_capturing_stream.store(cap);
  float thr[4] = {9.f, 8.f, 7.f, 6.f}, nf = 0.f, feats[2 * 4] = {1, 1, 1, 1, 1, 1, 1, 1};
  REQUIRE(crn_sense_set_thresholds(h, thr, 4, cap) == CRN_ERR_STATE && std::strstr(crn_last_error(), "captured") != nullptr);
  REQUIRE(crn_sense_reserve_noise_floor(h) == CRN_OK);
  REQUIRE(crn_sense_calibrate_thresholds(h, feats, 2, 4.0f, &nf, cap) == CRN_ERR_STATE);
  REQUIRE(crn_sense_set_thresholds(h, thr, 4, other) == CRN_OK);               // another stream: fine
  REQUIRE(crn_sense_run_device(h, g_iq, 2, 1024, 0, &o, cap) == CRN_OK);       // a launch on the capturing stream: fine
  g_fake_hip_capturing_stream.store(nullptr);
  // 40 updates back to back, more than the 8 staging slots: every one lands, the last one's values are the table's
  for (int i = 0; i < 40; i++) {
    for (int b = 0; b < 4; b++) thr[b] = 100.f * i + b;
    REQUIRE(crn_sense_set_thresholds(h, thr, 4, other) == CRN_OK);
  }
  REQUIRE(crn_sense_run_device(h, g_iq, 2, 1024, 0, &o, other) == CRN_OK);
  REQUIRE(g_last.thresh[0] == 3900.f && g_last.thresh[3] == 3903.f);
  REQUIRE(reinterpret_cast<const float *>(g_last.band_tab + 416)[2] == 3902.f);
  // all eight staging slots in flight, so the ninth update lets go of the tables' lock while it waits for the oldest — and in
  // that window another thread's crn_sense_set_bands swaps the plan for one of three bands.  The update must notice (CRN_ERR_STATE) and
  // write nothing: the new plan keeps the thresholds it came with.
  g_fake_gpu_latency_ns.store(30 * 1000 * 1000);
  for (int i = 0; i < 8; i++) REQUIRE(crn_sense_set_thresholds(h, thr, 4, other) == CRN_OK);
  static crn_handle *s_h;
  static int s_rc;
  s_h = h;
  s_rc = -1;
  g_fake_hip_on_event_sync = [] {
    g_fake_hip_on_event_sync = nullptr;
    const crn_band_seg segs[3] = {{8, 24, 0}, {40, 72, 1}, {100, 140, 2}};
    const float t3[3] = {11.f, 12.f, 13.f};
    s_rc = crn_sense_set_bands(s_h, segs, 3, 3, t3);
  };
  for (int b = 0; b < 4; b++) thr[b] = 7000.f + b;
  REQUIRE(crn_sense_set_thresholds(h, thr, 4, other) == CRN_ERR_STATE && std::strstr(crn_last_error(), "band plan changed") != nullptr);
  REQUIRE(s_rc == CRN_OK && g_fake_hip_on_event_sync == nullptr);
  g_fake_gpu_latency_ns.store(0);
  REQUIRE(crn_sense_run_device(h, g_iq, 2, 1024, 0, &o, other) == CRN_OK);
  REQUIRE(g_last.n_bands == 3 && g_last.thresh[0] == 11.f && g_last.thresh[2] == 13.f);
  REQUIRE(reinterpret_cast<const float *>(g_last.band_tab + 416)[1] == 12.f);
  (void)hipStreamDestroy(cap);
  (void)hipStreamDestroy(other);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);
}

int main() {
  for (int N : {512, 1024, 2048, 4096}) {
    test_tables(N, true);
    test_tables(N, false);
  }
  test_windows();
  test_geometry();
  test_arguments_and_counters();
  test_run_host();
  test_side_paths();
  test_device_limits_and_updates();
  if (g_failed) {
    std::fprintf(stderr, "api_unit: %d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("api_unit: tables (4 sizes x 2 plans), windows, launch geometry (5 CU counts x 4 sizes x 4 K x 21 batch sizes + Welch), arguments, live updates, host-buffer staging, side paths, device limits and update staging: ok\n");
  return 0;
}
