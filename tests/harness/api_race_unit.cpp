// TEST INFRASTRUCTURE: live updates of a handle against launches from another thread, without a GPU.  The handle's host files (Makefile: API_SRCS) +
// crn_ingest.cpp as they are over tests/harness/fake_hip; built twice — ThreadSanitizer and AddressSanitizer (Makefile).
//   thread A (the "CE thread"): pushes packets through a real ingest ring, whose launcher thread calls crn_sense_run_device
//   thread B (the handle's owner): crn_sense_set_bands (same number of bands), crn_sense_set_thresholds, crn_sense_set_ann in a loop
// The launch stand-in reads what a kernel reads through the pointers in its parameter block — the packed band table, the twiddles,
// the thresholds — and checks that the plan it sees is ONE of the plans thread B installs, whole (never a mix of two, never a freed
// slab: under ASan a stale pointer is a report, under TSan an unlocked field is one).  Reference for why this matters: execute()
// runs with CE_mutex held while the rx thread keeps pushing (src/extensible_cognitive_radio.cpp:1310-1324, 1792-1803).
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/crn_sense.h"
#include "../../include/crn_sense_sc16.h"
#include "../../cognitive-radio-network_amd/csrc/crn_forms.h"

std::atomic<long long> g_fake_gpu_latency_ns{0};

static std::atomic<long long> g_launches{0}, g_mixed{0}, g_plan_seen[2];

namespace crn {
hipError_t launch_sense(const SenseParams &p, int fft_len, bool, bool, int, hipStream_t, bool, int *deal_rounds_run) {
  if (deal_rounds_run) *deal_rounds_run = p.deal_rounds;
  // the plan as a kernel would find it: band 1's first segment (lo, hi) from the packed table, the segment tables, the thresholds
  const int sb = p.band_tab[1];                       // band_seg_begin[1]
  const int lo = p.band_tab[96 + sb], hi = p.band_tab[256 + sb];
  const int lo2 = p.seg_lo[p.band_seg_begin[1]], hi2 = p.seg_hi[p.band_seg_begin[1]];
  float thr;
  std::memcpy(&thr, &p.band_tab[416 + 1], sizeof(thr));
  const float2 w = p.tw1[fft_len / 16 + 1];           // a twiddle from the same slab
  const bool plan_a = lo == 8 && hi == 24, plan_b = lo == 40 && hi == 72;
  if (!(plan_a || plan_b) || lo != lo2 || hi != hi2 || !(w.x > 0.9f) || !(thr == p.thresh[1])) g_mixed++;
  g_plan_seen[plan_b ? 1 : 0]++;
  for (long long e = 0; e < p.n_epochs; e++) {
    if (p.decision) p.decision[e] = 1;
    if (p.features) p.features[e * p.n_bands] = thr;
  }
  g_launches++;
  return hipSuccess;
}
std::atomic<long long> g_warm{0};
}
std::atomic<long> g_pauses{0};
namespace crn {
hipError_t launch_nop(hipStream_t) { g_warm++; return hipSuccess; }   // crn_sense_warm_stream: the launcher thread's empty launch at a pre-wake
hipError_t launch_fft(const FftParams &, int, hipStream_t) { return hipSuccess; }
hipError_t launch_monitor(const MonitorParams &, hipStream_t) { return hipSuccess; }
hipError_t launch_noise_floor(const float *feat, int n, int nb, float *scratch, hipStream_t) {
  scratch[kNoiseFloorMaxEpochs] = feat[(long long)n * nb - 1];
  return hipSuccess;
}
hipError_t launch_synth(const SynthParams &, hipStream_t) { return hipSuccess; }
hipError_t launch_pack_sc16(const float *, long long, short *, float, hipStream_t) { return hipSuccess; }
hipError_t launch_pu_pattern(const SynthParams &, hipStream_t) { return hipSuccess; }
}  // namespace crn

#define REQUIRE(c)                                                                \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::fprintf(stderr, "api_race_unit: line %d: %s FAILED (%s)\n", __LINE__, #c, crn_last_error()); \
      std::exit(1);                                                               \
    }                                                                             \
  } while (0)

int main() {
  crn_cfg cfg;
  REQUIRE(crn_cfg_energy_scaled(&cfg, 1024, 4.0f) == CRN_OK);
  const crn_band_seg plan_a[4] = {{600, 620, 0}, {8, 24, 1}, {110, 170, 2}, {378, 444, 3}};
  const crn_band_seg plan_b[4] = {{600, 620, 0}, {40, 72, 1}, {110, 170, 2}, {378, 444, 3}};
  std::memcpy(cfg.segs, plan_a, sizeof(plan_a));
  cfg.n_segs = 4;
  crn_handle *h = nullptr;
  REQUIRE(crn_sense_create(&cfg, &h) == CRN_OK);
  crn_ingest *g = nullptr;
  REQUIRE(crn_ingest_create(h, 2, 256, 2, &g) == CRN_OK);
  REQUIRE(crn_sense_destroy(h) == CRN_ERR_STATE);      // a ring is attached: the handle stays (its launcher thread launches through it)

  std::atomic<bool> stop{false}, slow{false};
  std::thread pusher([&] {
    std::vector<float> pkt(256 * 2, 0.5f);
    crn_epoch_result r[8];
    int32_t n = 0;
    long pushed = 0;
    int64_t paused_at = -1;
    while (!stop.load()) {
      // second phase: a pause after every batch, so that the ring's stream sits idle for more than 2 ms and the next batch's pre-wake makes
      // the launcher thread call crn_sense_warm_stream (which reads the handle's device without the lock) while the plan is being swapped
      // (the pause follows a hand-off — the ring's batch counter moved — so it falls between two batches whatever phase the two streams are in)
      if (slow.load()) {
        crn_ingest_stats st;
        if (crn_ingest_get_stats(g, &st) == CRN_OK && st.batches != paused_at) {
          paused_at = st.batches;
          g_pauses++;
          std::this_thread::sleep_for(std::chrono::milliseconds(8));
        }
      }
      for (int s = 0; s < 2; s++) {
        const int rc = crn_ingest_push(g, s, pkt.data());
        pushed += rc == CRN_OK;
        // ... and packets come at a radio's pace in that phase (the pre-wake is ten packet times ahead of the hand-off: pushed back to
        // back, the hand-off overtakes the launcher thread's wake-up and clears the hint before it is seen)
        if (slow.load()) std::this_thread::sleep_for(std::chrono::microseconds(40));
        if (rc == CRN_ERR_BUSY) (void)crn_ingest_wait(g);
        else if (rc != CRN_OK) { std::fprintf(stderr, "push: %s\n", crn_last_error()); std::exit(1); }
      }
      if (crn_ingest_poll(g, r, 8, &n) != CRN_OK) { std::fprintf(stderr, "poll: %s\n", crn_last_error()); std::exit(1); }
    }
  });
  double w_ih[5][6], w_ho[6][4];
  std::memset(w_ih, 0, sizeof(w_ih));
  std::memset(w_ho, 0, sizeof(w_ho));
  int updates = 0;
  for (int it = 0; it < 400 || g_plan_seen[0].load() < 20 || g_plan_seen[1].load() < 20; it++) {
    const bool b = it & 1;
    REQUIRE(crn_sense_set_bands(h, b ? plan_b : plan_a, 4, 4, nullptr) == CRN_OK);
    float thr[4] = {1.f + it, 2.f + it, 3.f + it, 4.f + it};
    REQUIRE(crn_sense_set_thresholds(h, thr, 4, nullptr) == CRN_OK);       // (9 per pass of the staging ring's 8 slots: slots are reused)
    REQUIRE(crn_sense_set_ann(h, w_ih, w_ho, 0.8, nullptr) == CRN_ERR_STATE);   // a threshold handle: refused under the lock too
    crn_sense_stats st;
    REQUIRE(crn_sense_get_stats(h, &st) == CRN_OK);
    updates++;
    if (it > 200000) break;
    std::this_thread::yield();
  }
  slow.store(true);
  const long long warm_before = crn::g_warm.load();
  const auto t_slow = std::chrono::steady_clock::now();
  for (int it = 0; crn::g_warm.load() < warm_before + 8 && std::chrono::steady_clock::now() - t_slow < std::chrono::seconds(20); it++) {
    REQUIRE(crn_sense_set_bands(h, (it & 1) ? plan_b : plan_a, 4, 4, nullptr) == CRN_OK);
    REQUIRE(crn_sense_synchronize(h, nullptr) == CRN_OK);    // (reads the device field too)
    std::this_thread::sleep_for(std::chrono::microseconds(200));   // (std::mutex is not fair: leave the launcher thread a turn at the handle)
  }
  if (crn::g_warm.load() < warm_before + 8) {
    crn_ingest_stats st;
    (void)crn_ingest_get_stats(g, &st);
    std::fprintf(stderr, "DEBUG warm %lld -> %lld; batches %lld packets %lld dropped %lld epochs_ready %lld pauses %ld\n", warm_before, crn::g_warm.load(),
                 (long long)st.batches, (long long)st.packets, (long long)st.dropped, (long long)st.epochs_ready, g_pauses.load());
  }
  REQUIRE(crn::g_warm.load() >= warm_before + 8);            // the pre-wake's warm-up launches did run against the swaps
  slow.store(false);
  // a change of the number of bands is refused while the ring is attached (its result buffers were sized for 4)
  const crn_band_seg three[3] = {{600, 620, 0}, {8, 24, 1}, {110, 170, 2}};
  const float thr3[3] = {1, 2, 3};
  REQUIRE(crn_sense_set_bands(h, three, 3, 3, thr3) == CRN_ERR_STATE);
  stop.store(true);
  pusher.join();
  REQUIRE(crn_ingest_drain(g) == CRN_OK);
  REQUIRE(crn_ingest_destroy(g) == CRN_OK);
  REQUIRE(g_mixed.load() == 0 && g_launches.load() > 40 && g_plan_seen[0].load() >= 20 && g_plan_seen[1].load() >= 20);
  REQUIRE(crn_sense_destroy(h) == CRN_OK);             // ... and goes once the ring is gone
  std::printf("api_race_unit: %lld launches from the ring's launcher thread against %d band-plan + threshold updates (%lld saw plan A, %lld plan B, "
              "0 saw a mix): ok\n", g_launches.load(), updates, g_plan_seen[0].load(), g_plan_seen[1].load());
  return 0;
}
