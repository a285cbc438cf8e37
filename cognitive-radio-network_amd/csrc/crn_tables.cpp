// crn_tables.cpp — what a handle keeps in HBM for its configuration: the rules a configuration must meet and the builder of the table slab.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "crn_handle.h"
#include "crn_kernels.h"

static_assert(crn::kTabSegBeginWords >= CRN_MAX_BANDS + 1 && crn::kTabSegWords >= CRN_MAX_SEGS && crn::kTabThreshWords >= CRN_MAX_BANDS,
              "band_tab: the band plan's regions hold the largest plan");
static_assert(crn::kTabWihWords * sizeof(int) == sizeof(crn_cfg::ann_w_ih) && sizeof(crn_cfg::ann_w_ih) == 30 * sizeof(double) &&
              crn::kTabWhoWords * sizeof(int) == sizeof(crn_cfg::ann_w_ho) && sizeof(crn_cfg::ann_w_ho) == 24 * sizeof(double),
              "band_tab: the weight regions hold 30 and 24 doubles");

// exp(-2 pi j q / n) with the angle index reduced exactly and the trig done in double.
static float2 twiddle(long long q, int n) {
  q %= n;
  const double ang = -2.0 * M_PI * (double)q / (double)n;
  return make_float2((float)std::cos(ang), (float)std::sin(ang));
}

int crn::validate(const crn_cfg *c) {
  if (!c) return crn::fail(CRN_ERR_ARG, "null cfg");
  if (c->abi_version != CRN_ABI_VERSION) return crn::fail(CRN_ERR_ARG, "cfg.abi_version mismatch");
  if (const int n = c->fft_len; n != 512 && n != 1024 && n != 2048 && n != 4096) return crn::fail(CRN_ERR_ARG, "fft_len must be 512, 1024, 2048 or 4096");
  if (c->frames_per_epoch < 1) return crn::fail(CRN_ERR_ARG, "frames_per_epoch < 1");
  if (c->hop < 1 || c->hop > c->fft_len) return crn::fail(CRN_ERR_ARG, "hop out of range");
  if (c->mode != CRN_MODE_REF_MAG && c->mode != CRN_MODE_ENERGY) return crn::fail(CRN_ERR_ARG, "bad mode");
  if (c->decide < CRN_DECIDE_ANN || c->decide > CRN_DECIDE_NONE) return crn::fail(CRN_ERR_ARG, "bad decide");
  if (c->window < CRN_WINDOW_RECT || c->window > CRN_WINDOW_BLACKMAN_HARRIS) return crn::fail(CRN_ERR_ARG, "bad window");
  if (c->n_bands < 1 || c->n_bands > CRN_MAX_BANDS) return crn::fail(CRN_ERR_ARG, "n_bands out of range");
  if (c->n_segs < 1 || c->n_segs > CRN_MAX_SEGS) return crn::fail(CRN_ERR_ARG, "n_segs out of range");
  for (int s = 0; s < c->n_segs; s++) {
    const crn_band_seg &g = c->segs[s];
    if (g.lo < 0 || g.hi > c->fft_len || g.lo > g.hi || g.band < 0 || g.band >= c->n_bands)
      return crn::fail(CRN_ERR_ARG, "band segment " + std::to_string(s) + " out of range");
  }
  if (c->decide == CRN_DECIDE_ANN && c->n_bands != 4)
    return crn::fail(CRN_ERR_ARG, "DECIDE_ANN needs exactly 4 bands {NF, CH1, CH2, CH3}");
  if (c->decide == CRN_DECIDE_THRESHOLD && c->ref_band >= c->n_bands)
    return crn::fail(CRN_ERR_ARG, "ref_band out of range");
  return CRN_OK;
}

// Everything a handle keeps in HBM for the configuration `cfg`, built into one fresh slab (crn_sense_create, and again by
// crn_sense_set_bands on a live handle): twiddles, window, the band plan in its three forms, thresholds, ANN weights.  The handle is
// written last, once the slab is on the device: on any failure it is untouched (a live handle keeps its old plan).  tables_mu is held.
int crn::build_tables(crn_handle *h, const crn_cfg &cfg) {
  const int N = cfg.fft_len, R3 = N / 256, T = N / 16;
  std::vector<float2> tw1((size_t)17 * T), tw2((size_t)16 * R3);  // row 16 of tw1: W_N^{16 t}
  for (int i = 0; i < 16; i++)
    for (int t = 0; t < T; t++) tw1[(size_t)i * T + t] = twiddle((long long)i * t, N);
  for (int t = 0; t < T; t++) tw1[(size_t)16 * T + t] = twiddle(16LL * t, N);
  for (int i = 0; i < 16; i++)
    for (int m = 0; m < R3; m++) tw2[(size_t)i * R3 + m] = twiddle((long long)i * m, T);
  std::vector<float> win(N, 1.0f);
  if (cfg.window == CRN_WINDOW_HANN)
    for (int n = 0; n < N; n++) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)N));
  if (cfg.window == CRN_WINDOW_BLACKMAN_HARRIS)
    for (int n = 0; n < N; n++) {
      const double x = 2.0 * M_PI * (double)n / (double)(N - 1);
      win[n] = (float)(0.35875 - 0.48829 * std::cos(x) + 0.14128 * std::cos(2 * x) - 0.01168 * std::cos(3 * x));
    }

  double window_power = 0.0;
  for (int n = 0; n < N; n++) window_power += (double)win[n] * (double)win[n];

  // segments grouped by band, table order kept inside a band (the reference sums CH1's two runs in table order, CE_Predictive_Node.cpp:173-179)
  std::vector<int> seg_begin(cfg.n_bands + 1, 0), seg_lo, seg_hi, bins_begin(cfg.n_bands + 1, 0), bins;
  for (int b = 0; b < cfg.n_bands; b++) {
    seg_begin[b] = (int)seg_lo.size();
    bins_begin[b] = (int)bins.size();
    for (int s = 0; s < cfg.n_segs; s++)
      if (cfg.segs[s].band == b) {
        seg_lo.push_back(cfg.segs[s].lo);
        seg_hi.push_back(cfg.segs[s].hi);
        for (int k = cfg.segs[s].lo; k < cfg.segs[s].hi; k++) bins.push_back(k);
      }
  }
  unsigned acc_mask = 0;
  {
    // bin k sits in register j R3 + d of its thread: d = k / 256, j = ((k % 256) / 16) mod J (crn_frame.h, pass 3)
    const int J = 16 / R3;
    for (int sgi = 0; sgi < cfg.n_segs; sgi++)
      for (int k = cfg.segs[sgi].lo; k < cfg.segs[sgi].hi; k++) acc_mask |= 1u << ((((k & 255) >> 4) % J) * R3 + (k >> 8));
  }
  int aligned_shift = 0;
  if (N == 4096 && cfg.n_segs == cfg.n_bands && N % cfg.n_bands == 0 && cfg.decide != CRN_DECIDE_ANN) {
    const int W = N / cfg.n_bands;
    bool ok = W == 64 || W == 128 || W == 256;
    for (int b = 0; ok && b < cfg.n_bands; b++)
      ok = cfg.segs[b].band == b && cfg.segs[b].lo == b * W && cfg.segs[b].hi == (b + 1) * W;
    if (ok) aligned_shift = W == 64 ? 6 : W == 128 ? 7 : 8;
  }
  seg_begin[cfg.n_bands] = (int)seg_lo.size();
  bins_begin[cfg.n_bands] = (int)bins.size();
  if (bins.empty()) bins.push_back(0);

  // packed band table for the kernel's LDS copy (layout: crn_kernels.h)
  std::vector<int> band_tab(crn::kBandTabWords, 0);
  for (size_t i = 0; i < seg_begin.size(); i++) band_tab[crn::kTabSegBegin + i] = seg_begin[i];
  for (size_t i = 0; i < seg_lo.size(); i++) {
    band_tab[crn::kTabSegLo + i] = seg_lo[i];
    band_tab[crn::kTabSegHi + i] = seg_hi[i];
  }
  std::memcpy(&band_tab[crn::kTabThresh], cfg.thresh, sizeof(float) * CRN_MAX_BANDS);
  std::memcpy(&band_tab[crn::kTabWih], cfg.ann_w_ih, sizeof(cfg.ann_w_ih));  // 30 doubles
  std::memcpy(&band_tab[crn::kTabWho], cfg.ann_w_ho, sizeof(cfg.ann_w_ho));  // 24 doubles
  // Row entries for the register-resident band sums (epoch_close): every thread's accumulators sit at bins base + 256 d, so a segment is
  // cut at the 256-bin rows and each piece becomes (row d, band, [lo, hi) inside the row), grouped by row, band-table order kept inside a
  // row.  Only small plans qualify (<= 16 bands, <= 32 / R3 pieces per row); the others keep the LDS walk.
  int n_row_entries = 0;
  {
    struct RowPiece { int d, band, lo, hi; };
    std::vector<RowPiece> pieces;
    for (int b = 0; b < cfg.n_bands; b++)
      for (int sg = seg_begin[b]; sg < seg_begin[b + 1]; sg++)
        for (int d = seg_lo[sg] >> 8; seg_lo[sg] < seg_hi[sg] && d <= (seg_hi[sg] - 1) >> 8; d++) {
          const int lo = std::max(seg_lo[sg], 256 * d) - 256 * d, hi = std::min(seg_hi[sg], 256 * (d + 1)) - 256 * d;
          pieces.push_back({d, b, lo, hi});
        }
    // fixed layout, no walk: row d owns words [kTabRowEntries + d * cap, kTabRowEntries + (d + 1) * cap), cap = 32 / R3; an unused slot is 0 (span 0)
    const int cap = crn::kRowEntryWords / R3;
    bool fits = cfg.n_bands <= 16 && !pieces.empty();
    std::vector<int> used(16, 0);
    for (const RowPiece &pc : pieces)
      if (++used[pc.d] > cap) fits = false;
    if (fits) {
      std::fill(used.begin(), used.end(), 0);
      for (const RowPiece &pc : pieces) band_tab[crn::kTabRowEntries + pc.d * cap + used[pc.d]++] = (pc.band << 18) | (pc.lo << 9) | pc.hi;
      n_row_entries = (int)pieces.size();
    }
  }

  // The same once more for the kernels whose register rows start kTw1cRowShift bins early (crn_kernels.h: bin_of — the plain 4096-point
  // forms): every segment moved up by the shift, wrapped at N, cut at the 256-bin rows of THAT numbering; lo / hi count from the row's
  // start, i.e. they are the lane coordinates (lane_coord) the kernel compares.  A table of its own: the entries above stay what every
  // other kernel reads.  Band order, table order inside a band, a wrapped segment's upper part first.
  std::vector<int> row_entries_shift(crn::kRowEntryWords, 0);
  int n_row_entries_shift = 0;
  unsigned acc_mask_shift = 0;
  {
    const int S = crn::kTw1cRowShift, J = 16 / R3, cap = crn::kRowEntryWords / R3;
    struct RowPiece { int d, band, lo, hi; };
    std::vector<RowPiece> pieces;
    auto cut = [&](int band, int lo, int hi) {   // [lo, hi) in shifted numbering, inside [0, N)
      for (int d = lo >> 8; lo < hi && d <= (hi - 1) >> 8; d++)
        pieces.push_back({d, band, std::max(lo, 256 * d) - 256 * d, std::min(hi, 256 * (d + 1)) - 256 * d});
    };
    for (int b = 0; b < cfg.n_bands; b++)
      for (int sg = seg_begin[b]; sg < seg_begin[b + 1]; sg++) {
        const int lo = seg_lo[sg] + S, hi = seg_hi[sg] + S;
        cut(b, std::min(lo, N), std::min(hi, N));
        cut(b, std::max(lo, N) - N, std::max(hi, N) - N);
        for (int k = seg_lo[sg]; k < seg_hi[sg]; k++) {
          const int ks = (k + S) & (N - 1);
          acc_mask_shift |= 1u << ((((ks & 255) >> 4) % J) * R3 + (ks >> 8));
        }
      }
    bool fits = cfg.n_bands <= 16 && !pieces.empty();
    std::vector<int> used(16, 0);
    for (const RowPiece &pc : pieces)
      if (++used[pc.d] > cap) fits = false;
    if (fits) {
      std::fill(used.begin(), used.end(), 0);
      for (const RowPiece &pc : pieces) row_entries_shift[pc.d * cap + used[pc.d]++] = (pc.band << 18) | (pc.lo << 9) | pc.hi;
      n_row_entries_shift = (int)pieces.size();
    }
  }

  // twice the signed centre of every band (bins >= N / 2 are negative frequencies; lowest + highest signed bin, so a band with a
  // small gap in it — the reference plan's CH1 skips bins -1, -2 — is centred on its span): the carrier of the generator's
  // modulated signal kinds
  std::vector<int> band_c2(std::max(cfg.n_bands, 1), 0);
  for (int b = 0; b < cfg.n_bands; b++) {
    int lo = N, hi = -N;
    for (int i = bins_begin[b]; i < bins_begin[b + 1]; i++) {
      const int k = bins[i] >= N / 2 ? bins[i] - N : bins[i];
      lo = std::min(lo, k);
      hi = std::max(hi, k);
    }
    band_c2[b] = bins_begin[b + 1] > bins_begin[b] ? lo + hi : 0;
  }

  struct SlabPart { const void *src; size_t bytes; size_t off; };
  std::vector<SlabPart> parts = {
      {tw1.data(), tw1.size() * sizeof(float2), 0},
      {tw2.data(), tw2.size() * sizeof(float2), 0},
      {win.data(), win.size() * sizeof(float), 0},
      {cfg.thresh, sizeof(float) * CRN_MAX_BANDS, 0},
      {seg_begin.data(), seg_begin.size() * sizeof(int), 0},
      {seg_lo.data(), seg_lo.size() * sizeof(int), 0},
      {seg_hi.data(), seg_hi.size() * sizeof(int), 0},
      {bins_begin.data(), bins_begin.size() * sizeof(int), 0},
      {bins.data(), bins.size() * sizeof(int), 0},
      {cfg.ann_w_ih, sizeof(cfg.ann_w_ih), 0},
      {cfg.ann_w_ho, sizeof(cfg.ann_w_ho), 0},
      {band_tab.data(), band_tab.size() * sizeof(int), 0},
      {band_c2.data(), band_c2.size() * sizeof(int), 0},
      {row_entries_shift.data(), row_entries_shift.size() * sizeof(int), 0},
  };
  size_t total = 0;
  for (auto &p : parts) {
    p.off = total;
    total = align_up(total + p.bytes, 256);
  }
  std::vector<char> host(total, 0);
  for (auto &p : parts) std::memcpy(host.data() + p.off, p.src, p.bytes);
  void *slab = nullptr;
  hipError_t e = hipMalloc(&slab, total);
  if (e != hipSuccess) return crn::fail(CRN_ERR_NOMEM, std::string("hipMalloc(tables): ") + hipGetErrorString(e));
  e = hipMemcpy(slab, host.data(), total, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(slab);
    return crn::fail(CRN_ERR_DEVICE, std::string("hipMemcpy(tables): ") + hipGetErrorString(e));
  }
  // hipFree waits for the device: launches still reading the previous slab (crn_sense_set_bands on a live handle) finish first
  if (h->d_tables) (void)hipFree(h->d_tables);
  h->cfg = cfg;
  h->window_power = window_power;
  h->aligned_shift = aligned_shift;
  h->n_row_entries = n_row_entries;
  h->acc_mask = acc_mask;
  h->n_row_entries_shift = n_row_entries_shift;
  h->acc_mask_shift = acc_mask_shift;
  h->d_tables = slab;
  char *base = static_cast<char *>(h->d_tables);
  h->d_tw1 = reinterpret_cast<const float2 *>(base + parts[0].off);
  h->d_tw2 = reinterpret_cast<const float2 *>(base + parts[1].off);
  h->d_window = reinterpret_cast<const float *>(base + parts[2].off);
  h->d_thresh = reinterpret_cast<const float *>(base + parts[3].off);
  h->d_band_seg_begin = reinterpret_cast<const int *>(base + parts[4].off);
  h->d_seg_lo = reinterpret_cast<const int *>(base + parts[5].off);
  h->d_seg_hi = reinterpret_cast<const int *>(base + parts[6].off);
  h->d_band_bins_begin = reinterpret_cast<const int *>(base + parts[7].off);
  h->d_band_bins = reinterpret_cast<const int *>(base + parts[8].off);
  h->d_wih = reinterpret_cast<const double *>(base + parts[9].off);
  h->d_who = reinterpret_cast<const double *>(base + parts[10].off);
  h->d_band_tab = reinterpret_cast<const int *>(base + parts[11].off);
  h->d_band_c2 = reinterpret_cast<const int *>(base + parts[12].off);
  h->d_row_entries_shift = reinterpret_cast<const int *>(base + parts[13].off);
  return CRN_OK;
}
