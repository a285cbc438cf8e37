// crn_tracks.hip — emitter segments linked across epochs into tracks (crn_tracks_device, include/crn_sense.h): the two arrays
// crn_segments_device wrote become, per stream, an ordered list of tracks.  Tracks are the connected components of the link graph, so
// every epoch works at once; nothing here steps through time.
//
// Node (e, s) has the index e * max_segments + s.  Seven small launches on the caller's stream, all scratch in the caller's workspace
// (parent [nodes] int32, one 64-byte accumulator per node, two int32 per epoch):
//   1. init      parent[i] = i and a cleared accumulator for every stored node, -1 for the empty slots;
//   2. link      a wave per epoch e: its segments (lo, width) in LDS, then for each d = 1 .. max_miss + 1 the stored segments of epoch
//                e + d in LDS; lane a walks them (a broadcast read each) and unites on every hit.  The union is lock-free and leaves the
//                smallest index of a component as its root: crn_track_link.h has it, with the argument why it is safe;
//   3. gather    a wave per epoch: every node is flattened to its root (parent[i] = root, written with atomicMin like this pass's
//                halving, so that a slower lane's halving of the same node cannot put an older ancestor back) and adds itself to the root's accumulator
//                (integer atomics: exact in any order; the two fp64 sums with fp64 atomic adds).  One node per (epoch, root), settled
//                among the wave's lanes through LDS, adds to n_epochs_hit;
//   4. count     a wave per epoch: the roots of that epoch with n_epochs_hit >= min_epochs;
//   5. scan      a workgroup per stream: exclusive add scan of those counts over the stream's epochs, the stream's header, zeros in
//                the track slots nobody will fill;
//   6. emit      a wave per epoch: its surviving roots get their numbers (ascending root = ascending epoch, then slot) and, below
//                max_tracks, their records;
//   7. labels    d_track_of, one thread per slot (skipped when the caller passes NULL).
// A chain as long as the stream (one solid segment in every epoch) stays short under the halving; the most links (256 alternating
// one-bin segments, max_miss 3, a wide slack) cost finds that end after one or two steps because of the kept root.
// No scratch memory, 4 KiB of LDS at most; every write to memory is a vector store or a vector atomic.
#include "crn_segments.h"
#include "crn_track_link.h"

namespace crn {
namespace {

// what a root gathers from its members; 64 bytes, indexed like parent[]
struct TrackAcc {
  int hits, nseg, last_key, lo_off, hi_off;   // last_key = max of t * S + (S - 1 - s): the latest epoch, there the lowest slot
  unsigned peak;                              // bits of the largest peak_power (>= 0, so unsigned order is float order)
  int number, pad;                            // the track's number in its stream, -1 when dropped (written by emit)
  unsigned long long width_sum;
  double power, moment;                       // sum P, sum P (off + centroid)
  long long pad2;
};
static_assert(sizeof(TrackAcc) == 64, "workspace layout");

struct TrkParams {
  const crn_segment_epoch *epochs;
  const crn_segment *segments;
  crn_track_stream *streams;
  crn_track *tracks;
  int *track_of;
  int *parent;
  TrackAcc *acc;
  int *count, *base;   // per epoch: surviving roots, and their exclusive scan within the stream
  long long n_epochs;
  int n, S, eps, slack, max_miss, min_epochs, max_tracks;
};

__device__ __forceinline__ int stored(const TrkParams &p, long long e) {
  const int ns = p.epochs[e].n_stored;
  return ns < 0 ? 0 : ns > p.S ? p.S : ns;
}

__global__ __launch_bounds__(256) void tracks_init_kernel(const TrkParams p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n_epochs * p.S) return;
  const long long e = i / p.S;
  const int s = (int)(i - e * p.S);
  if (s >= stored(p, e)) {
    p.parent[i] = -1;
    return;
  }
  p.parent[i] = (int)i;
  TrackAcc a;
  a.hits = 0;
  a.nseg = 0;
  a.last_key = -1;
  a.lo_off = 0x7fffffff;
  a.hi_off = -0x7fffffff - 1;
  a.peak = 0;
  a.number = -1;
  a.pad = 0;
  a.width_sum = 0;
  a.power = 0.0;
  a.moment = 0.0;
  a.pad2 = 0;
  p.acc[i] = a;
}

__global__ __launch_bounds__(64) void tracks_link_kernel(const TrkParams p) {
  __shared__ int2 mine[MAX_SLOTS], next[MAX_SLOTS];   // (lo, width)
  const int l = threadIdx.x;
  const long long e = blockIdx.x;
  const int na = stored(p, e);
  if (na == 0) return;
  const int t = (int)(e % p.eps);
  for (int s = l; s < na; s += 64) {
    const crn_segment *g = p.segments + e * p.S + s;
    mine[s] = make_int2(g->lo, g->width);
  }
  const int mask = p.n - 1;
  for (int d = 1; d <= p.max_miss + 1 && t + d < p.eps; d++) {
    const int nb = stored(p, e + d);
    __syncthreads();   // the previous round's reads of next[] are over (and mine[] is written)
    for (int s = l; s < nb; s += 64) {
      const crn_segment *g = p.segments + (e + d) * p.S + s;
      next[s] = make_int2(g->lo, g->width);
    }
    __syncthreads();
    link_rows(p.parent, mine, na, (int)(e * p.S), next, nb, (int)((e + d) * p.S), l, mask, p.slack);
  }
}

__global__ __launch_bounds__(64) void tracks_gather_kernel(const TrkParams p) {
  __shared__ int roots[MAX_SLOTS];
  const int l = threadIdx.x;
  const long long e = blockIdx.x;
  const int ns = stored(p, e);
  if (ns == 0) return;
  const int t = (int)(e % p.eps), half = p.n / 2, mask = p.n - 1;
  for (int s = l; s < ns; s += 64) {
    const int i = (int)(e * p.S) + s;
    const int r = find<true>(p.parent, i);
    roots[s] = r;
    if (r != i) atomicMin(p.parent + i, r);
  }
  __syncthreads();
  for (int s = l; s < ns; s += 64) {
    const int r = roots[s];
    const crn_segment g = p.segments[e * p.S + s];
    const int off = wrapped(g.lo, p.segments[r].lo, half, mask);
    bool first = true;   // of this epoch's members of r
    for (int j = 0; j < s; j++) first = first && roots[j] != r;
    add_member(p.acc + r, g, off, first, t, s, p.S);
  }
}

__device__ __forceinline__ bool survives(const TrkParams &p, int i) { return p.parent[i] == i && p.acc[i].hits >= p.min_epochs; }

__global__ __launch_bounds__(64) void tracks_count_kernel(const TrkParams p) {
  const int l = threadIdx.x;
  const long long e = blockIdx.x;
  const int ns = stored(p, e);
  int c = 0;
  for (int s0 = 0; s0 < ns; s0 += 64) {
    const int s = s0 + l;
    c += __popcll(__ballot(s < ns && survives(p, (int)(e * p.S) + s)));
  }
  if (l == 0) p.count[e] = c;
}

// one workgroup per stream; thread i owns the epochs [i chunk, (i + 1) chunk) of the stream
__global__ __launch_bounds__(1024) void tracks_scan_kernel(const TrkParams p) {
  __shared__ int wave_sum[16], wave_nodes[16];
  const int i = threadIdx.x, l = i & 63, w = i >> 6;
  const long long e0 = (long long)blockIdx.x * p.eps;
  const long long chunk = ((long long)p.eps + 1023) / 1024;
  const long long lo = i * chunk < p.eps ? i * chunk : p.eps, hi = lo + chunk < p.eps ? lo + chunk : p.eps;
  int sum = 0, nodes = 0;
  for (long long t = lo; t < hi; t++) {
    sum += p.count[e0 + t];
    nodes += stored(p, e0 + t);
  }
  const int incl = wave_scan(sum, l);
#pragma unroll
  for (int s = 32; s > 0; s /= 2) nodes += __shfl_xor(nodes, s, 64);
  if (l == 63) wave_sum[w] = incl;
  if (l == 0) wave_nodes[w] = nodes;
  __syncthreads();
  int before = 0, total = 0, all_nodes = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    before += k < w ? wave_sum[k] : 0;
    total += wave_sum[k];
    all_nodes += wave_nodes[k];
  }
  int run = before + incl - sum;
  for (long long t = lo; t < hi; t++) {
    p.base[e0 + t] = run;
    run += p.count[e0 + t];
  }
  const int n_stored = total < p.max_tracks ? total : p.max_tracks;
  if (i == 0) {
    crn_track_stream h;
    h.n_found = total;
    h.n_stored = n_stored;
    h.n_nodes = all_nodes;
    h.reserved = 0;
    p.streams[blockIdx.x] = h;
  }
  zero_unused(p.tracks + (long long)blockIdx.x * p.max_tracks, n_stored, p.max_tracks, i);
}

__global__ __launch_bounds__(64) void tracks_emit_kernel(const TrkParams p) {
  const int l = threadIdx.x;
  const long long e = blockIdx.x;
  const int ns = stored(p, e);
  if (ns == 0) return;
  const int t = (int)(e % p.eps);
  const long long stream = e / p.eps;
  int number = p.base[e];
  for (int s0 = 0; s0 < ns; s0 += 64) {
    const int s = s0 + l, i = (int)(e * p.S) + s;
    const bool keep = s < ns && survives(p, i);
    const uint64_t kept = __ballot(keep);
    if (keep) {
      const int k = number + __popcll(kept & ((1ull << l) - 1));
      TrackAcc *a = p.acc + i;
      a->number = k;
      if (k < p.max_tracks) {
        const TrackAcc v = *a;
        crn_track o;
        o.first_t = t;
        o.first_slot = s;
        o.last_t = v.last_key / p.S;
        o.last_slot = p.S - 1 - v.last_key % p.S;
        o.n_epochs_hit = v.hits;
        o.n_segments = v.nseg;
        o.lo_off = v.lo_off;
        o.hi_off = v.hi_off;
        o.width_sum = (int64_t)v.width_sum;
        o.power_sum = (float)v.power;
        o.peak_power = __uint_as_float(v.peak);
        o.centre = centre(p.segments[i].lo, v.moment, v.power, p.n);
        o.flags = (t <= p.max_miss ? 1 : 0) | (o.last_t >= p.eps - 1 - p.max_miss ? 2 : 0);
        o.reserved[0] = o.reserved[1] = 0;
        p.tracks[stream * p.max_tracks + k] = o;
      }
    }
    number += __popcll(kept);
  }
}

__global__ __launch_bounds__(256) void tracks_labels_kernel(const TrkParams p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n_epochs * p.S) return;
  const int r = p.parent[i];
  p.track_of[i] = r < 0 ? -1 : p.acc[r].number;
}

// bytes of the three parts of the workspace, each a multiple of 64; false: more than 2^31 - 1 nodes
struct Layout {
  int64_t parent, acc, counts;
  int64_t total() const { return 64 + parent + acc + counts; }
};
bool layout(int64_t n_epochs, const crn_track_params &q, Layout *out) {
  if (n_epochs > INT32_MAX / q.max_segments) return false;
  const int64_t nodes = n_epochs * q.max_segments;
  out->parent = (4 * nodes + 63) / 64 * 64;
  out->acc = 64 * nodes;
  out->counts = (8 * n_epochs + 63) / 64 * 64;
  return true;
}

}  // namespace
}  // namespace crn

int64_t crn_tracks_workspace_bytes(int64_t n_epochs, const crn_track_params *params) {
  crn::Layout w;
  if (!params || crn::track_params_refusal(*params, n_epochs) || !crn::layout(n_epochs, *params, &w)) return -1;
  return w.total();
}

int crn_tracks_device(crn_handle *h, const crn_segment_epoch *d_epochs, const crn_segment *d_segments, int64_t n_epochs,
                      const crn_track_params *params, crn_track_stream *d_streams, crn_track *d_tracks, int32_t *d_track_of,
                      void *d_workspace, int64_t workspace_bytes, void *stream) {
  static_assert(sizeof(crn_track_params) == 32 && sizeof(crn_track) == 64 && sizeof(crn_track_stream) == 16, "include/crn_sense.h");
  using crn::misaligned;
  const char *who = "crn_tracks_device";
  if (!h || !params || !d_epochs || !d_segments || !d_streams || !d_tracks || !d_workspace)
    return crn::refuse(who, "null handle / params / epochs / segments / streams / tracks / workspace");
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  const crn_track_params &q = *params;
  if (const char *why = crn::track_params_refusal(q, n_epochs, n)) return crn::refuse(who, why);
  crn::Layout w;
  if (!crn::layout(n_epochs, q, &w)) return crn::refuse(who, "n_epochs x max_segments must stay below 2^31");
  if (misaligned(d_epochs, 16) || misaligned(d_segments, 16) || misaligned(d_streams, 16) || misaligned(d_tracks, 16) || misaligned(d_track_of, 4) ||
      misaligned(d_workspace, 8))
    return crn::refuse(who, "d_epochs, d_segments, d_streams and d_tracks must be 16-byte, d_workspace 8-byte, d_track_of 4-byte aligned");
  if (workspace_bytes < w.total()) return crn::refuse(who, "workspace smaller than crn_tracks_workspace_bytes");
  if (n_epochs == 0) return CRN_OK;
  hipError_t err = hipSetDevice(device);
  if (err != hipSuccess) return crn::fail_hip(who, err);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *ws = crn::align64(d_workspace);
  crn::TrkParams p;
  p.epochs = d_epochs;
  p.segments = d_segments;
  p.streams = d_streams;
  p.tracks = d_tracks;
  p.track_of = d_track_of;
  p.parent = reinterpret_cast<int *>(ws);
  p.acc = reinterpret_cast<crn::TrackAcc *>(ws + w.parent);
  p.count = reinterpret_cast<int *>(ws + w.parent + w.acc);
  p.base = p.count + n_epochs;
  p.n_epochs = n_epochs;
  p.n = n;
  p.S = q.max_segments;
  p.eps = q.epochs_per_stream;
  p.slack = q.slack_bins;
  p.max_miss = q.max_miss;
  p.min_epochs = q.min_epochs;
  p.max_tracks = q.max_tracks;
  const unsigned per_slot = (unsigned)((n_epochs * q.max_segments + 255) / 256), per_epoch = (unsigned)n_epochs;
  const unsigned n_streams = (unsigned)(n_epochs / q.epochs_per_stream);
  hipLaunchKernelGGL(crn::tracks_init_kernel, dim3(per_slot), dim3(256), 0, st, p);
  hipLaunchKernelGGL(crn::tracks_link_kernel, dim3(per_epoch), dim3(64), 0, st, p);
  hipLaunchKernelGGL(crn::tracks_gather_kernel, dim3(per_epoch), dim3(64), 0, st, p);
  hipLaunchKernelGGL(crn::tracks_count_kernel, dim3(per_epoch), dim3(64), 0, st, p);
  hipLaunchKernelGGL(crn::tracks_scan_kernel, dim3(n_streams), dim3(1024), 0, st, p);
  hipLaunchKernelGGL(crn::tracks_emit_kernel, dim3(per_epoch), dim3(64), 0, st, p);
  if (d_track_of) hipLaunchKernelGGL(crn::tracks_labels_kernel, dim3(per_slot), dim3(256), 0, st, p);
  err = hipGetLastError();
  if (err != hipSuccess) return crn::fail_hip(who, err);
  return CRN_OK;
}
