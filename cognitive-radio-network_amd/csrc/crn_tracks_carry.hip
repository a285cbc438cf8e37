// crn_tracks_carry.hip — tracks carried from one batch to the next (crn_tracks_carry_device, include/crn_sense.h): the linking of
// crn_tracks.hip over one call's epochs plus what the previous call left in the caller's carry buffer, so that a track that is on the air
// while a batch ends is one record, reported by the call in which it closes.
//
// Per stream the nodes are H = max_miss + 1 rows of S = max_segments ghost slots (the open tracks of the carry, in carry order), H rows of
// tail slots (the segments of the last H epochs before t_start, each knowing its open track) and one row per new epoch: R = 2H + eps rows,
// node = (stream R + row) S + slot, so that ascending index is carried tracks first, then time, then slot — the order of the roots.
// Seven small launches on the caller's stream, all scratch in the caller's workspace:
//   1. init     the old carry is read once, here: the stream's mark is checked (a carry that does not match is an empty one); a ghost's
//               accumulator is the carried one, parent[tail node] = its ghost (the index clamped), a new node is its own root with an
//               empty accumulator; the tail's (lo, width) pairs and the counts go to the workspace.  Nothing later reads the carry;
//   2. link     a wave per tail or new row: crn_tracks.hip's link pass, partners in NEW rows only;
//   3. gather   a wave per row.  New nodes add themselves to their root as in crn_tracks.hip, offsets taken from the root's lo_root;
//               tail nodes are only flattened (they were counted by the call that stored them); a ghost that is not its root adds its
//               accumulator re-based by delta;
//   4. count    per row: the roots that close with enough hits, the roots that stay open, and of those the ones with enough hits;
//   5. scan     a workgroup per stream: three exclusive scans over the rows, the stream's header, the zero fill, the new carry's header;
//   6. emit     a wave per row: closed roots to d_tracks, open roots to the new carry (and d_open); each open root keeps its position;
//   7. tail     a wave per row of the new tail: (lo, width, position of the open track) of the last H epochs up to T.
// The lock-free union, the link condition with its pair loop, a member's add, the centre, the zero fill and the wave scan are the ones
// crn_tracks.hip uses, from crn_track_link.h; so is the rule for a usable crn_track_params.
// No scratch memory, 4 KiB of LDS at most; every write to memory is a vector store or a vector atomic.
#include <cstddef>

#include "crn_segments.h"
#include "crn_track_link.h"

namespace crn {
namespace {

constexpr int MAX_H = 16;        // max_miss + 1 at most
constexpr int MAGIC = 0x43524e54;

// what a root gathers from its members, and what the carry keeps of an open track; 80 bytes
struct CarryAcc {
  int root_t, root_slot, lo_root;             // the root segment: global time, slot, lo
  int hits, nseg, lo_off, hi_off;
  unsigned peak;                              // bits of the largest peak_power
  unsigned long long last_key;                // max of t * S + (S - 1 - s) over the members, t global: 64 bits
  unsigned long long width_sum;
  double power, moment;
  int merged;                                 // n_epochs_hit is an upper bound (flag bit 2)
  int n_carried;                              // workspace: carried tracks in the component
  int number, pad;                            // workspace: the position among the open tracks (written by emit)
};
static_assert(sizeof(CarryAcc) == 80 && offsetof(CarryAcc, merged) == 64, "carry layout");

// the carry of one stream: this header, H x S tail slots (lo, width, open track, 0), H x S open tracks
struct CarryHeader {
  int magic, S, max_miss, n, T, n_open, pad[10];
  int tail_n[MAX_H];
};
static_assert(sizeof(CarryHeader) == 128, "carry layout");

// the part of the old carry's header the later passes need, in the workspace
struct StreamState {
  int valid, n_open, pad[14];
  int tail_n[MAX_H];
};
static_assert(sizeof(StreamState) == 128, "workspace layout");

struct CarryParams {
  const crn_segment_epoch *epochs;
  const crn_segment *segments;
  crn_track_carry_stream *streams;
  crn_track *tracks, *open;
  char *carry;
  int *parent;
  CarryAcc *acc;
  StreamState *state;
  int2 *tail_lw;        // [n_streams][H][S]
  int *count, *base;    // [n_streams][R][3]
  long long carry_stride;
  int n_streams, n, S, eps, H, R, slack, max_miss, min_epochs, max_tracks, t_start, flush;
};

__device__ __forceinline__ CarryHeader *carry_header(const CarryParams &p, int stream) {
  return reinterpret_cast<CarryHeader *>(p.carry + stream * p.carry_stride);
}
__device__ __forceinline__ int4 *carry_tail(const CarryParams &p, int stream) {
  return reinterpret_cast<int4 *>(p.carry + stream * p.carry_stride + sizeof(CarryHeader));
}
__device__ __forceinline__ CarryAcc *carry_open(const CarryParams &p, int stream) {
  return reinterpret_cast<CarryAcc *>(p.carry + stream * p.carry_stride + sizeof(CarryHeader) + (long long)p.H * p.S * 16);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// stored segments of row j of the tail-and-new part (0 .. H - 1: the tail, H .. H + eps - 1: the new epochs)
__device__ __forceinline__ int stored(const CarryParams &p, int stream, int j) {
  if (j < p.H) return p.state[stream].tail_n[j];
  return clampi(p.epochs[(long long)stream * p.eps + (j - p.H)].n_stored, 0, p.S);
}
// its (lo, width)
__device__ __forceinline__ int2 lo_width(const CarryParams &p, int stream, int j, int s) {
  if (j < p.H) return p.tail_lw[((long long)stream * p.H + j) * p.S + s];
  const crn_segment *g = p.segments + ((long long)stream * p.eps + (j - p.H)) * p.S + s;
  return make_int2(g->lo, g->width);
}
// node index of (row j of the tail-and-new part, slot s)
__device__ __forceinline__ int node(const CarryParams &p, int stream, int j, int s) { return (stream * p.R + p.H + j) * p.S + s; }

// one thread per node
__global__ __launch_bounds__(256) void carry_init_kernel(const CarryParams p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int per_stream = p.R * p.S, HS = p.H * p.S;
  if (i >= (long long)p.n_streams * per_stream) return;
  const int stream = (int)(i / per_stream), k = (int)(i - (long long)stream * per_stream);
  const CarryHeader *h = carry_header(p, stream);
  const bool valid = p.t_start > 0 && h->magic == MAGIC && h->S == p.S && h->max_miss == p.max_miss && h->n == p.n && h->T == p.t_start;
  const int n_open = valid ? clampi(h->n_open, 0, HS) : 0;
  if (k == 0) {
    StreamState *s = p.state + stream;   // written field by field: a local copy would be an indexed array, and so would sixteen plain loads of tail_n[]
    s->valid = valid;
    s->n_open = n_open;
    for (int j = 0; j < MAX_H; j++) s->tail_n[j] = j < p.H && n_open > 0 ? clampi(ld(h->tail_n + j), 0, p.S) : 0;
  }
  if (k < HS) {   // a ghost: the open track k of the carry
    if (k >= n_open) {
      p.parent[i] = -1;
      return;
    }
    // 80 bytes as five 16-byte words; the last holds merged, n_carried, number, pad
    const uint4 *src = reinterpret_cast<const uint4 *>(carry_open(p, stream) + k);
    uint4 *dst = reinterpret_cast<uint4 *>(p.acc + i);
    const uint4 w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3], w4 = src[4];
    p.parent[i] = (int)i;
    dst[0] = w0;
    dst[1] = w1;
    dst[2] = w2;
    dst[3] = w3;
    dst[4] = make_uint4(w4.x != 0, 1u, ~0u, 0u);
    return;
  }
  if (k < 2 * HS) {   // a tail segment: joined to its open track
    const int j = (k - HS) / p.S, s = (k - HS) - j * p.S;
    const int ns = n_open > 0 ? clampi(ld(h->tail_n + j), 0, p.S) : 0;
    if (s >= ns) {
      p.parent[i] = -1;
      return;
    }
    const int4 g = carry_tail(p, stream)[k - HS];
    p.tail_lw[(long long)stream * HS + (k - HS)] = make_int2(g.x, g.y);
    p.parent[i] = stream * per_stream + clampi(g.z, 0, n_open - 1);
    return;
  }
  const int e = (k - 2 * HS) / p.S, s = (k - 2 * HS) - e * p.S;
  const long long ge = (long long)stream * p.eps + e;
  if (s >= clampi(p.epochs[ge].n_stored, 0, p.S)) {
    p.parent[i] = -1;
    return;
  }
  p.parent[i] = (int)i;
  CarryAcc a;
  a.root_t = p.t_start + e;
  a.root_slot = s;
  a.lo_root = p.segments[ge * p.S + s].lo;
  a.hits = 0;
  a.nseg = 0;
  a.lo_off = 0x7fffffff;
  a.hi_off = -0x7fffffff - 1;
  a.peak = 0;
  a.last_key = 0;
  a.width_sum = 0;
  a.power = 0.0;
  a.moment = 0.0;
  a.merged = 0;
  a.n_carried = 0;
  a.number = -1;
  a.pad = 0;
  p.acc[i] = a;
}

// a wave per (stream, row of the tail-and-new part)
__global__ __launch_bounds__(64) void carry_link_kernel(const CarryParams p) {
  __shared__ int2 mine[MAX_SLOTS], next[MAX_SLOTS];   // (lo, width)
  const int l = threadIdx.x, rows = p.H + p.eps;
  const int stream = blockIdx.x / rows, j = blockIdx.x - stream * rows;
  const int na = stored(p, stream, j);
  if (na == 0) return;
  for (int s = l; s < na; s += 64) mine[s] = lo_width(p, stream, j, s);
  const int mask = p.n - 1;
  for (int d = 1; d <= p.H && j + d < rows; d++) {
    if (j + d < p.H) continue;   // partners are new epochs only (uniform over the wave)
    const int nb = stored(p, stream, j + d);
    __syncthreads();   // the previous round's reads of next[] are over (and mine[] is written)
    for (int s = l; s < nb; s += 64) next[s] = lo_width(p, stream, j + d, s);
    __syncthreads();
    link_rows(p.parent, mine, na, node(p, stream, j, 0), next, nb, node(p, stream, j + d, 0), l, mask, p.slack);
  }
}

// a wave per (stream, row): H ghost rows, H tail rows, eps new rows
__global__ __launch_bounds__(64) void carry_gather_kernel(const CarryParams p) {
  __shared__ int roots[MAX_SLOTS];
  const int l = threadIdx.x;
  const int stream = blockIdx.x / p.R, row = blockIdx.x - stream * p.R;
  const int half = p.n / 2, mask = p.n - 1;
  const int i0 = blockIdx.x * p.S;
  if (row < p.H) {   // ghosts: a carried track that is not the root of its component adds itself to the root, re-based
    const int ns = clampi(p.state[stream].n_open - row * p.S, 0, p.S);
    for (int s = l; s < ns; s += 64) {
      const int i = i0 + s;
      const int r = find<true>(p.parent, i);
      if (r == i) continue;
      atomicMin(p.parent + i, r);
      const CarryAcc b = p.acc[i];
      CarryAcc *a = p.acc + r;
      const int delta = wrapped(b.lo_root, a->lo_root, half, mask);
      atomicAdd(&a->hits, b.hits);
      atomicAdd(&a->nseg, b.nseg);
      atomicMax(&a->last_key, b.last_key);
      atomicMin(&a->lo_off, b.lo_off + delta);
      atomicMax(&a->hi_off, b.hi_off + delta);
      atomicMax(&a->peak, b.peak);
      atomicAdd(&a->width_sum, b.width_sum);
      atomicAdd(&a->power, b.power);
      atomicAdd(&a->moment, b.moment + (double)delta * b.power);
      atomicOr(&a->merged, b.merged);
      atomicAdd(&a->n_carried, 1);
    }
    return;
  }
  const int j = row - p.H;
  const int ns = stored(p, stream, j);
  if (ns == 0) return;
  for (int s = l; s < ns; s += 64) {
    const int i = i0 + s;
    const int r = find<true>(p.parent, i);
    roots[s] = r;
    if (r != i) atomicMin(p.parent + i, r);
  }
  if (j < p.H) return;   // tail segments were counted by the call that stored them
  __syncthreads();
  const int e = j - p.H;
  const long long ge = (long long)stream * p.eps + e;
  for (int s = l; s < ns; s += 64) {
    const int r = roots[s];
    const crn_segment g = p.segments[ge * p.S + s];
    CarryAcc *a = p.acc + r;
    const int off = wrapped(g.lo, a->lo_root, half, mask);
    bool first = true;   // of this epoch's members of r
    for (int k = 0; k < s; k++) first = first && roots[k] != r;
    add_member(a, g, off, first, p.t_start + e, s, p.S);
  }
}

// a root's record as it stands after the gather pass
struct Settled {
  int last_t, last_slot, hits, merged;
  bool open;
};
__device__ __forceinline__ Settled settle(const CarryParams &p, const CarryAcc &a) {
  Settled v;
  const unsigned long long t = a.last_key / (unsigned)p.S;
  v.last_t = t > 0x7fffffffull ? 0x7fffffff : (int)t;
  v.last_slot = p.S - 1 - (int)(a.last_key - t * (unsigned)p.S);
  v.merged = a.merged != 0 || a.n_carried >= 2;
  const long long span = (long long)v.last_t - a.root_t + 1;
  v.hits = v.merged && span < a.hits ? (int)span : a.hits;
  v.open = !p.flush && v.last_t >= p.t_start + p.eps - 1 - p.max_miss;
  return v;
}

// the slots of `row` that can hold a root: the carried tracks of a ghost row, the stored segments of a new row, none of a tail row
__device__ __forceinline__ int root_slots(const CarryParams &p, int stream, int row) {
  if (row < p.H) return clampi(p.state[stream].n_open - row * p.S, 0, p.S);
  if (row < 2 * p.H) return 0;
  return stored(p, stream, row - p.H);
}

__global__ __launch_bounds__(64) void carry_count_kernel(const CarryParams p) {
  const int l = threadIdx.x;
  const int stream = blockIdx.x / p.R, row = blockIdx.x - stream * p.R;
  const int ns = root_slots(p, stream, row);
  int closed = 0, open = 0, open_found = 0;
  for (int s0 = 0; s0 < ns; s0 += 64) {
    const int s = s0 + l, i = blockIdx.x * p.S + s;
    bool is_closed = false, is_open = false, enough = false;
    if (s < ns && p.parent[i] == i) {
      const Settled v = settle(p, p.acc[i]);
      enough = v.hits >= p.min_epochs;
      is_open = v.open;
      is_closed = !v.open && enough;
    }
    closed += __popcll(__ballot(is_closed));
    open += __popcll(__ballot(is_open));
    open_found += __popcll(__ballot(is_open && enough));
  }
  if (l == 0) {
    int *c = p.count + 3ll * blockIdx.x;
    c[0] = closed;
    c[1] = open;
    c[2] = open_found;
  }
}

// one workgroup per stream; thread i owns the rows [i chunk, (i + 1) chunk) of the stream
__global__ __launch_bounds__(1024) void carry_scan_kernel(const CarryParams p) {
  __shared__ int wave_sum[3][16], wave_nodes[16];
  const int i = threadIdx.x, l = i & 63, w = i >> 6;
  const int stream = blockIdx.x;
  const long long r0 = (long long)stream * p.R;
  const int chunk = (p.R + 1023) / 1024;
  const int lo = i * chunk < p.R ? i * chunk : p.R, hi = lo + chunk < p.R ? lo + chunk : p.R;
  int sum[3] = {0, 0, 0}, nodes = 0;
  for (int r = lo; r < hi; r++) {
    for (int c = 0; c < 3; c++) sum[c] += p.count[3 * (r0 + r) + c];
    if (r >= 2 * p.H) nodes += stored(p, stream, r - p.H);
  }
  int incl[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    incl[c] = wave_scan(sum[c], l);
    if (l == 63) wave_sum[c][w] = incl[c];
  }
#pragma unroll
  for (int s = 32; s > 0; s /= 2) nodes += __shfl_xor(nodes, s, 64);
  if (l == 0) wave_nodes[w] = nodes;
  __syncthreads();
  int total[3], all_nodes = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    int before = 0;
    total[c] = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      before += k < w ? wave_sum[c][k] : 0;
      total[c] += wave_sum[c][k];
    }
    int run = before + incl[c] - sum[c];
    for (int r = lo; r < hi; r++) {
      p.base[3 * (r0 + r) + c] = run;
      run += p.count[3 * (r0 + r) + c];
    }
  }
#pragma unroll
  for (int k = 0; k < 16; k++) all_nodes += wave_nodes[k];
  const int n_stored = total[0] < p.max_tracks ? total[0] : p.max_tracks;
  const int n_open_stored = !p.open ? 0 : total[2] < p.max_tracks ? total[2] : p.max_tracks;
  if (i == 0) {
    crn_track_carry_stream h;
    h.n_found = total[0];
    h.n_stored = n_stored;
    h.n_nodes = all_nodes;
    h.n_open = total[1];
    h.n_open_found = total[2];
    h.n_open_stored = n_open_stored;
    h.status = p.t_start > 0 && !p.state[stream].valid ? 1 : 0;
    h.reserved = 0;
    p.streams[stream] = h;
  }
  // the new carry's header: the mark, the open tracks, the stored segments of the times T - H .. T - 1 (rows eps .. eps + H - 1 of the
  // tail-and-new part: old tail rows where the call was shorter than H)
  if (i < 32) {
    int v = 0;
    if (i == 0) v = MAGIC;
    else if (i == 1) v = p.S;
    else if (i == 2) v = p.max_miss;
    else if (i == 3) v = p.n;
    else if (i == 4) v = p.t_start + p.eps;
    else if (i == 5) v = total[1];
    else if (i >= 16 && i - 16 < p.H && !p.flush) v = stored(p, stream, i - 16 + p.eps);
    reinterpret_cast<int *>(carry_header(p, stream))[i] = v;
  }
  zero_unused(p.tracks + (long long)stream * p.max_tracks, n_stored, p.max_tracks, i);
  if (p.open) zero_unused(p.open + (long long)stream * p.max_tracks, n_open_stored, p.max_tracks, i);
}

__device__ __forceinline__ crn_track record(const CarryParams &p, const CarryAcc &a, const Settled &v) {
  crn_track o;
  o.first_t = a.root_t;
  o.first_slot = a.root_slot;
  o.last_t = v.last_t;
  o.last_slot = v.last_slot;
  o.n_epochs_hit = v.hits;
  o.n_segments = a.nseg;
  o.lo_off = a.lo_off;
  o.hi_off = a.hi_off;
  o.width_sum = (int64_t)a.width_sum;
  o.power_sum = (float)a.power;
  o.peak_power = __uint_as_float(a.peak);
  o.centre = centre(a.lo_root, a.moment, a.power, p.n);
  o.flags = (a.root_t <= p.max_miss ? 1 : 0) | (v.last_t >= p.t_start + p.eps - 1 - p.max_miss ? 2 : 0) | (v.merged ? 4 : 0);
  o.reserved[0] = o.reserved[1] = 0;
  return o;
}

__global__ __launch_bounds__(64) void carry_emit_kernel(const CarryParams p) {
  const int l = threadIdx.x;
  const int stream = blockIdx.x / p.R, row = blockIdx.x - stream * p.R;
  const int ns = root_slots(p, stream, row);
  if (ns == 0) return;
  const int *b = p.base + 3ll * blockIdx.x;
  int n_closed = b[0], n_open = b[1], n_open_found = b[2];
  const uint64_t below = (1ull << l) - 1;
  for (int s0 = 0; s0 < ns; s0 += 64) {
    const int s = s0 + l, i = blockIdx.x * p.S + s;
    const bool root = s < ns && p.parent[i] == i;
    CarryAcc a;
    Settled v;
    bool enough = false, is_open = false;
    if (root) {
      a = p.acc[i];
      v = settle(p, a);
      enough = v.hits >= p.min_epochs;
      is_open = v.open;
    }
    const uint64_t closed = __ballot(root && !is_open && enough), open = __ballot(is_open), open_found = __ballot(is_open && enough);
    if (root && !is_open && enough) {
      const int k = n_closed + __popcll(closed & below);
      if (k < p.max_tracks) p.tracks[(long long)stream * p.max_tracks + k] = record(p, a, v);
    }
    if (is_open) {
      const int k = n_open + __popcll(open & below);   // below H x S: every open track owns a segment of the last H epochs
      p.acc[i].number = k;
      if (k < p.H * p.S) {
        a.hits = v.hits;
        a.merged = v.merged;
        a.n_carried = 0;
        a.number = 0;
        carry_open(p, stream)[k] = a;
      }
      if (p.open && enough) {
        const int ko = n_open_found + __popcll(open_found & below);
        if (ko < p.max_tracks) p.open[(long long)stream * p.max_tracks + ko] = record(p, a, v);
      }
    }
    n_closed += __popcll(closed);
    n_open += __popcll(open);
    n_open_found += __popcll(open_found);
  }
}

// a wave per (stream, row of the new tail): time T - H + j is row eps + j of the tail-and-new part
__global__ __launch_bounds__(64) void carry_tail_kernel(const CarryParams p) {
  const int l = threadIdx.x;
  const int stream = blockIdx.x / p.H, j = blockIdx.x - stream * p.H;
  const int src = p.eps + j;
  const int ns = stored(p, stream, src);
  int4 *out = carry_tail(p, stream) + j * p.S;
  for (int s = l; s < ns; s += 64) {
    const int2 g = lo_width(p, stream, src, s);
    const int r = p.parent[node(p, stream, src, s)];   // flat since the gather pass
    out[s] = make_int4(g.x, g.y, p.acc[r].number, 0);
  }
}

// bytes of the parts of the workspace, each a multiple of 64; rows and nodes over all streams; false: more than 2^31 - 1 nodes
struct Layout {
  int64_t rows, nodes, parent, acc, state, tail, counts;
  int64_t total() const { return 64 + parent + acc + state + tail + 2 * counts; }
};
int64_t carry_stride(const crn_track_params &q) {
  return (int64_t)sizeof(CarryHeader) + (int64_t)(q.max_miss + 1) * q.max_segments * (16 + (int64_t)sizeof(CarryAcc));
}
bool layout(int64_t n_epochs, const crn_track_params &q, Layout *out) {
  if (n_epochs > INT32_MAX / q.max_segments) return false;
  const int64_t n_streams = n_epochs / q.epochs_per_stream, H = q.max_miss + 1;
  out->rows = n_epochs + n_streams * 2 * H;
  out->nodes = out->rows * q.max_segments;
  if (out->nodes > INT32_MAX) return false;
  out->parent = (4 * out->nodes + 63) / 64 * 64;
  out->acc = (int64_t)sizeof(CarryAcc) * out->nodes;
  out->acc = (out->acc + 63) / 64 * 64;
  out->state = (int64_t)sizeof(StreamState) * n_streams;
  out->tail = (8 * n_streams * H * q.max_segments + 63) / 64 * 64;
  out->counts = (12 * out->rows + 63) / 64 * 64;
  return true;
}

}  // namespace
}  // namespace crn

int64_t crn_tracks_carry_bytes(int64_t n_streams, const crn_track_params *params) {
  if (!params || crn::track_params_refusal(*params, 0) || n_streams < 0 || n_streams > INT32_MAX) return -1;
  return n_streams > 0 ? n_streams * crn::carry_stride(*params) : 16;   // positive for valid arguments, like the workspace sizes
}

int64_t crn_tracks_carry_workspace_bytes(int64_t n_epochs, const crn_track_params *params) {
  crn::Layout w;
  if (!params || crn::track_params_refusal(*params, n_epochs) || !crn::layout(n_epochs, *params, &w)) return -1;
  return w.total();
}

int crn_tracks_carry_device(crn_handle *h, const crn_segment_epoch *d_epochs, const crn_segment *d_segments, int64_t n_epochs,
                            const crn_track_params *params, int64_t t_start, int32_t flush, void *d_carry, int64_t carry_bytes,
                            crn_track_carry_stream *d_streams, crn_track *d_tracks, crn_track *d_open, void *d_workspace,
                            int64_t workspace_bytes, void *stream) {
  static_assert(sizeof(crn_track_carry_stream) == 32, "include/crn_sense.h");
  using crn::misaligned;
  const char *who = "crn_tracks_carry_device";
  if (!h || !params || !d_epochs || !d_segments || !d_carry || !d_streams || !d_tracks || !d_workspace)
    return crn::refuse(who, "null handle / params / epochs / segments / carry / streams / tracks / workspace");
  int n = 0, device = 0;
  crn::handle_geometry(h, &n, &device);
  const crn_track_params &q = *params;
  if (const char *why = crn::track_params_refusal(q, n_epochs, n)) return crn::refuse(who, why);
  if (t_start < 0 || t_start + q.epochs_per_stream > INT32_MAX)
    return crn::refuse(who, "t_start must be >= 0 and t_start + epochs_per_stream at most 2^31 - 1");
  crn::Layout w;
  if (!crn::layout(n_epochs, q, &w)) return crn::refuse(who, "(n_epochs + 2 (max_miss + 1) streams) x max_segments must stay below 2^31");
  const int64_t n_streams = n_epochs / q.epochs_per_stream;
  if (misaligned(d_epochs, 16) || misaligned(d_segments, 16) || misaligned(d_streams, 16) || misaligned(d_tracks, 16) || misaligned(d_open, 16) ||
      misaligned(d_carry, 16) || misaligned(d_workspace, 8))
    return crn::refuse(who, "d_epochs, d_segments, d_streams, d_tracks, d_open and d_carry must be 16-byte, d_workspace 8-byte aligned");
  if (carry_bytes < crn_tracks_carry_bytes(n_streams, params)) return crn::refuse(who, "carry smaller than crn_tracks_carry_bytes");
  if (workspace_bytes < w.total()) return crn::refuse(who, "workspace smaller than crn_tracks_carry_workspace_bytes");
  if (n_epochs == 0) return CRN_OK;
  hipError_t err = hipSetDevice(device);
  if (err != hipSuccess) return crn::fail_hip(who, err);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char *ws = crn::align64(d_workspace);
  crn::CarryParams p;
  p.epochs = d_epochs;
  p.segments = d_segments;
  p.streams = d_streams;
  p.tracks = d_tracks;
  p.open = d_open;
  p.carry = static_cast<char *>(d_carry);
  p.parent = reinterpret_cast<int *>(ws);
  p.acc = reinterpret_cast<crn::CarryAcc *>(ws + w.parent);
  p.state = reinterpret_cast<crn::StreamState *>(ws + w.parent + w.acc);
  p.tail_lw = reinterpret_cast<int2 *>(ws + w.parent + w.acc + w.state);
  p.count = reinterpret_cast<int *>(ws + w.parent + w.acc + w.state + w.tail);
  p.base = reinterpret_cast<int *>(ws + w.parent + w.acc + w.state + w.tail + w.counts);
  p.carry_stride = crn::carry_stride(q);
  p.n_streams = (int)n_streams;
  p.n = n;
  p.S = q.max_segments;
  p.eps = q.epochs_per_stream;
  p.H = q.max_miss + 1;
  p.R = 2 * p.H + p.eps;
  p.slack = q.slack_bins;
  p.max_miss = q.max_miss;
  p.min_epochs = q.min_epochs;
  p.max_tracks = q.max_tracks;
  p.t_start = (int)t_start;
  p.flush = flush != 0;
  const unsigned per_slot = (unsigned)((w.nodes + 255) / 256), per_row = (unsigned)w.rows;
  const unsigned per_link_row = (unsigned)(n_streams * (p.H + p.eps)), per_tail_row = (unsigned)(n_streams * p.H);
  hipLaunchKernelGGL(crn::carry_init_kernel, dim3(per_slot), dim3(256), 0, st, p);
  hipLaunchKernelGGL(crn::carry_link_kernel, dim3(per_link_row), dim3(64), 0, st, p);
  hipLaunchKernelGGL(crn::carry_gather_kernel, dim3(per_row), dim3(64), 0, st, p);
  hipLaunchKernelGGL(crn::carry_count_kernel, dim3(per_row), dim3(64), 0, st, p);
  hipLaunchKernelGGL(crn::carry_scan_kernel, dim3((unsigned)n_streams), dim3(1024), 0, st, p);
  hipLaunchKernelGGL(crn::carry_emit_kernel, dim3(per_row), dim3(64), 0, st, p);
  if (!p.flush) hipLaunchKernelGGL(crn::carry_tail_kernel, dim3(per_tail_row), dim3(64), 0, st, p);
  err = hipGetLastError();
  if (err != hipSuccess) return crn::fail_hip(who, err);
  return CRN_OK;
}
