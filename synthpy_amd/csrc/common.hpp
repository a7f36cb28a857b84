// Shared host-side plumbing of libsynthray.so: error text, the per-process HIP context
// (device + one stream + timing events) and the opaque handle layouts.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "synthray.h"

namespace sr {

constexpr double kC = 299792458.0;  // scipy.constants.c (full_solver.py:93)

// ---- errors ----------------------------------------------------------------------
void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);

#define SR_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return sr::fail(SR_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),     \
                      __FILE__, __LINE__);                                                   \
  } while (0)

#define SR_CHECK(cond, ...)                                 \
  do {                                                      \
    if (!(cond)) return sr::fail(SR_ERR_INVALID, __VA_ARGS__); \
  } while (0)

// a callee that has set the error text and returns a status: a non-zero one is handed on
#define SR_RC(call)         \
  do {                      \
    const int rc_ = (call); \
    if (rc_) return rc_;    \
  } while (0)

// ---- context ---------------------------------------------------------------------
constexpr int kStreams = 2;
constexpr int kMaxTileSegs = 8;  // segments of a tile-path trace that are timed one by one (trace.hip: trace_tiled)
struct Context {
  int device = -1;
  hipStream_t stream = nullptr;  // the stream every call of the library queues its work on: streams[current]
  hipEvent_t *ev = nullptr;      // the timing events that go with it: evs[current]
  hipStream_t streams[kStreams] = {nullptr, nullptr};
  // [0..3]: start, kernels' start, kernels' end, end of a trace; [4 + 2q], [5 + 2q]: around the tile kernel of segment q
  hipEvent_t evs[kStreams][4 + 2 * kMaxTileSegs] = {};
  // One SIDE stream per library stream (round 5): the rays a tile-path trace loses are carried to the end of the volume by
  // k_trace_f64 there, beside the tile kernel's remaining segments on the library stream (trace.hip: trace_tiled).  Ordered with
  // side_ev[.][0] (the library stream got this far: the side stream may go on) and [1] (the side stream is done: joined before the
  // trace's last kernel).  Everything queued on a side stream is joined to its library stream before the call that queued it returns.
  hipStream_t side[kStreams] = {nullptr, nullptr};
  hipEvent_t side_ev[kStreams][2] = {};
  int current = 0;
  int n_cu = 256;
  // sr_grid_cus / sr_grid_stats (capped_grid below): the compute-unit count the grid caps are sized for when > 0 (0: n_cu),
  // the launches that went through capped_grid since the last reset, and those that got fewer blocks than they wanted
  int grid_cus_override = 0;
  int64_t grid_launches = 0, grid_short = 0;
};
Context &ctx();
int ensure_init();  // sr_init(0) on first use

// SYNTHRAY_ALLOC_FILL=<0..255> (a test knob, read at every allocation and every hand-out of the scratch block): the byte every
// buffer of the library is filled with before it is handed out, so that a kernel or host path that depends on what device memory
// held before shows (docs/ALLOCATIONS.md, tests/test_alloc_poison.py).  -1: unset, empty or not a byte -- nothing is filled.
inline int alloc_fill() {
  const char *e = getenv("SYNTHRAY_ALLOC_FILL");
  if (!e || !e[0]) return -1;
  char *end = nullptr;
  const long v = strtol(e, &end, 0);
  return (end && *end == '\0' && v >= 0 && v <= 255) ? (int)v : -1;
}
// `bytes` at p hold `fill` when this returns: waited for, because the buffer may next be used on the side stream or the other
// library stream.  Memsets, uploads and kernels of the caller come after it.
inline hipError_t dev_fill(void *p, size_t bytes, int fill) {
  if (fill < 0 || !p || bytes == 0) return hipSuccess;
  hipStream_t st = ctx().stream;
  const hipError_t e = hipMemsetAsync(p, fill, bytes, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}
// THE device allocation of the library (every other site goes through it): raw bytes and the runtime's own status, for the
// callers that have a failure path of their own (the scratch block's second try, the tile records that may be refused).
inline hipError_t dev_alloc_bytes(void **p, size_t bytes) {
  *p = nullptr;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    *p = nullptr;
    return e;
  }
  e = dev_fill(*p, bytes, alloc_fill());
  if (e != hipSuccess) {
    (void)hipFree(*p);
    *p = nullptr;
  }
  return e;
}
template <typename T>
int dev_alloc(T **p, size_t count) {
  *p = nullptr;
  if (count == 0) return SR_OK;
  SR_HIP(dev_alloc_bytes(reinterpret_cast<void **>(p), count * sizeof(T)));
  return SR_OK;
}
inline void dev_free(void *p) {
  if (p) (void)hipFree(p);
}

// The device buffers of ONE call of an entry point that takes host arrays: fresh hipMallocs (a volume's staging is gigabytes, and
// the scratch block below is kept from call to call), freed together when the owner goes -- on every return, early or not -- or
// one by one with release().  Helpers take the owner by reference and add their buffers to it.
class CallBuffers {
 public:
  CallBuffers() = default;
  CallBuffers(const CallBuffers &) = delete;
  CallBuffers &operator=(const CallBuffers &) = delete;
  ~CallBuffers() {
    for (void *p : held_) dev_free(p);
  }
  template <typename T>
  int alloc(T **p, size_t count) {
    SR_RC(dev_alloc(p, count));
    if (*p) held_.push_back(*p);
    return SR_OK;
  }
  template <typename T>
  int zeroed(T **p, size_t count, hipStream_t st) {  // a result that kernels add into
    SR_RC(alloc(p, count));
    if (*p) SR_HIP(hipMemsetAsync(*p, 0, count * sizeof(T), st));
    return SR_OK;
  }
  // a host array into a fresh buffer, the copy queued on `st`; a NULL array is skipped and *p stays NULL (sr_optics without E)
  template <typename T>
  int upload(T **p, const T *host, size_t count, hipStream_t st) {
    *p = nullptr;
    if (!host) return SR_OK;
    SR_RC(alloc(p, count));
    if (*p) SR_HIP(hipMemcpyAsync(*p, host, count * sizeof(T), hipMemcpyHostToDevice, st));
    return SR_OK;
  }
  void release(void *p) {  // free one buffer before the call ends (to cap its peak)
    const auto it = std::find(held_.begin(), held_.end(), p);
    if (it == held_.end()) return;
    dev_free(p);
    held_.erase(it);
  }

 private:
  std::vector<void *> held_;
};
// The tail of such a call, after its launches: their error, the results to the host (a NULL destination is skipped), and the
// stream is waited for -- the call is done with its buffers.
struct HostOut {
  void *host;
  const void *dev;
  size_t bytes;
};
int stage_out(hipStream_t st, std::initializer_list<HostOut> out);

inline unsigned grid_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// The grid of every launch that covers its work with a grid-stride loop: the blocks the work needs, at most per_cu blocks per
// compute unit (and at least one).  Each call is ONE launch: it is counted in the context, and so is a launch that gets fewer
// blocks than it wanted and therefore takes a second trip through its loop (sr_grid_stats).  grid_cus() is the device's
// compute-unit count unless sr_grid_cus has set another one, a measurement and test knob: no kernel needs a minimum grid to
// be correct, so every site takes the cap as it comes (at 1 compute unit: per_cu blocks).
inline int grid_cus() {
  const Context &c = ctx();
  return c.grid_cus_override > 0 ? c.grid_cus_override : c.n_cu;
}
inline unsigned capped_grid(int64_t blocks_wanted, int per_cu) {
  Context &c = ctx();
  const int n_cu = grid_cus();
  const int64_t cap = (int64_t)n_cu * per_cu;
  ++c.grid_launches;
  if (blocks_wanted > cap) ++c.grid_short;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks_wanted, cap));
}

// Device memory for the staging of ONE call (download in ray order, counts as float64, amplitude, sr_rays_optics): a block per
// stream that grows and is kept, so that the entry points a caller loops over do not hipMalloc / hipFree (each waits for the
// device) every time.  The caller must be done with it (stream synchronised) before it returns.  Blocks beyond kScratchKeep
// are given back by scratch_trim() at the end of the call; sr_release_caches() frees all.  nullptr + error text on failure.
constexpr size_t kScratchKeep = (size_t)2 << 30;
void *scratch(size_t bytes);
void scratch_trim();
void scratch_release();
// Host -> device copy of `bytes` on `st`, then the stream is waited for.  From pageable memory the runtime's own staging runs on
// one thread (8-30 GB/s on this box); here several threads copy slices into page-locked bounce buffers of the library and
// each slice goes to the device by DMA as soon as it is in: the link's rate.  Page-locked sources are copied directly.
int upload_sync(void *dst, const void *src, size_t bytes, hipStream_t st);
// Exclusive scan of v[0..n) in place on `st` (trace.hip, the ray binning's scan); sums: (n + 2047) / 2048 words of workspace.
void exclusive_scan_u32(uint32_t *v, int64_t n, uint32_t *sums, hipStream_t st);

// Per-launch totals (ray steps, deposited rays) are summed by one atomic per wavefront.  156 000 wavefronts adding to ONE
// address take ~2 ms of serialised device-scope atomics (it was the whole duration of the deposit kernel), so the totals
// are striped over kStripes cache lines picked by the workgroup index and added up on the host.
constexpr int kStripes = 256, kStripeStride = 16;  // 16 x 8 B = one 128-byte line per stripe
// [0..15] plain counters ([1], [2]: queue lengths of a trace, [3]: rays past the first kernel so far, [5]: edge guard, [8]: the
// rays the tile path has lost so far in this trace = entries of the straggler records), then 3 striped totals: 0 ray steps, 1 deposited rays, 2 the steps of an edge-guard re-trace (not
// part of the job's ray-step count: those rays' steps were counted when the mixed kernel took them)
constexpr size_t kCounterWords = 16 + 3 * (size_t)kStripes * kStripeStride;
#ifdef __HIPCC__
__device__ __forceinline__ unsigned long long *stripe(unsigned long long *base, int which) {
  return base + 16 + ((size_t)which * kStripes + (blockIdx.x & (kStripes - 1))) * kStripeStride;
}
#endif
// Append the launch slots of the lanes with `want` to a queue: the wavefront ballots, ONE lane reserves popcount(mask)
// slots with a single atomic, and each lane takes its prefix rank (compaction by ballot + prefix popcount).  Must be
// reached by the whole wavefront.
#ifdef __HIPCC__
__device__ __forceinline__ void queue_push(unsigned long long *count, uint32_t *list, bool want, uint32_t slot) {
  const unsigned long long mask = __ballot(want);
  if (mask == 0ull) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(mask));
  base = __shfl(base, leader, 64);
  if (want) list[base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull))] = slot;
}
#endif
// The cell of p on one axis of an sr_field (the `cell` / `outside` lines of sr_field_resample's rule, include/synthray.h; shared by
// resample.hip and push.hip): the largest i with g[i] <= p, clipped to n - 2; false when p lies outside (or is NaN).
#ifdef __HIPCC__
// BOUNDS: g0 = g[0] and gL = g[n - 1] come from the caller (push.hip holds them as kernel arguments for its own inside test);
// otherwise they are read here (resample.hip).
template <bool BOUNDS>
__device__ __forceinline__ bool locate_in(const double *__restrict__ g, int n, double inv_h, double lo_in, double hi_in, double p,
                                          int &cell, double &w) {
  const double g0 = BOUNDS ? lo_in : g[0], gL = BOUNDS ? hi_in : g[n - 1];
  if (!(p >= g0 && p <= gL)) return false;
  int i = (int)((p - g0) * inv_h);
  i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
  if (!(g[i] <= p && (i == n - 2 || p < g[i + 1]))) {  // a non-uniform axis, or a guess one cell off: bisect
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (g[mid] <= p)
        lo = mid;
      else
        hi = mid;
    }
    i = lo;
  }
  cell = i;
  w = (p - g[i]) / (g[i + 1] - g[i]);
  return true;
}
__device__ __forceinline__ bool locate(const double *__restrict__ g, int n, double inv_h, double p, int &cell, double &w) {
  return locate_in<false>(g, n, inv_h, 0.0, 0.0, p, cell, w);
}
// One scalar at the cell (ci, cj, ck) with the blend of sr_field_resample's rule (shared by thomson.hip and sightlines.hip); nc:
// components per node, c: the one wanted; sx, sy: the node strides of x and y.  In two halves, so that a kernel can have the eight
// corner reads of its next point in flight while it works on this one: corners_load only reads, corners_blend only computes.
template <typename T>
struct Corners {
  T v[8];  // (di, dj, dk) at v[4*di + 2*dj + dk]
};
template <typename T>
__device__ __forceinline__ Corners<T> corners_load(const T *__restrict__ src, int nc, int c, int64_t sx, int64_t sy, int ci, int cj,
                                                   int ck) {
  const T *lo = src + (((int64_t)ci * sx + (int64_t)cj * sy + (int64_t)ck) * nc + c);
  const T *hi = lo + sx * nc;
  const int64_t ry = sy * nc;
  return Corners<T>{{lo[0], lo[nc], lo[ry], lo[ry + nc], hi[0], hi[nc], hi[ry], hi[ry + nc]}};
}
template <typename T>
__device__ __forceinline__ double corners_blend(const Corners<T> &f, double ux, double wx, double w00, double w01, double w10,
                                                double w11) {
  const double s0 = (((double)f.v[0] * w00 + (double)f.v[1] * w01) + (double)f.v[2] * w10) + (double)f.v[3] * w11;
  const double s1 = (((double)f.v[4] * w00 + (double)f.v[5] * w01) + (double)f.v[6] * w10) + (double)f.v[7] * w11;
  return ux * s0 + wx * s1;
}
template <typename T>
__device__ __forceinline__ double blend(const T *__restrict__ src, int nc, int c, int64_t sx, int64_t sy, int ci, int cj, int ck,
                                        double ux, double wx, double w00, double w01, double w10, double w11) {
  return corners_blend(corners_load(src, nc, c, sx, sy, ci, cj, ck), ux, wx, w00, w01, w10, w11);
}
#endif
inline unsigned long long stripe_sum(const unsigned long long *host_words, int which) {
  unsigned long long t = 0;
  for (int s = 0; s < kStripes; ++s) t += host_words[16 + ((size_t)which * kStripes + s) * kStripeStride];
  return t;
}
// The counter words and striped totals by name.  [kGuardQueue]: length of the edge guard's queue, and after it the length of the
// queue its float64 re-trace leaves (the two are reset together).  stripe_base: the first word of striped total `which`.
constexpr int kGuardQueue = 4;
constexpr int kStripeDeposited = 1, kStripeRetrace = 2;
constexpr size_t kStripeBytes = sizeof(unsigned long long) * kStripes * kStripeStride;  // one striped total
inline unsigned long long *counter_word(unsigned long long *counters, int word) { return counters + word; }
inline unsigned long long *stripe_base(unsigned long long *counters, int which) {
  return counters + 16 + (size_t)which * kStripes * kStripeStride;
}

// ---- runtime values -> template arguments --------------------------------------------------------------------------------
// with_flags(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): every launch that picks a kernel
// instantiation from runtime booleans is written once, as a generic lambda, and prunes the combinations that must not exist with
// `if constexpr` (they are never instantiated).
template <typename F>
void with_flags(F &&f) {
  f();
}
template <typename F, typename... Rest>
void with_flags(F &&f, bool b, Rest... rest) {
  if (b)
    with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else
    with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// with_count<MAX>(f, n) calls f(std::integral_constant<int, n>{}) for n in 1..MAX (n is clamped to that range)
template <int MAX, typename F>
void with_count(F &&f, int n) {
  if constexpr (MAX > 1) {
    if (n < MAX) return with_count<MAX - 1>(f, n);
  }
  f(std::integral_constant<int, MAX>{});
}

// ---- the packed node order of a volume ---------------------------------------------------------------------------
// Node (ia, ib, ic) -- ia along the probing axis -- sits at
//     ((ia / 8) * nb*nc + ib*nc + ic) * 8 + ia % 8 :
// OCTETS of eight consecutive node planes; inside an octet the lateral columns are contiguous and each column's eight
// planes are one 128-byte line of float4 records.  A ray marching along `a` still walks four line-sized streams (one new
// line per column every eight steps), and the lines all the rays of a launch need at about the same time -- they advance
// through the planes together -- form ONE contiguous region of nb*nc*128 bytes instead of one line in every 16*na bytes:
// that is what HBM sees when the lines are not shared (sparse bundles).  The last octet is padded (zeros).
#if defined(__HIPCC__)
#define SR_HD __host__ __device__
#else
#define SR_HD
#endif
SR_HD inline int64_t node_index(int ia, int ib, int ic, int nb, int nc) {
  return ((int64_t)(ia >> 3) * nb * nc + (int64_t)ib * nc + ic) * 8 + (ia & 7);
}
inline size_t packed_nodes(int na, int nb, int nc) { return (size_t)((na + 7) / 8) * (size_t)nb * (size_t)nc * 8; }

}  // namespace sr

// ---- opaque handles --------------------------------------------------------------
// Volume: one float4 per node {dnd_b, dnd_c, dnd_a, hi(n-1)} in the packed node order above (sr::node_index;
// b = (a+1)%3, c = (a+2)%3), plus lo(n-1) so that n-1 = hi + lo keeps 48 bits, and the node coordinates in float64
// (what scipy's interpolator works with).
struct sr_volume {
  int nx = 0, ny = 0, nz = 0;
  int axis = 2;          // physical index of `a`
  int na = 0, nb = 0, nc = 0;
  int flags = 0;
  double omega = 0;
  float4 *P = nullptr;   // packed node order (sr::node_index), sr::packed_nodes records
  float *L = nullptr;    // the same order, or nullptr
  double *K = nullptr;   // kappa per node (packed order) or nullptr (inverse bremsstrahlung)
  double *Q = nullptr;   // {ne, Bx, By, Bz} per node (packed order), or nullptr (Faraday rotation)
  // The tile path's coefficient records ready-made (trace_tile.inc, REC): per node plane k and lateral CELL (ib, ic) the 16 float64
  // {a[4], b[4], c[4], d[4]} coefs_from_corners forms, at R[((k * (nc-1) + ic) * (nb-1) + ib) * 16] -- 128 B per (cell, plane), built
  // at the first trace that wants them (SYNTHRAY_TILE_RECORDS) and kept with the volume; nullptr: not built
  mutable double *R = nullptr;
  mutable bool R_tried = false;  // the allocation was refused once: do not ask again
  double verdet = 0;
  // a slab of node planes k_lo..k_hi of a domain with n_glob planes on the probing axis (A12); whole volume: 0..n-1
  bool is_slab = false;
  int k_lo = 0, k_hi = 0, n_glob = 0;
  double *g[3] = {nullptr, nullptr, nullptr};   // device node coordinates, order (a, b, c)
  double *rg[3] = {nullptr, nullptr, nullptr};  // device 1/(g[i+1]-g[i]), order (a, b, c)
  std::vector<double> hg[3];                    // host copies, order (a, b, c)
  // per-plane RK4 step constants (trace.hip: StepTab), one device table per `substeps` value, built at the first trace
  // that asks for it and kept until the volume goes: a pure function of the node coordinates, omega and substeps
  mutable std::map<int, void *> step_tabs;
};

struct sr_rays {
  int64_t n = 0;
  int64_t cap = 0;       // rays the buffers were made for (sr_rays_create); sr_trace's pipeline runs a shorter last chunk with n < cap,
                         // and every buffer allocated later (sort_tmp, rec, rec2, order2) is sized by cap, never by the current n
  // launch positions' bounding box, (min x, y, z, max x, y, z), found at upload / generate: the rays per lateral cell of the
  // BEAM (not of the whole lateral grid) decide between the tile path and the per-ray kernel (trace.hip: tile_plan)
  double bbox[6] = {0, 0, 0, 0, 0, 0};
  bool have_bbox = false;
  bool bbox_given = false;  // sr_rays_set_bbox: the caller's word for the beam; stays across hand-offs (comm.hip, sr_rays_handoff_upload)
  double *s0 = nullptr;  // (9, N) original order
  // outputs are kept in LAUNCH order (coalesced); perm[j] = original index of launch slot j
  double *sf = nullptr;  // (9, N)
  double *rf = nullptr;  // (4, N)
  double *Jf = nullptr;  // (2, N, 2)
  uint32_t *perm = nullptr;
  uint32_t *keys = nullptr;
  uint32_t *bins = nullptr;  // counting-sort workspace: [coarse digit][workgroup] counts + scan totals
  uint32_t *sort_tmp = nullptr;  // (key, ray) pairs grouped by coarse digit, 2 x N
  int64_t bins_cap = 0;
  uint32_t *fb_list = nullptr;      // rays for the time-stepping fallback
  unsigned long long *counters = nullptr;  // plain words [1], [2]: queue lengths of a trace, [3]: first-level queue total; stripes: ray steps, deposited
  double *rec = nullptr;                   // (10, N) hand-off records (A12), allocated at first use
  double *rec2 = nullptr;                  // the records' second buffer and the new order, for the tile path's re-binning (trace_tile.inc)
  uint32_t *order2 = nullptr;
  // the tile path's binning: the packed lateral cell (ib | ic << 16; 0xFFFFFFFF: none) of every ray where the LAST binning found it,
  // by the ray's index (binning from s0) or by its place in the records it was binned from; the tile kernel places its tile from it
  uint32_t *cells = nullptr;
  bool have_cells = false;
  // the tile path's stragglers (trace_tile.inc): (10, cap) records of the rays a tile lost, in the order they were lost -- the state
  // they entered their segment with, then (k_trace_f64 on the side stream) their state on the volume's / slab's last node plane --
  // and the entry counts after each segment (what one straggler launch takes)
  double *strag_rec = nullptr;
  unsigned long long *strag_snap = nullptr;
  int strag_snap_cap = 0;
  bool have_s0 = false, traced = false, sorted = false, have_rec = false;
  bool have_order = false;  // a trace has been queued since the bundle was made / resized: perm[] is its launch order (sr_rays_launch_order)
  bool counters_carry = false;  // the step / fallback totals of earlier traces have not been read yet: keep adding
  int tile_segs = 0;  // the last trace ran the tile path in this many timed segments (0: not the tile path, or more than kMaxTileSegs)
  int tile_segs_run = 0;  // ... in this many segments, timed or not (sr_rays_tile_segments)
  bool tile_rec = false;  // ... with the records kernel (sr_rays_tile_records)
  // Edge guard (deposit.hip): per launch slot, a bound on how far the exit ANGLE of a ray traced by the mixed build may
  // be from the float64 build's [rad]; 0 for rays the float64 kernels wrote, +inf when the kernel keeps no bound.  With
  // it go what a re-trace needs: the volume and the parameters of the last trace (the volume must outlive the deposits).
  float *guard = nullptr;
  const sr_volume *last_vol = nullptr;
  sr_trace_params last_p{};
  void *guard_set = nullptr;             // sr_rays_refine: the diagnostics' chains and detector edges (device), and the host copy
  std::vector<char> guard_set_host;      // the upload reads
  bool guard_live = false;   // the last trace ran the mixed build on a whole volume: guard[] is meaningful
  double guard_len = 0;      // extent of the volume along the probing axis [m]: position bound = guard_len * angle bound
};

namespace sr {
int retrace_f64(const sr_rays *r, const uint32_t *list, const unsigned long long *count);  // trace.hip (edge guard)
int download_rows(const sr_rays *r, double *sf, double *rf, double *Jf, int64_t ld, int64_t off, double *staging);  // trace.hip
// deposit.hip: the A9 counts binning of DEVICE coordinates (x[i], y[i]) into a SR_IMG_COUNTS image (added to what it holds), the
// entries with skip[i] != 0 left out (skip may be NULL); *deposited (a device word the caller has zeroed) gets the number binned.
// Queued on `st`, not waited for.
int counts_deposit_device(const double *x, const double *y, const uint8_t *skip, int64_t n, sr_image *img,
                          unsigned long long *deposited, hipStream_t st);
}

struct sr_image {
  int kind = 0;
  int nx = 0, ny = 0;  // bins (counts, intensity) or edges (complex)
  int n_ch = 0;        // intensity: channels
  double x_lo = 0, x_hi = 0, y_lo = 0, y_hi = 0;
  void *d = nullptr;
  int64_t bytes = 0;
};

// A scalar or 3-vector field on a rectilinear grid (resample.hip creates and resamples it, emission.hip marches through it).
struct sr_field {
  int n[3] = {0, 0, 0};
  int n_comp = 1;
  bool is_f64 = false;
  void *data = nullptr;                        // (nx, ny, nz[, n_comp]) C order, the caller's dtype
  double *g[3] = {nullptr, nullptr, nullptr};  // node coordinates widened to float64
  std::vector<double> hg[3];                   // host copies of g (grids are compared without touching the device)
  double inv_h[3] = {0, 0, 0};                 // (n - 1) / (g[n-1] - g[0]): the first guess of a cell on a uniform axis
};

// ---- what the entry points of the field diagnostics share on the host (runtime.hip) ----------------------------------------
namespace sr {
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline bool positive(double v) { return std::isfinite(v) && v > 0.0; }

// The grid of a field as a kernel takes it (push.hip, thomson.hip): what sr::locate_in<true> reads, per axis.
struct FieldGrid {
  const double *g[3];  // node coordinates
  int n[3];
  double inv_h[3], lo[3], hi[3];  // lo = g[0], hi = g[n-1]: the box
};
FieldGrid grid_of(const sr_field *f);

// Every field given (f != NULL) has its n_comp, and the dtype and the grid of `ref` (one of them, named ref_name); before the
// device is touched.
struct FieldSpec {
  const char *name;
  const sr_field *f;
  int n_comp;
};
int check_fields(const char *who, const sr_field *ref, const char *ref_name, std::initializer_list<FieldSpec> fields);

// The pieces of one call's scratch block: take() them in order, each aligned to 256 bytes, then alloc() gets the block
// (sr::scratch) and sets every pointer taken; false + error text on failure.  A piece of 0 elements shares the next one's address.
class Carve {
 public:
  template <typename T>
  void take(T **p, size_t count) {
    slots_.push_back({(void **)p, bytes_});
    bytes_ += up256(sizeof(T) * count);
  }
  bool alloc();

 private:
  struct Slot {
    void **p;
    size_t at;
  };
  std::vector<Slot> slots_;
  size_t bytes_ = 0;
};

// The end of a timed call: the stream is waited for, *kernel_ms (may be NULL) gets the time between c.ev[0] and c.ev[1], the
// scratch block is trimmed.
int finish_timed(Context &c, double *kernel_ms);
}  // namespace sr
