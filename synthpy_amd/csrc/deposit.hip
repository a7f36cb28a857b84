// A7-A11 on the device: ray-transfer-matrix optics (rtm_solver.py:48-136 and the chains
// :197-286, :376-422), Rays.histogram = np.histogram2d (:156-178), Interferometry.interferogram
// (:424-453) and interfere_ref_beam (diagnostics.py:559-581).  Beyond the reference: analyser-weighted intensity images
// of the same rays and the rotation map of an analyser pair (k_deposit_intensity, k_intensity2d, k_rotation).
//
// Detector arithmetic is integer work downstream of a float64 coordinate, so the coordinate
// has to round exactly as the reference's: this file is compiled with -ffp-contract=off and
// fuses only where OpenBLAS' dgemm does (distance: x' = fma(d, theta, x); see the oracle, A7).
// Bin edges are numpy's linspace values i*step + lo (last edge = hi), recomputed per ray.
//
// Layout: the loaders and tests the kernels share (exit_ray, load_field / store_field, bin_hist2, guard_seed / guard_uncertain,
// add_hits); ONE skeleton for the fused deposits, deposit_patch (one ray per work-item, the workgroup's patch of the detector
// privatised in LDS), which a kernel gives a front end (bins ray i, says what it adds) and a patch type (tile shape and layout,
// what a hit adds to a tile bin and an image bin, how a flush item goes to the image); host side: sr::CallBuffers / sr::stage_out,
// read_out, deposit_begin / deposit_finish, guard_queue_reset, kernels picked by sr::with_flags / sr::with_count.
#include <algorithm>

#include "common.hpp"

namespace {

struct Chain {
  sr_optic op[SR_MAX_OPTICS];
  int n;
  double kwave;
};

struct RefBeam {
  double f, xw, yw;  // exp(1j * f * (xw*x + yw*y)) added to E_y
};
// the reference beams of one deposit, added in order (diagnostics.py:559-581; two_lens_solve adds (10, 20) after the caller's)
struct RefSet {
  int n;
  RefBeam b[SR_MAX_REF_BEAMS];
  __device__ __forceinline__ void add_to(double xm, double ym, double &er, double &ei) const {
    for (int q = 0; q < n; ++q) {  // uses self.rf, still in metres (diagnostics.py:579-581)
      double s, c;
      sincos(b[q].f * (b[q].xw * xm + b[q].yw * ym), &s, &c);
      er += c;
      ei += s;
    }
  }
};

struct Edges {
  double lo, hi, step;
  int n;  // number of bins
};

__device__ __forceinline__ double edge_at(const Edges &e, int i) { return i == e.n ? e.hi : (double)i * e.step + e.lo; }

__device__ __forceinline__ int walk(const Edges &e, double v) {
  int j = (int)((v - e.lo) / e.step);
  j = j < 0 ? 0 : (j > e.n - 1 ? e.n - 1 : j);
  while (j > 0 && v < edge_at(e, j)) --j;
  while (j < e.n - 1 && v >= edge_at(e, j + 1)) ++j;
  return j;
}
// np.histogramdd: searchsorted(edges, v, 'right'), last edge closed, outliers and NaN dropped
__device__ __forceinline__ int bin_hist(const Edges &e, double v) {
  if (!(v >= e.lo && v <= e.hi)) return -1;
  if (v == e.hi) return e.n - 1;
  return walk(e, v);
}
// np.digitize(v, edges) - 1 with the right edge open (rtm_solver.py:442-446)
__device__ __forceinline__ int bin_digitize(const Edges &e, double v) {
  if (!(v >= e.lo && v < e.hi)) return -1;
  return walk(e, v);
}

// could a coordinate within `err` of v fall in another bin (or on the other side of the detector's edge)?
__device__ __forceinline__ bool near_bin_edge(const Edges &e, double v, double err) {
  if (!(v == v)) return false;
  if (v < e.lo) return e.lo - v <= err;
  if (v > e.hi) return v - e.hi <= err;
  const int j = v == e.hi ? e.n - 1 : walk(e, v);
  return v - edge_at(e, j) <= err || edge_at(e, j + 1) - v <= err;
}

struct Ray4 {
  double x, th, y, ph;
  double e0r, e0i, e1r, e1i;
};

// The field factors exp(1j*k*|dr|) of the distance ops commute with everything else in a chain (lenses and masks do
// not touch a surviving ray's E), so their arguments are summed and ONE rotation is applied at the end: one sincos of
// a ~3e8 rad argument per ray instead of one per leg.  (Sum rounding ~6e-8 rad, the size of the reference's own
// rounding of each leg's argument.)
// EDGE GUARD.  The mixed build's exit ray differs from the float64 build's by at most (e_pos, e_ang) in position [mm] and
// angle [rad] on either axis (from the tracer's per-ray bound: trace_mx.inc).  Between its masks the chain is LINEAR,
// x = A*x0 + B*theta0 per axis, so the 2x2 ray-transfer matrices from the chain's start to the current optic are carried
// along (they depend on the chain only: wave-uniform) and the half-width of a coordinate there is |A|*e_pos + |B|*e_ang --
// no interval blow-up: an imaging chain has B = 0 on the detector whatever its legs.  `near` is set when a mask's decision
// or (after the chain) the bin could differ inside that half-width: such rays are traced again in float64 before they are
// counted (sr_rays_deposit).
struct Err4 {
  double e_pos, e_ang;                     // the tracer's bound for this ray
  double ax, bx, cx, dx, ay, by, cy, dy;   // x = ax*x0 + bx*th0, th = cx*x0 + dx*th0; the same for (y, phi)
  bool near;
  // a zero transfer coefficient contributes nothing even when the bound is +inf (0 * inf = NaN would make every compare false)
  static __device__ __forceinline__ double term(double coef, double e) { return coef != 0.0 ? fabs(coef) * e : 0.0; }
  __device__ __forceinline__ double hx() const { return term(ax, e_pos) + term(bx, e_ang); }
  __device__ __forceinline__ double hy() const { return term(ay, e_pos) + term(by, e_ang); }
};

template <bool WITH_E, bool GUARD = false>
__device__ __forceinline__ void apply_chain(const Chain &C, Ray4 &r, Err4 *g = nullptr) {
  double turn = 0.0;
  for (int o = 0; o < C.n; ++o) {
    const sr_optic q = C.op[o];
    bool kill = false;
    if (GUARD) {  // the decision of a mask is looked at BEFORE it is applied; a NaN ray compares false everywhere
      switch (q.op) {
        case SR_OP_DIST:
          g->ax = fma(q.a, g->cx, g->ax);
          g->bx = fma(q.a, g->dx, g->bx);
          g->ay = fma(q.a, g->cy, g->ay);
          g->by = fma(q.a, g->dy, g->by);
          break;
        case SR_OP_LENS:
          g->cx = fma(-1.0 / q.a, g->ax, g->cx);
          g->dx = fma(-1.0 / q.a, g->bx, g->dx);
          g->cy = fma(-1.0 / q.b, g->ay, g->cy);
          g->dy = fma(-1.0 / q.b, g->by, g->dy);
          break;
        case SR_OP_CIRC_AP:
        case SR_OP_CIRC_STOP:
          if (fabs(sqrt(r.x * r.x + r.y * r.y) - fabs(q.a)) <= g->hx() + g->hy()) g->near = true;
          break;
        case SR_OP_RECT_AP:
          if (fabs(fabs(r.x) - fabs(q.a)) <= g->hx() || fabs(fabs(r.y) - fabs(q.b)) <= g->hy()) g->near = true;
          break;
        case SR_OP_KNIFE:
          if (fabs((q.iarg == 0 ? r.x : r.y) - q.a) <= (q.iarg == 0 ? g->hx() : g->hy())) g->near = true;
          break;
        case SR_OP_SCALE:
          g->ax *= q.a;
          g->bx *= q.a;
          g->ay *= q.a;
          g->by *= q.a;
          break;
        default:
          break;
      }
    }
    switch (q.op) {
      case SR_OP_PHASE:
      case SR_OP_DIST: {
        const double xn = fma(q.a, r.th, r.x), yn = fma(q.a, r.ph, r.y);
        if (WITH_E && C.kwave > 0 && q.iarg == 0) {
          const double dx = xn - r.x, dy = yn - r.y;
          turn += C.kwave * sqrt(dx * dx + dy * dy);
        }
        if (q.op == SR_OP_DIST) {
          r.x = xn;
          r.y = yn;
        }
      } break;
      case SR_OP_LENS: {
        const double m1 = -1.0 / q.a, m2 = -1.0 / q.b;
        r.th = m1 * r.x + r.th;
        r.ph = m2 * r.y + r.ph;
      } break;
      case SR_OP_CIRC_AP:
        kill = (r.x * r.x + r.y * r.y > q.a * q.a);
        break;
      case SR_OP_CIRC_STOP:
        kill = (r.x * r.x + r.y * r.y < q.a * q.a);
        break;
      case SR_OP_RECT_AP:
        kill = (r.x * r.x > q.a * q.a) && (r.y * r.y > q.b * q.b);
        break;
      case SR_OP_KNIFE: {
        const double v = q.iarg == 0 ? r.x : r.y;
        kill = q.b > 0 ? (v > q.a) : (q.b < 0 ? (v < q.a) : false);
      } break;
      case SR_OP_SCALE:
        r.x = r.x * q.a;
        r.y = r.y * q.a;
        break;
      default:
        break;
    }
    if (kill) {
      const double nan = __builtin_nan("");
      r.x = r.th = r.y = r.ph = nan;
      if (WITH_E) r.e0r = r.e0i = r.e1r = r.e1i = nan;
    }
  }
  if (WITH_E && turn != 0.0) {
    double s, c;
    sincos(turn, &s, &c);
    double tr = r.e0r * c - r.e0i * s, ti = r.e0r * s + r.e0i * c;
    r.e0r = tr;
    r.e0i = ti;
    tr = r.e1r * c - r.e1i * s;
    ti = r.e1r * s + r.e1i * c;
    r.e1r = tr;
    r.e1i = ti;
  }
}

// ---- what the kernels of this file share ---------------------------------------------------------------------------
// the exit ray of launch slot i of a resident bundle, m_to_mm (rtm_solver.py:48-51); xm, ym: its position still in metres
__device__ __forceinline__ Ray4 exit_ray(const double *rf, int64_t N, int64_t i, double &xm, double &ym) {
  xm = rf[i];
  ym = rf[2 * N + i];
  return Ray4{xm * 1e3, rf[N + i], ym * 1e3, rf[3 * N + i], 0, 0, 0, 0};
}
__device__ __forceinline__ Ray4 exit_ray(const double *rf, int64_t N, int64_t i) {
  double xm, ym;
  return exit_ray(rf, N, i, xm, ym);
}
// E (2, N) complex: the field of ray i
__device__ __forceinline__ void load_field(const double *__restrict__ E, int64_t N, int64_t i, Ray4 &r) {
  r.e0r = E[2 * i];
  r.e0i = E[2 * i + 1];
  r.e1r = E[2 * (N + i)];
  r.e1i = E[2 * (N + i) + 1];
}
__device__ __forceinline__ void store_field(const Ray4 &r, double *__restrict__ E, int64_t N, int64_t i) {
  E[2 * i] = r.e0r;
  E[2 * i + 1] = r.e0i;
  E[2 * (N + i)] = r.e1r;
  E[2 * (N + i) + 1] = r.e1i;
}
// np.histogram2d's bins of (x, y): true for a hit; (bx, by) are left alone for a NaN coordinate
__device__ __forceinline__ bool bin_hist2(const Edges &ex, const Edges &ey, double x, double y, int &bx, int &by) {
  if (!(x == x && y == y)) return false;
  bx = bin_hist(ex, x);
  by = bin_hist(ey, y);
  return bx >= 0 && by >= 0;
}
// the hits of a launch: one atomic per wavefront into the striped total (reached by the whole wavefront)
__device__ __forceinline__ void add_hits(unsigned long long *__restrict__ counter, bool hit) {
  unsigned long long tot = hit ? 1ull : 0ull;
  for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
  if ((threadIdx.x & 63) == 0 && tot) atomicAdd(sr::stripe(counter, sr::kStripeDeposited), tot);
}

struct Guard {
  const float *bound;         // per launch slot: angle bound of the mixed build [rad]; 0 = a float64 result
  double len;                 // position bound = len * angle bound [m]
  uint32_t *list;             // the slots to trace again
  unsigned long long *count;
};
// the half-widths a ray with angle bound ea starts its chain with; 1.0000001: the few roundings of the half-widths themselves
__device__ __forceinline__ Err4 guard_seed(const Guard &G, double ea) {
  return Err4{1e3 * (G.len * ea) * 1.0000001, ea * 1.0000001, 1, 0, 0, 1, 1, 0, 0, 1, false};
}
// after apply_chain<false, true>(C, r, &g): could a mask's decision or the pixel differ from the float64 result's?
__device__ __forceinline__ bool guard_uncertain(const Err4 &g, const Edges &ex, const Edges &ey, const Ray4 &r) {
  return g.near || near_bin_edge(ex, r.x, g.hx()) || near_bin_edge(ey, r.y, g.hy());
}

// host-buffer optics: r (4,N) mm in/out, E (2,N) complex in/out
// (the field rows are spelled out: with load_field / store_field the compiler keeps a second scaled index alive across the
// chain, 51 VGPRs instead of 49)
template <bool WITH_E>
__global__ void k_optics(Chain C, int64_t N, const double *__restrict__ rin, const double *__restrict__ Ein,
                         double *__restrict__ rout, double *__restrict__ Eout) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  Ray4 r{rin[i], rin[N + i], rin[2 * N + i], rin[3 * N + i], 0, 0, 0, 0};
  if (WITH_E) {
    r.e0r = Ein[2 * i];
    r.e0i = Ein[2 * i + 1];
    r.e1r = Ein[2 * (N + i)];
    r.e1i = Ein[2 * (N + i) + 1];
  }
  apply_chain<WITH_E>(C, r);
  rout[i] = r.x;
  rout[N + i] = r.th;
  rout[2 * N + i] = r.y;
  rout[3 * N + i] = r.ph;
  if (WITH_E) {
    Eout[2 * i] = r.e0r;
    Eout[2 * i + 1] = r.e0i;
    Eout[2 * (N + i)] = r.e1r;
    Eout[2 * (N + i) + 1] = r.e1i;
  }
}

__global__ void k_hist2d(const double *__restrict__ x, const double *__restrict__ y, int64_t N, Edges ex, Edges ey,
                         uint32_t *__restrict__ H) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  int bx, by;
  if (bin_hist2(ex, ey, x[i], y[i], bx, by)) atomicAdd(&H[(int64_t)by * ex.n + bx], 1u);
}
// the same binning of coordinates that are already on the device, entries with skip[i] != 0 left out (sr::counts_deposit_device);
// a grid-stride loop, so the hits of a launch are one atomic per wavefront of a bounded grid
__global__ __launch_bounds__(256) void k_hist2d_device(const double *__restrict__ x, const double *__restrict__ y,
                                                       const uint8_t *__restrict__ skip, int64_t N, Edges ex, Edges ey,
                                                       uint32_t *__restrict__ H, unsigned long long *__restrict__ deposited) {
  unsigned long long mine = 0ull;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    int bx, by;
    if ((skip == nullptr || skip[i] == 0) && bin_hist2(ex, ey, x[i], y[i], bx, by)) {
      atomicAdd(&H[(int64_t)by * ex.n + bx], 1u);
      ++mine;
    }
  }
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(deposited, mine);
}

__global__ void k_interferogram(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ E,
                                int64_t N, Edges ex, Edges ey, double *__restrict__ amp) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int bx = bin_digitize(ex, x[i]), by = bin_digitize(ey, y[i]);
  if (bx < 0 || by < 0) return;
  const int64_t plane = (int64_t)ex.n * ey.n, p = (int64_t)by * ex.n + bx;
  unsafeAtomicAdd(&amp[2 * p], E[2 * i]);
  unsafeAtomicAdd(&amp[2 * p + 1], E[2 * i + 1]);
  unsafeAtomicAdd(&amp[2 * (plane + p)], E[2 * (N + i)]);
  unsafeAtomicAdd(&amp[2 * (plane + p) + 1], E[2 * (N + i) + 1]);
}

// H = sqrt(Re(Ax)^2 + Re(Ay)^2)  (rtm_solver.py:450)
__global__ void k_amplitude(const double *__restrict__ amp, int64_t plane, double *__restrict__ H) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= plane) return;
  const double ax = amp[2 * p], ay = amp[2 * (plane + p)];
  H[p] = sqrt(ax * ax + ay * ay);
}

__global__ void k_ref_beam(const double *__restrict__ x, const double *__restrict__ y, int64_t N, RefBeam R,
                           double *__restrict__ E) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  const double arg = R.f * (R.xw * x[i] + R.yw * y[i]);
  double s, c;
  sincos(arg, &s, &c);
  E[2 * (N + i)] += c;
  E[2 * (N + i) + 1] += s;
}

// sr_rays_optics: the deposit's front end (m_to_mm -> reference beams -> chain) on a resident bundle, written in the ORIGINAL
// ray order (perm[j] = original index of launch slot j) for the host
template <bool WITH_E>
__global__ __launch_bounds__(256) void k_rays_optics(Chain C, RefSet R, int64_t N, const double *__restrict__ rf, const double *__restrict__ Jf,
                                                     const uint32_t *__restrict__ perm, double *__restrict__ rout, double *__restrict__ Eout) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= N) return;
  double xm, ym;
  Ray4 r = exit_ray(rf, N, j, xm, ym);
  if (WITH_E) {
    load_field(Jf, N, j, r);
    R.add_to(xm, ym, r.e1r, r.e1i);
  }
  apply_chain<WITH_E>(C, r);
  const int64_t i = perm[j];
  rout[i] = r.x;
  rout[N + i] = r.th;
  rout[2 * N + i] = r.y;
  rout[3 * N + i] = r.ph;
  if (WITH_E) store_field(r, Eout, N, i);
}

__global__ void k_counts_f64(const uint32_t *__restrict__ cnt, int64_t n, double *__restrict__ H) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p < n) H[p] = (double)cnt[p];
}

// Fused deposits: exit-plane rays in HBM (metres) -> m_to_mm -> [reference beam] -> chain -> detector, one ray per work-item.
//
// The rays arrive in launch order, i.e. binned by entry cell, and the imaging chains map neighbouring rays
// to neighbouring pixels, so the 256 hits of a workgroup fall in a compact patch of the detector.  With
// TILED the workgroup privatises that patch in LDS: the patch origin is the minimum (bx, by) over the
// workgroup (LDS atomicMin), hits inside the TW x TH tile are LDS atomics, the few outside it go straight
// to HBM, and the tile is flushed with one global atomic per NON-EMPTY flush item, row by row (coalesced).
// Integer counts are order-independent, so the image is bit-identical with and without tiles; the float64
// images sum in a different order (float64 atomics either way).  A zero contribution is skipped everywhere (x + 0 = x).
//
// A PATCH TYPE says what is deposited: the tile's shape TW x TH, its LDS cells (kCells of Cell, kPlanes planes of TW*TH flush
// items), what a hit carries (Val), and add_tile(tile, bin in the tile, v), add_image(bin in the image, v), flush(tile, plane,
// bin in the tile, bin in the image).  Layout and flush order decide the LDS banks and the atomics' pattern: they are the
// patch type's, not the skeleton's.
constexpr int kTileW = 64, kTileH = 32;   // counts: 2048 bins, 8 KiB of LDS
constexpr int kCTileW = 32, kCTileH = 16;  // complex: 512 bins x 4 doubles, 16 KiB of LDS
constexpr int kITileW = 32, kITileH = 16;  // intensity: 512 bins x NCH doubles (16 KiB at four channels: the complex tile's known-good size)

struct CountsPatch {
  static constexpr int TW = kTileW, TH = kTileH, kPlanes = 1, kCells = TW * TH;
  using Cell = uint32_t;  // of the tile and of the image
  struct Val {};
  uint32_t *__restrict__ img;
  __device__ __forceinline__ void add_tile(Cell *tile, int t, const Val &) const { atomicAdd(&tile[t], 1u); }
  __device__ __forceinline__ void add_image(int64_t p, const Val &) const { atomicAdd(&img[p], 1u); }
  __device__ __forceinline__ void flush(const Cell *tile, int, int t, int64_t p) const {
    const uint32_t cnt = tile[t];
    if (cnt) atomicAdd(&img[p], cnt);
  }
};

// (2, ny, nx) complex image; the tile is [bin][4] interleaved: {Re Ex, Im Ex, Re Ey, Im Ey} of a bin side by side
struct ComplexPatch {
  static constexpr int TW = kCTileW, TH = kCTileH, kPlanes = 1, kCells = TW * TH * 4;
  using Cell = double;
  using Val = Ray4;  // the ray's field
  double *__restrict__ img;
  int64_t plane;
  // E_x of an unrotated ray is exactly -0: skipping zeros saves half of the atomics
  static __device__ __forceinline__ void add(double *x, double *y, double e0r, double e0i, double e1r, double e1i) {
    if (e0r != 0.0) unsafeAtomicAdd(&x[0], e0r);
    if (e0i != 0.0) unsafeAtomicAdd(&x[1], e0i);
    if (e1r != 0.0) unsafeAtomicAdd(&y[0], e1r);
    if (e1i != 0.0) unsafeAtomicAdd(&y[1], e1i);
  }
  __device__ __forceinline__ void add_tile(Cell *tile, int t, const Val &r) const {
    double *s = tile + (size_t)t * 4;
    add(s, s + 2, r.e0r, r.e0i, r.e1r, r.e1i);
  }
  __device__ __forceinline__ void add_image(int64_t p, const Val &r) const {
    add(img + 2 * p, img + 2 * (plane + p), r.e0r, r.e0i, r.e1r, r.e1i);
  }
  __device__ __forceinline__ void flush(const Cell *tile, int, int t, int64_t p) const {
    const double *s = tile + (size_t)t * 4;
    if (s[0] != 0.0 || s[1] != 0.0 || s[2] != 0.0 || s[3] != 0.0) add(img + 2 * p, img + 2 * (plane + p), s[0], s[1], s[2], s[3]);
  }
};

// (NCH, ny, nx) float64 image; the tile is [channel][bin] planar and flushed channel by channel
template <int NCH>
struct IntensityPatch {
  static constexpr int TW = kITileW, TH = kITileH, kPlanes = NCH, kCells = TW * TH * NCH;
  using Cell = double;
  struct Val {
    double w[NCH];
  };
  double *__restrict__ img;
  int64_t plane;
  __device__ __forceinline__ void add_tile(Cell *tile, int t, const Val &v) const {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (v.w[c] != 0.0) unsafeAtomicAdd(&tile[c * (TW * TH) + t], v.w[c]);
  }
  __device__ __forceinline__ void add_image(int64_t p, const Val &v) const {
    double *g = img + p;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (v.w[c] != 0.0) unsafeAtomicAdd(&g[c * plane], v.w[c]);
  }
  __device__ __forceinline__ void flush(const Cell *tile, int c, int t, int64_t p) const {
    const double s = tile[c * (TW * TH) + t];
    if (s != 0.0) unsafeAtomicAdd(&img[c * plane + p], s);
  }
};

template <int KIND>
using ImagePatch = std::conditional_t<KIND == SR_IMG_COMPLEX, ComplexPatch, CountsPatch>;  // of an sr_image kind (k_deposit)

// The skeleton.  front(i, bx, by, v) is called by EVERY work-item, out-of-range ones included (the edge guard's queue_push must
// be reached by the whole wavefront); it leaves (bx, by) at (-1, -1) unless ray i hits the detector, and in v what the hit adds.
template <bool TILED, typename Patch, typename Front>
__device__ __forceinline__ void deposit_patch(const Edges &ex, const Edges &ey, const Patch &P, unsigned long long *__restrict__ counter,
                                              Front &&front) {
  constexpr int TW = Patch::TW, TH = Patch::TH, TB = TW * TH;
  __shared__ int org[2];
  __shared__ typename Patch::Cell tile[TILED ? Patch::kCells : 1];
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (TILED) {
    if (threadIdx.x < 2) org[threadIdx.x] = 0x7fffffff;
    for (int t = threadIdx.x; t < Patch::kCells; t += blockDim.x) tile[t] = 0;
    __syncthreads();
  }
  int bx = -1, by = -1;
  typename Patch::Val v{};
  front(i, bx, by, v);
  const bool hit = bx >= 0 && by >= 0;
  int tx = -1, ty = -1;
  if (TILED) {
    if (hit) {
      atomicMin(&org[0], bx);
      atomicMin(&org[1], by);
    }
    __syncthreads();
    tx = bx - org[0];
    ty = by - org[1];
  }
  const bool in_tile = TILED && hit && tx < TW && ty < TH;  // tx, ty >= 0 by construction of the origin
  if (hit) {
    if (in_tile)
      P.add_tile(tile, ty * TW + tx, v);
    else
      P.add_image((int64_t)by * ex.n + bx, v);
  }
  if (TILED) {
    __syncthreads();
    const int ox = org[0], oy = org[1];
    if (ox != 0x7fffffff) {  // at least one hit in this workgroup
      for (int q = threadIdx.x; q < TB * Patch::kPlanes; q += blockDim.x) {
        const int c = q / TB, t = q % TB;
        const int gx = ox + t % TW, gy = oy + t / TW;
        if (gx >= ex.n || gy >= ey.n) continue;  // the tile overhangs the detector
        P.flush(tile, c, t, (int64_t)gy * ex.n + gx);
      }
    }
  }
  add_hits(counter, hit);
}

// counts (np.histogram2d's binning; GUARD: the edge guard queues the rays whose pixel is not certain, which are counted after
// their float64 re-trace by k_deposit_list) or the complex image (np.digitize's binning, reference beams, field factors)
template <int KIND, bool TILED, bool GUARD = false>
__global__ __launch_bounds__(256) void k_deposit(Chain C, RefSet R, int64_t N, const double *__restrict__ rf,
                                                 const double *__restrict__ Jf, Edges ex, Edges ey,
                                                 typename ImagePatch<KIND>::Cell *__restrict__ img,
                                                 unsigned long long *__restrict__ counter, Guard G) {
  if constexpr (KIND == SR_IMG_COMPLEX) {
    deposit_patch<TILED>(ex, ey, ComplexPatch{img, (int64_t)ex.n * ey.n}, counter, [&](int64_t i, int &bx, int &by, Ray4 &r) {
      if (i >= N) return;
      double xm, ym;
      r = exit_ray(rf, N, i, xm, ym);
      load_field(Jf, N, i, r);
      R.add_to(xm, ym, r.e1r, r.e1i);
      apply_chain<true>(C, r);
      bx = bin_digitize(ex, r.x);
      by = bin_digitize(ey, r.y);
    });
  } else {
    deposit_patch<TILED>(ex, ey, CountsPatch{img}, counter, [&](int64_t i, int &bx, int &by, CountsPatch::Val &) {
      bool again = false;
      if (i < N) {
        Ray4 r = exit_ray(rf, N, i);
        const double ea = GUARD ? (double)G.bound[i] : 0.0;
        if (!(ea < INFINITY)) {  // a kernel that keeps no bound (sub-steps, optional terms): every such ray is traced again
          again = true;
        } else if (ea > 0.0) {  // a mixed-precision result: is its pixel (and every mask's decision) the float64 result's as well?
          Err4 g = guard_seed(G, ea);
          apply_chain<false, true>(C, r, &g);
          again = guard_uncertain(g, ex, ey, r);
        } else {
          apply_chain<false>(C, r);
        }
        if (!again) bin_hist2(ex, ey, r.x, r.y, bx, by);
      }
      if (GUARD) sr::queue_push(G.count, G.list, again, (uint32_t)i);  // must be reached by the whole wavefront
    });
  }
}

// counts deposit of the launch slots list[0..*count): the rays the edge guard had traced again (few; global atomics)
__global__ __launch_bounds__(256) void k_deposit_list(Chain C, int64_t N, const double *__restrict__ rf, Edges ex, Edges ey,
                                                      uint32_t *__restrict__ img, unsigned long long *__restrict__ counter,
                                                      const uint32_t *__restrict__ list, const unsigned long long *__restrict__ count) {
  const unsigned long long n = *count;
  unsigned long long hits = 0;
  for (unsigned long long t = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; t < n; t += (unsigned long long)gridDim.x * blockDim.x) {
    Ray4 r = exit_ray(rf, N, list[t]);
    apply_chain<false>(C, r);
    int bx, by;
    if (bin_hist2(ex, ey, r.x, r.y, bx, by)) {
      atomicAdd(&img[(int64_t)by * ex.n + bx], 1u);
      ++hits;
    }
  }
  if (hits) atomicAdd(sr::stripe(counter, sr::kStripeDeposited), hits);
}

// ---- polarimetry: analyser-weighted intensity images (no reference counterpart) ------------------------------------
// Channel c holds the analyser's transmission axis (a, b) = (-sin beta, cos beta); a ray's weight there is
// |a E_x + b E_y|^2, or |E_x|^2 + |E_y|^2 for a channel without analyser (a NaN).  The sums are incoherent: the field
// factors of a chain's legs have modulus 1 and drop out, so the masks-only chain is all a ray needs.
struct Analysers {
  double a[SR_MAX_ANALYSERS], b[SR_MAX_ANALYSERS];
};

__device__ __forceinline__ double analyser_weight(const Analysers &A, int c, const Ray4 &r) {
  const double a = A.a[c], b = A.b[c];
  if (a != a) return (r.e0r * r.e0r + r.e0i * r.e0i) + (r.e1r * r.e1r + r.e1i * r.e1i);
  const double re = a * r.e0r + b * r.e1r, im = a * r.e0i + b * r.e1i;
  return re * re + im * im;
}

// host-array form (sr_intensity2d): x, y already through the chain, np.histogram2d's binning with weights
template <int NCH>
__global__ void k_intensity2d(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ E, int64_t N,
                              Edges ex, Edges ey, Analysers A, double *__restrict__ I) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  int bx, by;
  if (!bin_hist2(ex, ey, x[i], y[i], bx, by)) return;
  const int64_t plane = (int64_t)ex.n * ey.n, p = (int64_t)by * ex.n + bx;
  Ray4 r{};
  load_field(E, N, i, r);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const double w = analyser_weight(A, c, r);
    if (w != 0.0) unsafeAtomicAdd(&I[c * plane + p], w);
  }
}

// Fused intensity deposit: masks-only chain -> bin_hist -> NCH weighted float64 sums per ray in ONE pass over the rays
template <int NCH, bool TILED>
__global__ __launch_bounds__(256) void k_deposit_intensity(Chain C, int64_t N, const double *__restrict__ rf,
                                                           const double *__restrict__ Jf, Edges ex, Edges ey, Analysers A,
                                                           double *__restrict__ img, unsigned long long *__restrict__ counter) {
  using Patch = IntensityPatch<NCH>;
  deposit_patch<TILED>(ex, ey, Patch{img, (int64_t)ex.n * ey.n}, counter, [&](int64_t i, int &bx, int &by, typename Patch::Val &v) {
    if (i >= N) return;
    Ray4 r = exit_ray(rf, N, i);
    apply_chain<false>(C, r);
    if (!bin_hist2(ex, ey, r.x, r.y, bx, by)) return;
    load_field(Jf, N, i, r);
#pragma unroll
    for (int c = 0; c < NCH; ++c) v.w[c] = analyser_weight(A, c, r);
  });
}

// Rotation map of two analyser channels at +beta and -beta (sr_image_rotation): D = (I+ - I-)/(I+ + I-),
// R = hypot(sin 2b, D cos 2b), delta = atan2(D cos 2b, sin 2b), alpha = (delta + asin(D/R))/2; NaN where I+ + I- == 0
__global__ void k_rotation(const double *__restrict__ Ip, const double *__restrict__ Im, int64_t plane, double s2b, double c2b,
                           double *__restrict__ alpha) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= plane) return;
  const double tot = Ip[p] + Im[p];
  if (tot == 0.0) {
    alpha[p] = __builtin_nan("");
    return;
  }
  const double D = (Ip[p] - Im[p]) / tot, dc = D * c2b;
  const double R = hypot(s2b, dc);
  const double q = fmin(1.0, fmax(-1.0, D / R));  // |D| <= R up to the rounding of the hypot
  alpha[p] = 0.5 * (atan2(dc, s2b) + asin(q));
}

// Edge guard for SEVERAL counts diagnostics at once (sr_rays_refine): a ray is queued when its pixel or a mask's decision is
// not certain for ANY of them; one float64 re-trace then serves every deposit that follows.
struct GuardSet {
  Chain C[SR_MAX_REFINE];
  Edges ex[SR_MAX_REFINE], ey[SR_MAX_REFINE];
  int n;
};
__global__ __launch_bounds__(256) void k_guard_flags(const GuardSet *__restrict__ S, int64_t N, const double *__restrict__ rf, Guard G) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  bool again = false;
  if (i < N) {
    const double ea = (double)G.bound[i];
    if (!(ea < INFINITY)) {
      again = true;
    } else if (ea > 0.0) {
      for (int q = 0; q < S->n && !again; ++q) {
        Ray4 r = exit_ray(rf, N, i);
        Err4 g = guard_seed(G, ea);
        apply_chain<false, true>(S->C[q], r, &g);
        again = guard_uncertain(g, S->ex[q], S->ey[q], r);
      }
    }
  }
  sr::queue_push(G.count, G.list, again, (uint32_t)i);
}

int make_chain(const sr_optic *chain, int n_ops, double kwave, Chain &C) {
  SR_CHECK(n_ops >= 0 && n_ops <= SR_MAX_OPTICS, "optic chain length %d out of range (0..%d)", n_ops, SR_MAX_OPTICS);
  SR_CHECK(n_ops == 0 || chain != nullptr, "optic chain is NULL");
  C.n = n_ops;
  C.kwave = kwave;
  for (int i = 0; i < n_ops; ++i) {
    SR_CHECK(chain[i].op >= SR_OP_DIST && chain[i].op <= SR_OP_PHASE, "unknown optic op %d at position %d", chain[i].op, i);
    if (chain[i].op == SR_OP_LENS) SR_CHECK(chain[i].a != 0 && chain[i].b != 0, "lens focal length must be non-zero");
    C.op[i] = chain[i];
  }
  return SR_OK;
}

RefBeam make_ref(double n_fringes, double deg) {
  RefBeam R{0, 0, 0};
  if (deg >= 45) deg = -fabs(deg - 90);
  const double rad = deg * M_PI / 180;
  R.yw = atan(rad);
  R.xw = sqrt(1 - R.yw * R.yw);
  R.f = 2 * n_fringes / 3;
  return R;
}
int make_refs(const sr_deposit_params *p, RefSet &R) {
  R.n = 0;
  for (auto &b : R.b) b = RefBeam{0, 0, 0};
  if (!p) return SR_OK;
  SR_CHECK(p->ref_on >= 0 && p->ref_on <= SR_MAX_REF_BEAMS, "ref_on = %d: at most %d reference beams", p->ref_on, SR_MAX_REF_BEAMS);
  R.n = p->ref_on;
  for (int q = 0; q < R.n; ++q) R.b[q] = make_ref(p->ref_n_fringes[q], p->ref_deg[q]);
  return SR_OK;
}

Edges make_edges(double lo, double hi, int nbins) {
  return Edges{lo, hi, (hi - lo) / nbins, nbins};  // step: np.linspace's delta / div
}

int make_analysers(const double *ab, int n_ch, Analysers &A) {
  SR_CHECK(ab != nullptr && n_ch >= 1 && n_ch <= SR_MAX_ANALYSERS, "analysers: %d channels (1..%d), or NULL", n_ch, SR_MAX_ANALYSERS);
  for (int c = 0; c < SR_MAX_ANALYSERS; ++c) A.a[c] = A.b[c] = 0.0;
  for (int c = 0; c < n_ch; ++c) {
    A.a[c] = ab[2 * c];
    A.b[c] = ab[2 * c + 1];
    SR_CHECK((A.a[c] != A.a[c]) == (A.b[c] != A.b[c]), "analyser %d: (a, b) must both be NaN (no analyser) or both finite", c);
  }
  return SR_OK;
}

// ---- staging of the host-array entry points: sr::CallBuffers and sr::stage_out (common.hpp), and ---------------------------
// n doubles for the host: fill(d, grid, st) launches the kernel that writes them into the call's scratch block (256 per workgroup)
template <typename Fill>
int read_out(double *host, int64_t n, Fill &&fill) {
  hipStream_t st = sr::ctx().stream;
  double *d = static_cast<double *>(sr::scratch(sizeof(double) * n));
  if (!d) return SR_ERR_HIP;
  fill(d, dim3(sr::grid_for(n, 256)), st);
  return sr::stage_out(st, {{host, d, sizeof(double) * n}});
}

// ---- what the bundle deposits share --------------------------------------------------------------------------------------
// the edge guard's queue of a bundle, emptied: its length (and the re-trace's own queue after it) and the re-trace's step total
int guard_queue_reset(const sr_rays *r, hipStream_t st) {
  SR_HIP(hipMemsetAsync(sr::counter_word(r->counters, sr::kGuardQueue), 0, 2 * sizeof(unsigned long long), st));
  SR_HIP(hipMemsetAsync(sr::stripe_base(r->counters, sr::kStripeRetrace), 0, sr::kStripeBytes, st));
  return SR_OK;
}
Guard guard_of(const sr_rays *r) { return Guard{r->guard, r->guard_len, r->fb_list, sr::counter_word(r->counters, sr::kGuardQueue)}; }

// A timed bundle deposit: begin resets the stats and (unless the bundle is empty: nothing else happens then) the `deposited`
// total and records the start; finish records the end and, when stats are asked for, waits and fills them in.
int deposit_begin(const sr_rays *r, sr_deposit_stats *stats) {
  if (stats) *stats = sr_deposit_stats{0.0, 0, 0};
  if (r->n == 0) return SR_OK;
  sr::Context &c = sr::ctx();
  SR_HIP(hipMemsetAsync(sr::stripe_base(r->counters, sr::kStripeDeposited), 0, sr::kStripeBytes, c.stream));
  SR_HIP(hipEventRecord(c.ev[0], c.stream));
  return SR_OK;
}
int deposit_finish(const sr_rays *r, sr_deposit_stats *stats, bool guarded) {
  sr::Context &c = sr::ctx();
  SR_HIP(hipGetLastError());
  SR_HIP(hipEventRecord(c.ev[1], c.stream));
  if (!stats) return SR_OK;
  std::vector<unsigned long long> hw(sr::kCounterWords, 0ull);
  SR_HIP(hipMemcpyAsync(hw.data(), r->counters, sizeof(unsigned long long) * sr::kCounterWords, hipMemcpyDeviceToHost, c.stream));
  SR_HIP(hipStreamSynchronize(c.stream));
  float ms = 0.f;
  SR_HIP(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
  stats->kernel_ms = ms;
  stats->deposited = (int64_t)sr::stripe_sum(hw.data(), sr::kStripeDeposited);
  stats->retraced = guarded ? (int64_t)hw[sr::kGuardQueue] : 0;
  return SR_OK;
}

// the device buffer of a new image, zeroed (sr_image_create, sr_image_create_intensity)
int image_alloc(sr_image **out, int kind, int n_ch, int nx, int ny, double x_lo, double x_hi, double y_lo, double y_hi, int64_t bytes) {
  int rc = sr::ensure_init();
  if (rc) return rc;
  void *d = nullptr;
  hipError_t e = sr::dev_alloc_bytes(&d, (size_t)bytes);
  if (e != hipSuccess) return sr::fail(SR_ERR_HIP, "sr_image_create: allocating %lld bytes failed: %s", (long long)bytes, hipGetErrorString(e));
  e = hipMemsetAsync(d, 0, (size_t)bytes, sr::ctx().stream);
  if (e != hipSuccess) {
    sr::dev_free(d);
    return sr::fail(SR_ERR_HIP, "sr_image_create: memset failed: %s", hipGetErrorString(e));
  }
  *out = new sr_image{kind, nx, ny, n_ch, x_lo, x_hi, y_lo, y_hi, d, bytes};
  return SR_OK;
}

}  // namespace

int sr::counts_deposit_device(const double *x, const double *y, const uint8_t *skip, int64_t n, sr_image *img,
                              unsigned long long *deposited, hipStream_t st) {
  SR_CHECK(img != nullptr && img->kind == SR_IMG_COUNTS, "counts_deposit_device: needs a counts image");
  if (n <= 0) return SR_OK;
  const unsigned grid = (unsigned)std::min<int64_t>(sr::grid_for(n, 256), 1024);
  hipLaunchKernelGGL(k_hist2d_device, dim3(grid), dim3(256), 0, st, x, y, skip, n, make_edges(img->x_lo, img->x_hi, img->nx),
                     make_edges(img->y_lo, img->y_hi, img->ny), static_cast<uint32_t *>(img->d), deposited);
  SR_HIP(hipGetLastError());
  return SR_OK;
}

extern "C" {

int sr_optics(const sr_optic *chain, int n_ops, double kwave, int64_t N, const double *r_in, const double *E_in,
              double *r_out, double *E_out) {
  SR_CHECK(N >= 0 && r_in && r_out, "sr_optics: bad argument");
  SR_CHECK((E_in == nullptr) == (E_out == nullptr), "sr_optics: E_in and E_out must both be given or both NULL");
  Chain C;
  int rc = make_chain(chain, n_ops, kwave, C);
  if (rc) return rc;
  if (N == 0) return SR_OK;
  if ((rc = sr::ensure_init())) return rc;
  hipStream_t st = sr::ctx().stream;
  sr::CallBuffers buf;
  double *dr = nullptr, *dE = nullptr;
  const size_t rb = sizeof(double) * 4 * N;
  SR_RC(buf.upload(&dr, r_in, 4 * (size_t)N, st));
  SR_RC(buf.upload(&dE, E_in, 4 * (size_t)N, st));
  sr::with_flags(
      [&](auto with_e) {
        hipLaunchKernelGGL((k_optics<with_e.value>), dim3(sr::grid_for(N, 256)), dim3(256), 0, st, C, N, (const double *)dr,
                           (const double *)dE, dr, dE);
      },
      E_in != nullptr);
  return sr::stage_out(st, {{r_out, dr, rb}, {E_out, dE, rb}});
}

int sr_hist2d(const double *x, const double *y, int64_t N, int nxb, int nyb, double x_lo, double x_hi, double y_lo,
              double y_hi, uint32_t *H) {
  SR_CHECK(N >= 0 && (N == 0 || (x && y)) && H, "sr_hist2d: bad argument");
  SR_CHECK(nxb >= 1 && nyb >= 1, "sr_hist2d: bins must be positive");
  SR_CHECK(x_hi > x_lo && y_hi > y_lo, "sr_hist2d: empty range");
  int rc = sr::ensure_init();
  if (rc) return rc;
  hipStream_t st = sr::ctx().stream;
  sr::CallBuffers buf;
  double *dx = nullptr, *dy = nullptr;
  uint32_t *dH = nullptr;
  const size_t bins = (size_t)nxb * nyb;
  SR_RC(buf.zeroed(&dH, bins, st));
  if (N > 0) {
    SR_RC(buf.upload(&dx, x, (size_t)N, st));
    SR_RC(buf.upload(&dy, y, (size_t)N, st));
    hipLaunchKernelGGL(k_hist2d, dim3(sr::grid_for(N, 256)), dim3(256), 0, st, (const double *)dx, (const double *)dy, N,
                       make_edges(x_lo, x_hi, nxb), make_edges(y_lo, y_hi, nyb), dH);
  }
  return sr::stage_out(st, {{H, dH, sizeof(uint32_t) * bins}});
}

int sr_interferogram(const double *x, const double *y, const double *E, int64_t N, int nxe, int nye, double x_lo,
                     double x_hi, double y_lo, double y_hi, double *amp, double *H) {
  SR_CHECK(N >= 0 && (N == 0 || (x && y && E)) && (amp || H), "sr_interferogram: bad argument");
  SR_CHECK(nxe >= 2 && nye >= 2, "sr_interferogram: need at least 2 edges per axis");
  SR_CHECK(x_hi > x_lo && y_hi > y_lo, "sr_interferogram: empty range");
  int rc = sr::ensure_init();
  if (rc) return rc;
  hipStream_t st = sr::ctx().stream;
  sr::CallBuffers buf;
  double *dx = nullptr, *dy = nullptr, *dE = nullptr, *dA = nullptr;
  const int64_t plane = (int64_t)(nxe - 1) * (nye - 1);
  const size_t ab = sizeof(double) * 4 * (size_t)plane;
  SR_RC(buf.zeroed(&dA, 4 * (size_t)plane, st));
  if (N > 0) {
    SR_RC(buf.upload(&dx, x, (size_t)N, st));
    SR_RC(buf.upload(&dy, y, (size_t)N, st));
    SR_RC(buf.upload(&dE, E, 4 * (size_t)N, st));
    hipLaunchKernelGGL(k_interferogram, dim3(sr::grid_for(N, 256)), dim3(256), 0, st, (const double *)dx, (const double *)dy,
                       (const double *)dE, N, make_edges(x_lo, x_hi, nxe - 1), make_edges(y_lo, y_hi, nye - 1), dA);
  }
  if (!H) return sr::stage_out(st, {{amp, dA, ab}});
  SR_HIP(hipGetLastError());
  if (amp) SR_HIP(hipMemcpyAsync(amp, dA, ab, hipMemcpyDeviceToHost, st));
  return read_out(H, plane, [&](double *dH, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL(k_amplitude, grid, dim3(256), 0, s, (const double *)dA, plane, dH);
  });
}

int sr_interfere_ref_beam(const double *x, const double *y, int64_t N, double n_fringes, double deg, double *E) {
  SR_CHECK(N >= 0 && (N == 0 || (x && y && E)), "sr_interfere_ref_beam: bad argument");
  if (N == 0) return SR_OK;
  int rc = sr::ensure_init();
  if (rc) return rc;
  hipStream_t st = sr::ctx().stream;
  sr::CallBuffers buf;
  double *dx = nullptr, *dy = nullptr, *dE = nullptr;
  SR_RC(buf.upload(&dx, x, (size_t)N, st));
  SR_RC(buf.upload(&dy, y, (size_t)N, st));
  SR_RC(buf.upload(&dE, E, 4 * (size_t)N, st));
  hipLaunchKernelGGL(k_ref_beam, dim3(sr::grid_for(N, 256)), dim3(256), 0, st, (const double *)dx, (const double *)dy, N,
                     make_ref(n_fringes, deg), dE);
  return sr::stage_out(st, {{E, dE, sizeof(double) * 4 * N}});
}

// ---- device-resident images -------------------------------------------------------------
void sr_image_destroy(sr_image *img) {
  if (!img) return;
  sr::dev_free(img->d);
  delete img;
}

int sr_image_create(sr_image **out, int kind, int nx, int ny, double x_lo, double x_hi, double y_lo, double y_hi) {
  SR_CHECK(out != nullptr, "sr_image_create: NULL out");
  *out = nullptr;
  SR_CHECK(kind == SR_IMG_COUNTS || kind == SR_IMG_COMPLEX, "sr_image_create: unknown kind %d", kind);
  SR_CHECK(x_hi > x_lo && y_hi > y_lo, "sr_image_create: empty range");
  if (kind == SR_IMG_COUNTS)
    SR_CHECK(nx >= 1 && ny >= 1, "sr_image_create: bins must be positive");
  else
    SR_CHECK(nx >= 2 && ny >= 2, "sr_image_create: need at least 2 edges per axis");
  return image_alloc(out, kind, 0, nx, ny, x_lo, x_hi, y_lo, y_hi,
                     kind == SR_IMG_COUNTS ? (int64_t)sizeof(uint32_t) * nx * ny : (int64_t)sizeof(double) * 4 * (nx - 1) * (ny - 1));
}

int sr_image_create_intensity(sr_image **out, int n_ch, int nx, int ny, double x_lo, double x_hi, double y_lo, double y_hi) {
  SR_CHECK(out != nullptr, "sr_image_create_intensity: NULL out");
  *out = nullptr;
  SR_CHECK(n_ch >= 1 && n_ch <= SR_MAX_ANALYSERS, "sr_image_create_intensity: %d channels (1..%d)", n_ch, SR_MAX_ANALYSERS);
  SR_CHECK(x_hi > x_lo && y_hi > y_lo, "sr_image_create_intensity: empty range");
  SR_CHECK(nx >= 1 && ny >= 1, "sr_image_create_intensity: bins must be positive");
  return image_alloc(out, SR_IMG_INTENSITY, n_ch, nx, ny, x_lo, x_hi, y_lo, y_hi, (int64_t)sizeof(double) * n_ch * nx * ny);
}

int sr_image_zero(sr_image *img) {
  SR_CHECK(img != nullptr, "sr_image_zero: NULL image");
  SR_HIP(hipMemsetAsync(img->d, 0, (size_t)img->bytes, sr::ctx().stream));
  return SR_OK;
}

int sr_image_download(const sr_image *img, void *host) {
  SR_CHECK(img && host, "sr_image_download: NULL argument");
  SR_HIP(hipMemcpyAsync(host, img->d, (size_t)img->bytes, hipMemcpyDeviceToHost, sr::ctx().stream));
  SR_HIP(hipStreamSynchronize(sr::ctx().stream));
  return SR_OK;
}

int sr_image_amplitude(const sr_image *img, double *H) {
  SR_CHECK(img && H, "sr_image_amplitude: NULL argument");
  SR_CHECK(img->kind == SR_IMG_COMPLEX, "sr_image_amplitude: image does not hold a complex field");
  const int64_t plane = (int64_t)(img->nx - 1) * (img->ny - 1);
  return read_out(H, plane, [&](double *dH, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(k_amplitude, grid, dim3(256), 0, st, (const double *)img->d, plane, dH);
  });
}

int64_t sr_image_bytes(const sr_image *img) { return img ? img->bytes : 0; }

int sr_image_counts_f64(const sr_image *img, double *H) {
  SR_CHECK(img && H, "sr_image_counts_f64: NULL argument");
  SR_CHECK(img->kind == SR_IMG_COUNTS, "sr_image_counts_f64: image does not hold counts");
  const int64_t n = (int64_t)img->nx * img->ny;
  return read_out(H, n, [&](double *dH, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(k_counts_f64, grid, dim3(256), 0, st, (const uint32_t *)img->d, n, dH);
  });
}

int sr_rays_optics(const sr_rays *r, const sr_optic *chain, int n_ops, const sr_deposit_params *p, double *rf_out, double *E_out) {
  SR_CHECK(r && rf_out, "sr_rays_optics: NULL argument");
  if (!r->traced) return sr::fail(SR_ERR_STATE, "sr_rays_optics: rays have not been traced");
  Chain C;
  int rc = make_chain(chain, n_ops, p ? p->kwave : 0.0, C);
  if (rc) return rc;
  RefSet R;
  if ((rc = make_refs(p, R))) return rc;
  const int64_t N = r->n;
  if (N == 0) return SR_OK;
  hipStream_t st = sr::ctx().stream;
  double *dr = static_cast<double *>(sr::scratch(sizeof(double) * (E_out ? 8 : 4) * (size_t)N));
  if (!dr) return SR_ERR_HIP;
  double *dE = E_out ? dr + 4 * (size_t)N : nullptr;
  sr::with_flags(
      [&](auto with_e) {
        hipLaunchKernelGGL((k_rays_optics<with_e.value>), dim3(sr::grid_for(N, 256)), dim3(256), 0, st, C, R, N, (const double *)r->rf,
                           with_e.value ? (const double *)r->Jf : nullptr, (const uint32_t *)r->perm, dr, dE);
      },
      E_out != nullptr);
  rc = sr::stage_out(st, {{rf_out, dr, sizeof(double) * 4 * N}, {E_out, dE, sizeof(double) * 4 * N}});
  if (rc) return rc;
  sr::scratch_trim();
  return SR_OK;
}

int sr_rays_refine(const sr_rays *r, int n_diag, const sr_optic *const *chains, const int *n_ops, sr_image *const *imgs,
                   int64_t *retraced) {
  SR_CHECK(r != nullptr && n_diag >= 0 && n_diag <= SR_MAX_REFINE, "sr_rays_refine: bad argument (at most %d diagnostics)", SR_MAX_REFINE);
  if (!r->traced) return sr::fail(SR_ERR_STATE, "sr_rays_refine: rays have not been traced");
  if (retraced) *retraced = 0;
  if (!r->guard_live || r->n == 0 || n_diag == 0) return SR_OK;  // float64 results already: nothing to refine
  GuardSet S;
  S.n = 0;
  for (int q = 0; q < n_diag; ++q) {
    SR_CHECK(chains && n_ops && imgs && imgs[q], "sr_rays_refine: NULL diagnostic %d", q);
    if (imgs[q]->kind != SR_IMG_COUNTS) continue;  // complex images are not counts: no guard (engine.resolve_precision)
    int rc = make_chain(chains[q], n_ops[q], 0.0, S.C[S.n]);
    if (rc) return rc;
    S.ex[S.n] = make_edges(imgs[q]->x_lo, imgs[q]->x_hi, imgs[q]->nx);
    S.ey[S.n] = make_edges(imgs[q]->y_lo, imgs[q]->y_hi, imgs[q]->ny);
    ++S.n;
  }
  if (S.n == 0) return SR_OK;
  hipStream_t st = sr::ctx().stream;
  const int64_t N = r->n;
  // the set travels through a buffer that belongs to the bundle (device side) and a copy the bundle keeps (host side): no wait
  // is needed for either, so a chunked driver can queue refine + deposits without a host round trip (retraced == NULL)
  sr_rays *rw = const_cast<sr_rays *>(r);
  if (!rw->guard_set) SR_HIP(sr::dev_alloc_bytes(&rw->guard_set, sizeof(GuardSet)));
  rw->guard_set_host.assign(reinterpret_cast<const char *>(&S), reinterpret_cast<const char *>(&S) + sizeof(GuardSet));
  SR_HIP(hipMemcpyAsync(rw->guard_set, rw->guard_set_host.data(), sizeof(GuardSet), hipMemcpyHostToDevice, st));
  int rc = guard_queue_reset(r, st);
  if (rc) return rc;
  const Guard G = guard_of(r);
  hipLaunchKernelGGL(k_guard_flags, dim3(sr::grid_for(N, 256)), dim3(256), 0, st, (const GuardSet *)rw->guard_set, N, (const double *)r->rf, G);
  SR_HIP(hipGetLastError());
  if ((rc = sr::retrace_f64(r, G.list, G.count))) return rc;
  if (retraced) {
    unsigned long long n_again = 0;
    SR_HIP(hipMemcpyAsync(&n_again, G.count, sizeof n_again, hipMemcpyDeviceToHost, st));
    SR_HIP(hipStreamSynchronize(st));
    *retraced = (int64_t)n_again;
  }
  return SR_OK;
}

int sr_rays_deposit(const sr_rays *r, const sr_optic *chain, int n_ops, const sr_deposit_params *p, sr_image *img,
                    sr_deposit_stats *stats) {
  SR_CHECK(r && img, "sr_rays_deposit: NULL argument");
  if (!r->traced) return sr::fail(SR_ERR_STATE, "sr_rays_deposit: rays have not been traced");
  SR_CHECK(img->kind != SR_IMG_INTENSITY, "sr_rays_deposit: an intensity image is filled by sr_rays_deposit_intensity");
  Chain C;
  int rc = make_chain(chain, n_ops, p ? p->kwave : 0.0, C);
  if (rc) return rc;
  RefSet R;
  if ((rc = make_refs(p, R))) return rc;
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;
  const int64_t N = r->n;
  if ((rc = deposit_begin(r, stats)) || N == 0) return rc;
  const unsigned grid = sr::grid_for(N, 256);
  const bool tiled = p ? p->lds_tiles != 0 : true;
  const bool cplx = img->kind == SR_IMG_COMPLEX;
  const Edges ex = make_edges(img->x_lo, img->x_hi, cplx ? img->nx - 1 : img->nx);
  const Edges ey = make_edges(img->y_lo, img->y_hi, cplx ? img->ny - 1 : img->ny);
  const double *rf = r->rf, *Jf = r->Jf;
  // exact counts (the default): rays of a mixed-precision trace whose pixel or mask decision is not certain are traced
  // again in float64 and counted afterwards -- the image is the float64 build's, integer for integer
  const bool exact = !cplx && (p ? p->exact_counts != 0 : true) && r->guard_live;
  const Guard G = guard_of(r);
  if (exact && (rc = guard_queue_reset(r, st))) return rc;
  sr::with_flags(
      [&](auto is_cplx, auto is_tiled, auto guarded) {
        constexpr int KIND = is_cplx.value ? SR_IMG_COMPLEX : SR_IMG_COUNTS;
        if constexpr (!(is_cplx.value && guarded.value))  // the guard is the counts image's
          hipLaunchKernelGGL((k_deposit<KIND, is_tiled.value, guarded.value>), dim3(grid), dim3(256), 0, st, C, R, N, rf, Jf, ex, ey,
                             static_cast<typename ImagePatch<KIND>::Cell *>(img->d), r->counters, G);
      },
      cplx, tiled, exact);
  if (exact) {
    SR_HIP(hipGetLastError());
    if ((rc = sr::retrace_f64(r, G.list, G.count))) return rc;
    const unsigned lgrid = sr::capped_grid(grid, 8);
    hipLaunchKernelGGL(k_deposit_list, dim3(lgrid), dim3(256), 0, st, C, N, rf, ex, ey, (uint32_t *)img->d, r->counters,
                       (const uint32_t *)G.list, (const unsigned long long *)G.count);
  }
  return deposit_finish(r, stats, exact);
}

// ---- polarimetry (no reference counterpart) ----------------------------------------------
int sr_intensity2d(const double *x, const double *y, const double *E, int64_t N, const double *analyser_ab, int n_ch, int nxb,
                   int nyb, double x_lo, double x_hi, double y_lo, double y_hi, double *I) {
  SR_CHECK(N >= 0 && (N == 0 || (x && y && E)) && I, "sr_intensity2d: bad argument");
  SR_CHECK(nxb >= 1 && nyb >= 1, "sr_intensity2d: bins must be positive");
  SR_CHECK(x_hi > x_lo && y_hi > y_lo, "sr_intensity2d: empty range");
  Analysers A;
  int rc = make_analysers(analyser_ab, n_ch, A);
  if (rc) return rc;
  if ((rc = sr::ensure_init())) return rc;
  hipStream_t st = sr::ctx().stream;
  sr::CallBuffers buf;
  double *dx = nullptr, *dy = nullptr, *dE = nullptr, *dI = nullptr;
  const size_t cells = (size_t)n_ch * nxb * nyb;
  SR_RC(buf.zeroed(&dI, cells, st));
  if (N > 0) {
    SR_RC(buf.upload(&dx, x, (size_t)N, st));
    SR_RC(buf.upload(&dy, y, (size_t)N, st));
    SR_RC(buf.upload(&dE, E, 4 * (size_t)N, st));
    const Edges ex = make_edges(x_lo, x_hi, nxb), ey = make_edges(y_lo, y_hi, nyb);
    sr::with_count<SR_MAX_ANALYSERS>(
        [&](auto nch) {
          hipLaunchKernelGGL((k_intensity2d<nch.value>), dim3(sr::grid_for(N, 256)), dim3(256), 0, st, (const double *)dx,
                             (const double *)dy, (const double *)dE, N, ex, ey, A, dI);
        },
        n_ch);
  }
  return sr::stage_out(st, {{I, dI, sizeof(double) * cells}});
}

int sr_rays_deposit_intensity(const sr_rays *r, const sr_optic *chain, int n_ops, const double *analyser_ab, int n_ch,
                              int lds_tiles, sr_image *img, sr_deposit_stats *stats) {
  SR_CHECK(r && img, "sr_rays_deposit_intensity: NULL argument");
  if (!r->traced) return sr::fail(SR_ERR_STATE, "sr_rays_deposit_intensity: rays have not been traced");
  if (!r->Jf) return sr::fail(SR_ERR_STATE, "sr_rays_deposit_intensity: the bundle was traced without the Jones vector Jf");
  SR_CHECK(img->kind == SR_IMG_INTENSITY, "sr_rays_deposit_intensity: image does not hold intensities");
  SR_CHECK(n_ch == img->n_ch, "sr_rays_deposit_intensity: %d analysers for an image of %d channels", n_ch, img->n_ch);
  Chain C;
  int rc = make_chain(chain, n_ops, 0.0, C);
  if (rc) return rc;
  Analysers A;
  if ((rc = make_analysers(analyser_ab, n_ch, A))) return rc;
  hipStream_t st = sr::ctx().stream;
  const int64_t N = r->n;
  if ((rc = deposit_begin(r, stats)) || N == 0) return rc;
  const Edges ex = make_edges(img->x_lo, img->x_hi, img->nx), ey = make_edges(img->y_lo, img->y_hi, img->ny);
  sr::with_count<SR_MAX_ANALYSERS>(
      [&](auto nch) {
        sr::with_flags(
            [&](auto is_tiled) {
              hipLaunchKernelGGL((k_deposit_intensity<nch.value, is_tiled.value>), dim3(sr::grid_for(N, 256)), dim3(256), 0, st, C, N,
                                 (const double *)r->rf, (const double *)r->Jf, ex, ey, A, (double *)img->d, r->counters);
            },
            lds_tiles != 0);
      },
      n_ch);
  return deposit_finish(r, stats, false);
}

int sr_image_rotation(const sr_image *img, int ch_plus, int ch_minus, double beta, double *alpha) {
  SR_CHECK(img && alpha, "sr_image_rotation: NULL argument");
  SR_CHECK(img->kind == SR_IMG_INTENSITY, "sr_image_rotation: image does not hold intensities");
  SR_CHECK(ch_plus >= 0 && ch_plus < img->n_ch && ch_minus >= 0 && ch_minus < img->n_ch && ch_plus != ch_minus,
           "sr_image_rotation: channels %d, %d of an image of %d", ch_plus, ch_minus, img->n_ch);
  SR_CHECK(beta > 0 && beta < M_PI / 2, "sr_image_rotation: beta must lie in (0, pi/2)");
  const int64_t plane = (int64_t)img->nx * img->ny;
  const double *I = (const double *)img->d;
  return read_out(alpha, plane, [&](double *dA, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(k_rotation, grid, dim3(256), 0, st, I + ch_plus * plane, I + ch_minus * plane, plane, sin(2 * beta), cos(2 * beta), dA);
  });
}

}  // extern "C"
