// After the path: Fresnel propagation of the traced field (src/simulator/fresnel_integral.py), the reference's one route to
// wave optics.  Two stages:
//   scatter to grid (propagate's two LinearNDInterpolators, fresnel_integral.py:69-78): every node of the
//     meshgrid(x, y) grid gets the rays' amplitude and phase interpolated linearly in the Delaunay triangle of ALL rays
//     that holds it, 0 outside their convex hull -- scipy's LinearNDInterpolator(..., fill_value=0), without building
//     the triangulation;
//   propagation (fresnel_propagate, :25-59): reflect-pad + Tukey window (fused with U0 = amp e^{-i phase} when the field
//     comes from the grid), forward 2-D Z2Z FFT, transfer function (and LANEX PSF), inverse FFT, phase factor, centre crop.
// float64 / complex128 throughout, as the reference computes.
//
// Scatter to grid.  The rays are counting-sorted into a uniform grid of bins over their bounding box (~3 rays per bin).
// The hull: the extreme ray in each of 64 directions (one lane per direction), every ray strictly inside the polygon of
// those rays dropped (ballot compaction), the exact hull of the few left by a monotone chain on the host.  Then one
// work-item per node inside the hull:
//   candidates C = the rays in a window of bins around the node (grown as needed);
//   walk in DT(C), the Delaunay triangulation of C: a = the candidate nearest the node, b = the one nearest a (a
//     nearest-neighbour pair is a Delaunay edge).  For an edge (u, v) with the node on its left, the Delaunay triangle on
//     that side is (u, v, c) with c the left candidate whose circle through u, v is smallest on that side: one scan of C
//     with in-circle comparisons.  If (u, v, c) holds the node the walk stops, else it crosses the edge the node lies
//     beyond (a visibility walk, which terminates in a Delaunay triangulation).  No candidate on the left: the node is
//     outside conv(C), and C grows;
//   verify: the triangle is Delaunay in C, so its circumcircle holds no candidate.  If the window covers every bin the
//     circle overlaps, the circle holds no ray at all and the triangle is THE Delaunay triangle of all rays that holds the
//     node.  If not, the window takes in the circle's bins (the rays that may lie in it become candidates) and the node is
//     walked again.
// A node over the first pass's budget (rays in its window, steps of a walk) is queued (ballot, one atomic per wavefront)
// for a second kernel that repeats the same search with a workgroup per node (cooperative scans, no budget): thin
// triangles along the hull have circles that reach across the whole beam.  Orientation and in-circle are float64 in
// coordinates relative to the node, every product rounded (-ffp-contract=off).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "fft.hpp"

namespace {

constexpr int kDirs = 64;               // directions of the hull pre-filter: one lane of a wavefront each
constexpr int kTeam = 256;              // work-items per node in the second pass
constexpr int64_t kBudgetRays = 2048;   // first pass: rays in a node's window
constexpr int kBudgetSteps = 64;        // first pass: steps of one walk
constexpr int kTeamSteps = 1 << 20;     // second pass: steps of one walk (a bound, never reached by a Delaunay walk)
constexpr double kRaysPerBin = 3.0;

// ---- bounding box ---------------------------------------------------------------------------------------------------
// doubles as unsigned integers of the same order (atomicMin / atomicMax)
__device__ __forceinline__ unsigned long long order_key(double d) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
double from_order_key(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double d;
  std::memcpy(&d, &u, sizeof d);
  return d;
}

// bb: keys of min x, min y (atomicMin), max x, max y (atomicMax)
__global__ void k_bbox(const double *__restrict__ x, const double *__restrict__ y, int64_t n, unsigned long long *__restrict__ bb) {
  double lx = INFINITY, ly = INFINITY, hx = -INFINITY, hy = -INFINITY;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    lx = fmin(lx, x[i]);
    ly = fmin(ly, y[i]);
    hx = fmax(hx, x[i]);
    hy = fmax(hy, y[i]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    lx = fmin(lx, __shfl_down(lx, off, 64));
    ly = fmin(ly, __shfl_down(ly, off, 64));
    hx = fmax(hx, __shfl_down(hx, off, 64));
    hy = fmax(hy, __shfl_down(hy, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&bb[0], order_key(lx));
    atomicMin(&bb[1], order_key(ly));
    atomicMax(&bb[2], order_key(hx));
    atomicMax(&bb[3], order_key(hy));
  }
}

// ---- binning ----------------------------------------------------------------------------------------------------------
struct BinGrid {
  int nbx, nby;
  double x0, y0, ibx, iby;  // lower corner of the rays' box, bins per unit length
};

__device__ __forceinline__ int bin_of(double v, double v0, double inv, int n) {
  const double t = floor((v - v0) * inv);
  return t < 0.0 ? 0 : (t >= (double)(n - 1) ? n - 1 : (int)t);
}

__global__ void k_bin_count(const double *__restrict__ x, const double *__restrict__ y, int64_t n, BinGrid g,
                            uint32_t *__restrict__ cnt) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&cnt[(int64_t)bin_of(y[i], g.y0, g.iby, g.nby) * g.nbx + bin_of(x[i], g.x0, g.ibx, g.nbx)], 1u);
}

__global__ void k_bin_scatter(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ amp,
                              const double *__restrict__ phase, int64_t n, BinGrid g, uint32_t *__restrict__ cursor,
                              double2 *__restrict__ xy, double2 *__restrict__ val, int *__restrict__ id) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t k = atomicAdd(&cursor[(int64_t)bin_of(y[i], g.y0, g.iby, g.nby) * g.nbx + bin_of(x[i], g.x0, g.ibx, g.nbx)], 1u);
    xy[k] = make_double2(x[i], y[i]);
    val[k] = make_double2(amp[i], phase[i]);
    id[k] = (int)i;
  }
}

// ---- hull pre-filter --------------------------------------------------------------------------------------------------
// Lane k of every wavefront owns direction 2 pi k / 64 and keeps the ray with the largest projection on it (relative to
// (cx, cy)); the wavefront's 64 rays of a step are broadcast one by one.  best[k] = max of (projection rounded to float32,
// ordered) << 32 | ray index: float32 rounding may pick a nearly extreme ray, and any ray will do -- the polygon of the
// picked rays lies inside the hull, which is all the filter needs.
__global__ void k_extremes(const double *__restrict__ x, const double *__restrict__ y, int64_t n, double cx, double cy,
                           unsigned long long *__restrict__ best) {
  const int lane = threadIdx.x & 63;
  double sn, cs;
  sincos(M_PI * (double)lane / 32.0, &sn, &cs);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  double bv = -INFINITY;
  int64_t bi = -1;
  for (int64_t base = wave * 64; base < n; base += n_waves * 64) {
    const int64_t i = base + lane;
    const double rx = i < n ? x[i] - cx : 0.0, ry = i < n ? y[i] - cy : 0.0;
    const int m = (int)(n - base < 64 ? n - base : 64);
    for (int r = 0; r < m; ++r) {
      const double qx = __shfl(rx, r, 64), qy = __shfl(ry, r, 64);
      const double d = cs * qx + sn * qy;
      if (d > bv) {
        bv = d;
        bi = base + r;
      }
    }
  }
  if (bi >= 0) {
    const unsigned u = __float_as_uint((float)bv);
    const unsigned key = (u >> 31) ? ~u : (u | 0x80000000u);
    atomicMax(&best[lane], ((unsigned long long)key << 32) | (unsigned long long)(uint32_t)bi);
  }
}

// The rays NOT strictly inside the convex polygon P (m counter-clockwise vertices, rays themselves) go to list: a ray
// strictly inside it is strictly inside the hull, so no hull vertex.  One ray per work-item (queue_push wants the whole
// wavefront).
__global__ __launch_bounds__(256) void k_hull_filter(const double *__restrict__ x, const double *__restrict__ y, int64_t n,
                                                     const double2 *__restrict__ P, int m, unsigned long long *__restrict__ count,
                                                     uint32_t *__restrict__ list) {
  __shared__ double2 poly[kDirs];
  for (int t = threadIdx.x; t < m; t += blockDim.x) poly[t] = P[t];
  __syncthreads();
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  bool keep = false;
  if (i < n) {
    const double px = x[i], py = y[i];
    bool inside = m >= 3;  // no polygon: every ray goes on
    for (int k = 0; k < m && inside; ++k) {
      const double2 a = poly[k], b = poly[k + 1 == m ? 0 : k + 1];
      inside = (a.x - px) * (b.y - py) - (a.y - py) * (b.x - px) > 0.0;
    }
    keep = !inside;
  }
  sr::queue_push(count, list, keep, (uint32_t)i);
}

// ---- point location -----------------------------------------------------------------------------------------------------
struct Bins {
  BinGrid g;
  const double2 *xy;       // ray positions in bin order
  const double2 *val;      // (amplitude, phase), the same order
  const int *id;           // the ray's index in the caller's arrays
  const uint32_t *start;   // nbx * nby + 1: bin b holds slots start[b] .. start[b + 1]
};

struct Win {
  int x0, x1, y0, y1;  // inclusive bin ranges
};

struct Cand {
  double x, y;  // relative to the node
  double key;   // squared distance (nearest scans)
  int slot;     // position in bin order, -1: none
  int id;       // ray index (ties go to the lower one)
};

// orientation of (a, b, c): > 0 counter-clockwise
__device__ __forceinline__ double orient(double ax, double ay, double bx, double by, double cx, double cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}
// > 0: d lies inside the circle through a, b, c (counter-clockwise)
__device__ __forceinline__ double incircle(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) {
  const double adx = ax - dx, ady = ay - dy, bdx = bx - dx, bdy = by - dy, cdx = cx - dx, cdy = cy - dy;
  const double a2 = adx * adx + ady * ady, b2 = bdx * bdx + bdy * bdy, c2 = cdx * cdx + cdy * cdy;
  return a2 * (bdx * cdy - cdx * bdy) + b2 * (cdx * ady - adx * cdy) + c2 * (adx * bdy - bdx * ady);
}

// NT work-items search one node together (1: the first pass; kTeam: a workgroup in the second); lds: NT entries.
template <int NT>
struct Team {
  Cand *lds;
  __device__ int tid() const { return NT == 1 ? 0 : (int)threadIdx.x; }
  // the best of the work-items' candidates by `better`, returned to all
  template <class Better>
  __device__ Cand best(const Cand &c, Better better) const {
    if (NT == 1) return c;
    const int t = threadIdx.x;
    lds[t] = c;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
      if (t < off && better(lds[t + off], lds[t])) lds[t] = lds[t + off];
      __syncthreads();
    }
    const Cand r = lds[0];
    __syncthreads();
    return r;
  }
};

// f(slot) for every ray in the window; a row of the window is one contiguous run of slots
template <int NT, class F>
__device__ void for_window(const Bins &B, const Win &w, const Team<NT> &tm, F f) {
  for (int by = w.y0; by <= w.y1; ++by) {
    const int64_t row = (int64_t)by * B.g.nbx;
    const uint32_t e = B.start[row + w.x1 + 1];
    for (uint32_t k = B.start[row + w.x0] + (uint32_t)tm.tid(); k < e; k += NT) f((int)k);
  }
}

__device__ int64_t window_rays(const Bins &B, const Win &w) {
  int64_t n = 0;
  for (int by = w.y0; by <= w.y1; ++by) {
    const int64_t row = (int64_t)by * B.g.nbx;
    n += (int64_t)B.start[row + w.x1 + 1] - (int64_t)B.start[row + w.x0];
  }
  return n;
}

// the window ray nearest (qx, qy); with skip >= 0, neither ray `skip` nor a ray at its position
template <int NT>
__device__ Cand nearest(const Bins &B, const Win &w, const Team<NT> &tm, double px, double py, double qx, double qy, int skip) {
  Cand c{0.0, 0.0, INFINITY, -1, INT_MAX};
  for_window(B, w, tm, [&](int k) {
    const double2 r = B.xy[k];
    const double x = r.x - px, y = r.y - py, dx = x - qx, dy = y - qy;
    const double d = dx * dx + dy * dy;
    if (skip >= 0 && (k == skip || d == 0.0)) return;
    const int id = B.id[k];
    if (d < c.key || (d == c.key && id < c.id)) c = Cand{x, y, d, k, id};
  });
  return tm.best(c, [](const Cand &a, const Cand &b) {
    return a.slot >= 0 && (b.slot < 0 || a.key < b.key || (a.key == b.key && a.id < b.id));
  });
}

// the Delaunay mate of edge (u, v) in the window's rays: among the rays left of u -> v, the one whose circle through u, v
// holds no other (in-circle order; a tie, co-circular rays, goes to the lower index); slot -1: no ray on that side
template <int NT>
__device__ Cand mate(const Bins &B, const Win &w, const Team<NT> &tm, double px, double py, const Cand &u, const Cand &v) {
  Cand c{0.0, 0.0, 0.0, -1, INT_MAX};
  for_window(B, w, tm, [&](int k) {
    const double2 r = B.xy[k];
    const double x = r.x - px, y = r.y - py;
    if (!(orient(u.x, u.y, v.x, v.y, x, y) > 0.0)) return;
    const int id = B.id[k];
    if (c.slot >= 0) {
      const double ic = incircle(u.x, u.y, v.x, v.y, c.x, c.y, x, y);
      if (!(ic > 0.0 || (ic == 0.0 && id < c.id))) return;
    }
    c = Cand{x, y, 0.0, k, id};
  });
  return tm.best(c, [&](const Cand &a, const Cand &b) {
    if (a.slot < 0) return false;
    if (b.slot < 0) return true;
    const double ic = incircle(u.x, u.y, v.x, v.y, b.x, b.y, a.x, a.y);
    return ic > 0.0 || (ic == 0.0 && a.id < b.id);
  });
}

// the bins the circumcircle of (a, b, c) overlaps (a margin of 1e-9 of its radius); all bins if it has none
__device__ Win circle_bins(const Bins &B, double px, double py, const Cand &a, const Cand &b, const Cand &c) {
  const double bx = b.x - a.x, by = b.y - a.y, cx = c.x - a.x, cy = c.y - a.y;
  const double d = 2.0 * (bx * cy - by * cx);
  const double b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
  const double ux = (cy * b2 - by * c2) / d, uy = (bx * c2 - cx * b2) / d;  // centre relative to a
  const double r = sqrt(ux * ux + uy * uy) * (1.0 + 1e-9) + 1e-9 / fmax(B.g.ibx, B.g.iby);
  const double ox = (px + a.x) + ux, oy = (py + a.y) + uy;
  if (!(fabs(ox) + fabs(oy) + r < INFINITY)) return Win{0, B.g.nbx - 1, 0, B.g.nby - 1};
  return Win{bin_of(ox - r, B.g.x0, B.g.ibx, B.g.nbx), bin_of(ox + r, B.g.x0, B.g.ibx, B.g.nbx),
             bin_of(oy - r, B.g.y0, B.g.iby, B.g.nby), bin_of(oy + r, B.g.y0, B.g.iby, B.g.nby)};
}

// The Delaunay triangle of all rays that holds node (px, py).  1: found, slots in t; 0: no ray triangle holds the node
// (outside the hull); -1: over the budget (rays in the window or steps of a walk).
template <int NT>
__device__ int locate(const Bins &B, const Team<NT> &tm, double px, double py, int64_t budget, int max_steps, int t[3]) {
  const int cx = bin_of(px, B.g.x0, B.g.ibx, B.g.nbx), cy = bin_of(py, B.g.y0, B.g.iby, B.g.nby);
  Win w{cx, cx, cy, cy};
  for (;;) {
    if (budget < INT64_MAX && window_rays(B, w) > budget) return -1;
    bool grow = false;
    Cand u = nearest(B, w, tm, px, py, 0.0, 0.0, -1), v{}, c{};
    if (u.slot < 0) {
      grow = true;
    } else {
      v = nearest(B, w, tm, px, py, u.x, u.y, u.slot);
      grow = v.slot < 0;
    }
    if (!grow) {
      const double o0 = orient(u.x, u.y, v.x, v.y, 0.0, 0.0);
      if (o0 < 0.0) {
        const Cand s = u;
        u = v;
        v = s;
      }
      for (int step = 0;; ++step) {
        if (step == max_steps) return -1;
        c = mate(B, w, tm, px, py, u, v);
        // The node on the line of the starting pair (on a ray, on an edge, on the hull's boundary): its triangle may lie
        // on either side.  No ray on this one (the pair runs clockwise along the hull): the other one.
        if (c.slot < 0 && step == 0 && o0 == 0.0) {
          const Cand s = u;
          u = v;
          v = s;
          c = mate(B, w, tm, px, py, u, v);
        }
        if (c.slot < 0) {  // (u, v) is a hull edge of the candidates and the node lies beyond it
          grow = true;
          break;
        }
        const double o1 = orient(v.x, v.y, c.x, c.y, 0.0, 0.0), o2 = orient(c.x, c.y, u.x, u.y, 0.0, 0.0);
        if (o1 >= 0.0 && o2 >= 0.0) break;
        if (o1 < 0.0)
          u = c;  // beyond edge (v, c): walk on over (c, v)
        else
          v = c;  // beyond edge (c, u): walk on over (u, c)
      }
    }
    if (grow) {
      if (w.x0 == 0 && w.y0 == 0 && w.x1 == B.g.nbx - 1 && w.y1 == B.g.nby - 1) return 0;
      const int gx = max(1, (w.x1 - w.x0 + 1) / 2), gy = max(1, (w.y1 - w.y0 + 1) / 2);
      w = Win{max(0, w.x0 - gx), min(B.g.nbx - 1, w.x1 + gx), max(0, w.y0 - gy), min(B.g.nby - 1, w.y1 + gy)};
      continue;
    }
    const Win cw = circle_bins(B, px, py, u, v, c);
    if (cw.x0 >= w.x0 && cw.x1 <= w.x1 && cw.y0 >= w.y0 && cw.y1 <= w.y1) {
      t[0] = u.slot;
      t[1] = v.slot;
      t[2] = c.slot;
      return 1;
    }
    w = Win{min(w.x0, cw.x0), max(w.x1, cw.x1), min(w.y0, cw.y0), max(w.y1, cw.y1)};
  }
}

// node strictly inside or on the hull H (h counter-clockwise vertices): wedge from H[0] by binary search
__device__ bool in_hull(const double2 *__restrict__ H, int h, double px, double py) {
  if (h < 3) return false;
  const double ox = H[0].x - px, oy = H[0].y - py;
  auto side = [&](int i) { return ox * (H[i].y - py) - oy * (H[i].x - px); };  // orient(H0, Hi, node)
  if (!(side(1) >= 0.0) || !(side(h - 1) <= 0.0)) return false;
  int lo = 1, hi = h - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (side(mid) >= 0.0)
      lo = mid;
    else
      hi = mid;
  }
  return (H[lo].x - px) * (H[lo + 1].y - py) - (H[lo].y - py) * (H[lo + 1].x - px) >= 0.0;
}

// amplitude and phase of node q from its triangle (vertices in ascending ray index, barycentric weights), or 0 / -1
__device__ void store_node(const Bins &B, int64_t q, double px, double py, bool found, const int t[3], double *__restrict__ amp,
                           double *__restrict__ phase, int *__restrict__ tri) {
  if (!found) {
    amp[q] = 0.0;
    phase[q] = 0.0;
    if (tri) tri[3 * q] = tri[3 * q + 1] = tri[3 * q + 2] = -1;
    return;
  }
  int s[3] = {t[0], t[1], t[2]}, id[3] = {B.id[t[0]], B.id[t[1]], B.id[t[2]]};
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (id[j] > id[j + 1]) {
        const int a = id[j], b = s[j];
        id[j] = id[j + 1];
        s[j] = s[j + 1];
        id[j + 1] = a;
        s[j + 1] = b;
      }
  const double2 A = B.xy[s[0]], Bv = B.xy[s[1]], Cv = B.xy[s[2]];
  const double ax = A.x - px, ay = A.y - py, bx = Bv.x - px, by = Bv.y - py, cx = Cv.x - px, cy = Cv.y - py;
  const double la = bx * cy - by * cx, lb = cx * ay - cy * ax, lc = ax * by - ay * bx;
  const double area = (la + lb) + lc;
  const double wa = la / area, wb = lb / area, wc = lc / area;
  const double2 va = B.val[s[0]], vb = B.val[s[1]], vc = B.val[s[2]];
  amp[q] = (wa * va.x + wb * vb.x) + wc * vc.x;
  phase[q] = (wa * va.y + wb * vb.y) + wc * vc.y;
  if (tri) {
    tri[3 * q] = id[0];
    tri[3 * q + 1] = id[1];
    tri[3 * q + 2] = id[2];
  }
}

// first pass: one work-item per node; cnt[0]: nodes queued for the second pass (list), cnt[1]: nodes outside the hull
__global__ __launch_bounds__(256) void k_locate(Bins B, const double2 *__restrict__ hull, int nh, const double *__restrict__ gx,
                                                int nx, const double *__restrict__ gy, int64_t n_nodes, double *__restrict__ amp,
                                                double *__restrict__ phase, int *__restrict__ tri,
                                                unsigned long long *__restrict__ cnt, uint32_t *__restrict__ list) {
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  bool defer = false, outside = false;
  if (q < n_nodes) {
    const double px = gx[q % nx], py = gy[q / nx];
    int t[3] = {-1, -1, -1};
    int r = 0;
    if (in_hull(hull, nh, px, py)) r = locate(B, Team<1>{nullptr}, px, py, kBudgetRays, kBudgetSteps, t);
    defer = r < 0;
    outside = r == 0;
    if (!defer) store_node(B, q, px, py, r > 0, t, amp, phase, tri);
  }
  const unsigned long long m = __ballot(outside);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[1], (unsigned long long)__popcll(m));
  sr::queue_push(&cnt[0], list, defer, (uint32_t)q);
}

// second pass: a workgroup per queued node, no budget; cnt[2]: nodes it could not resolve (none in a Delaunay walk)
__global__ __launch_bounds__(kTeam) void k_locate_team(Bins B, const uint32_t *__restrict__ list, int64_t n_list,
                                                       const double *__restrict__ gx, int nx, const double *__restrict__ gy,
                                                       double *__restrict__ amp, double *__restrict__ phase, int *__restrict__ tri,
                                                       unsigned long long *__restrict__ cnt) {
  __shared__ Cand lds[kTeam];
  const Team<kTeam> tm{lds};
  for (int64_t w = blockIdx.x; w < n_list; w += gridDim.x) {
    const int64_t q = list[w];
    const double px = gx[q % nx], py = gy[q / nx];
    int t[3] = {-1, -1, -1};
    const int r = locate(B, tm, px, py, INT64_MAX, kTeamSteps, t);
    if (threadIdx.x == 0) {
      if (r < 0) atomicAdd(&cnt[2], 1ull);
      if (r == 0) atomicAdd(&cnt[1], 1ull);
      store_node(B, q, px, py, r > 0, t, amp, phase, tri);
    }
  }
}

// ---- propagation ---------------------------------------------------------------------------------------------------------
// prepare_field_for_propagation on the gridded field: U[r][c] = U0[src0[r]][src1[c]] * (w0[r] * w1[c]) with
// U0 = amp * exp(-i phase) = (amp cos(phase), amp (-sin(phase))), as numpy forms it
__global__ void k_pad_window(const double *__restrict__ amp, const double *__restrict__ phase, int n1, const int *__restrict__ src0,
                             const int *__restrict__ src1, const double *__restrict__ w0, const double *__restrict__ w1, int m0,
                             int m1, double2 *__restrict__ out) {
  const int64_t n = (int64_t)m0 * m1;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = q / m1, c = q - r * m1;
    const int64_t s = (int64_t)src0[r] * n1 + src1[c];
    const double a = amp[s];
    double sn, cs;
    sincos(phase[s], &sn, &cs);
    const double w = w0[r] * w1[c];
    out[q] = make_double2((a * cs) * w, (a * -sn) * w);
  }
}

// the transfer function H = exp(-i pi_lz S) and, with psf > 0, the PSF exp(-psf S), S = fx^2 + fy^2
__global__ void k_transfer(double2 *__restrict__ F, int m0, int m1, const double *__restrict__ fx, const double *__restrict__ fy,
                           double pi_lz, double psf) {
  const int64_t n = (int64_t)m0 * m1;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = q / m1, c = q - r * m1;
    const double S = fx[r] * fx[r] + fy[c] * fy[c];
    double sn, cs;
    sincos(pi_lz * S, &sn, &cs);
    const double hr = cs, hi = -sn;
    const double2 v = F[q];
    double2 o = make_double2(v.x * hr - v.y * hi, v.x * hi + v.y * hr);
    if (psf > 0.0) {
      const double g = exp(-(psf * S));
      o.x *= g;
      o.y *= g;
    }
    F[q] = o;
  }
}

// the centre crop times the phase factor (and numpy's 1/(m0 m1), folded into post)
__global__ void k_crop(const double2 *__restrict__ F, int m1, int r0, int nr, int c0, int nc, double post_re, double post_im,
                       double2 *__restrict__ out) {
  const int64_t n = (int64_t)nr * nc;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = q / nc, c = q - r * nc;
    const double2 v = F[(r0 + r) * (int64_t)m1 + c0 + c];
    out[q] = make_double2(v.x * post_re - v.y * post_im, v.x * post_im + v.y * post_re);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
unsigned grid_of(int64_t n, int block, int per_cu) {
  return sr::capped_grid((n + block - 1) / block, per_cu);
}

// Andrew's monotone chain over the rays idx: the strict convex hull (collinear and repeated points dropped),
// counter-clockwise from the lowest-x point
std::vector<uint32_t> monotone_chain(const double *x, const double *y, std::vector<uint32_t> idx) {
  std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return x[a] < x[b] || (x[a] == x[b] && y[a] < y[b]); });
  const int64_t n = (int64_t)idx.size();
  if (n < 3) return idx;
  auto cross = [&](uint32_t o, uint32_t a, uint32_t b) { return (x[a] - x[o]) * (y[b] - y[o]) - (y[a] - y[o]) * (x[b] - x[o]); };
  std::vector<uint32_t> h((size_t)(2 * n));
  int64_t k = 0;
  for (int64_t i = 0; i < n; ++i) {
    while (k >= 2 && cross(h[k - 2], h[k - 1], idx[i]) <= 0.0) --k;
    h[k++] = idx[i];
  }
  for (int64_t i = n - 2, lower = k + 1; i >= 0; --i) {
    while (k >= lower && cross(h[k - 2], h[k - 1], idx[i]) <= 0.0) --k;
    h[k++] = idx[i];
  }
  h.resize((size_t)(k - 1));
  return h;
}

// Scatter to grid: d_amp, d_phase (ny x nx) and, with want_tri, d_tri (ny x nx x 3) on the device; stats as the header says.
int scatter_to_grid(const char *who, int64_t n, const double *rx, const double *ry, const double *ra, const double *rp, int nx,
                    const double *gx, int ny, const double *gy, bool want_tri, sr::CallBuffers &buf, double **d_amp, double **d_phase,
                    int **d_tri, int64_t *stats) {
  hipStream_t st = sr::ctx().stream;
  const int64_t n_nodes = (int64_t)nx * ny;
  double *d_in = nullptr, *d_g = nullptr;
  unsigned long long *d_w = nullptr;  // [0..3] box, [4..67] extremes, [68..71] counters
  SR_RC(buf.alloc(&d_in, (size_t)(4 * n)));
  SR_RC(buf.alloc(&d_g, (size_t)(nx + ny)));
  SR_RC(buf.alloc(&d_w, 4 + kDirs + 4));
  SR_RC(buf.alloc(d_amp, (size_t)n_nodes));
  SR_RC(buf.alloc(d_phase, (size_t)n_nodes));
  if (want_tri) SR_RC(buf.alloc(d_tri, (size_t)(3 * n_nodes)));
  const double *x = d_in, *y = d_in + n, *a = d_in + 2 * n, *p = d_in + 3 * n;
  SR_RC(sr::upload_sync(d_in, rx, sizeof(double) * n, st));
  SR_RC(sr::upload_sync(d_in + n, ry, sizeof(double) * n, st));
  SR_RC(sr::upload_sync(d_in + 2 * n, ra, sizeof(double) * n, st));
  SR_RC(sr::upload_sync(d_in + 3 * n, rp, sizeof(double) * n, st));
  SR_HIP(hipMemcpyAsync(d_g, gx, sizeof(double) * nx, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(d_g + nx, gy, sizeof(double) * ny, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemsetAsync(d_w, 0xff, 2 * sizeof(unsigned long long), st));
  SR_HIP(hipMemsetAsync(d_w + 2, 0, (2 + kDirs + 4) * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_bbox, dim3(grid_of(n, 256, 8)), dim3(256), 0, st, x, y, n, d_w);
  hipLaunchKernelGGL(k_extremes, dim3(grid_of(n, 256, 8)), dim3(256), 0, st, x, y, n, rx[0], ry[0], d_w + 4);
  SR_HIP(hipGetLastError());
  unsigned long long hw[4 + kDirs];
  SR_HIP(hipMemcpyAsync(hw, d_w, sizeof hw, hipMemcpyDeviceToHost, st));
  SR_HIP(hipStreamSynchronize(st));

  // bins: ~kRaysPerBin rays each over the rays' box, square-ish
  const double bx0 = from_order_key(hw[0]), by0 = from_order_key(hw[1]);
  const double wx = from_order_key(hw[2]) - bx0, wy = from_order_key(hw[3]) - by0;
  const double target = std::max(1.0, (double)n / kRaysPerBin);
  BinGrid g{1, 1, bx0, by0, 0.0, 0.0};
  if (wx > 0.0 && wy > 0.0) {
    g.nbx = (int)std::min(16384.0, std::max(1.0, std::ceil(std::sqrt(target * wx / wy))));
    g.nby = (int)std::min(16384.0, std::max(1.0, std::ceil(target / g.nbx)));
    g.ibx = g.nbx / wx;
    g.iby = g.nby / wy;
  }
  const int64_t nb = (int64_t)g.nbx * g.nby;
  uint32_t *d_start = nullptr, *d_cursor = nullptr, *d_sums = nullptr, *d_list = nullptr;
  double2 *d_xy = nullptr, *d_val = nullptr, *d_poly = nullptr;
  int *d_id = nullptr;
  SR_RC(buf.alloc(&d_start, (size_t)(nb + 1)));
  SR_RC(buf.alloc(&d_cursor, (size_t)(nb + 1)));
  SR_RC(buf.alloc(&d_sums, (size_t)((nb + 1 + 2047) / 2048)));
  SR_RC(buf.alloc(&d_xy, (size_t)n));
  SR_RC(buf.alloc(&d_val, (size_t)n));
  SR_RC(buf.alloc(&d_id, (size_t)n));
  SR_RC(buf.alloc(&d_list, (size_t)std::max<int64_t>(n, n_nodes)));
  SR_RC(buf.alloc(&d_poly, kDirs));

  // the pre-filter polygon: the hull of the 64 extreme rays
  std::vector<uint32_t> ext;
  for (int k = 0; k < kDirs; ++k)
    if (hw[4 + k]) ext.push_back((uint32_t)(hw[4 + k] & 0xffffffffull));
  const std::vector<uint32_t> poly = monotone_chain(rx, ry, ext);
  const int m = poly.size() >= 3 ? (int)poly.size() : 0;
  std::vector<double2> hpoly((size_t)m);
  for (int k = 0; k < m; ++k) hpoly[k] = make_double2(rx[poly[k]], ry[poly[k]]);
  if (m) SR_HIP(hipMemcpyAsync(d_poly, hpoly.data(), sizeof(double2) * m, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_hull_filter, dim3(sr::grid_for(n, 256)), dim3(256), 0, st, x, y, n, (const double2 *)d_poly, m, d_w + 68,
                     d_list);
  // the counting sort by bin
  SR_HIP(hipMemsetAsync(d_start, 0, sizeof(uint32_t) * (nb + 1), st));
  hipLaunchKernelGGL(k_bin_count, dim3(grid_of(n, 256, 8)), dim3(256), 0, st, x, y, n, g, d_start);
  sr::exclusive_scan_u32(d_start, nb + 1, d_sums, st);
  SR_HIP(hipMemcpyAsync(d_cursor, d_start, sizeof(uint32_t) * (nb + 1), hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_bin_scatter, dim3(grid_of(n, 256, 8)), dim3(256), 0, st, x, y, a, p, n, g, d_cursor, d_xy, d_val, d_id);
  SR_HIP(hipGetLastError());
  unsigned long long n_left = 0;
  SR_HIP(hipMemcpyAsync(&n_left, d_w + 68, sizeof n_left, hipMemcpyDeviceToHost, st));
  SR_HIP(hipStreamSynchronize(st));

  // the exact hull of what the filter left
  std::vector<uint32_t> left((size_t)n_left);
  if (n_left) SR_HIP(hipMemcpy(left.data(), d_list, sizeof(uint32_t) * n_left, hipMemcpyDeviceToHost));
  const std::vector<uint32_t> hull = monotone_chain(rx, ry, left);
  const int nh = hull.size() >= 3 ? (int)hull.size() : 0;
  double2 *d_hull = nullptr;
  SR_RC(buf.alloc(&d_hull, (size_t)std::max(nh, 1)));
  std::vector<double2> hh((size_t)nh);
  for (int k = 0; k < nh; ++k) hh[k] = make_double2(rx[hull[k]], ry[hull[k]]);
  if (nh) SR_HIP(hipMemcpyAsync(d_hull, hh.data(), sizeof(double2) * nh, hipMemcpyHostToDevice, st));

  SR_HIP(hipMemsetAsync(d_w + 68, 0, 4 * sizeof(unsigned long long), st));
  const Bins B{g, d_xy, d_val, d_id, d_start};
  const double *d_gx = d_g, *d_gy = d_g + nx;
  hipLaunchKernelGGL(k_locate, dim3(sr::grid_for(n_nodes, 256)), dim3(256), 0, st, B, (const double2 *)d_hull, nh, d_gx, nx, d_gy,
                     n_nodes, *d_amp, *d_phase, want_tri ? *d_tri : nullptr, d_w + 68, d_list);
  SR_HIP(hipGetLastError());
  unsigned long long c[4];
  SR_HIP(hipMemcpyAsync(c, d_w + 68, sizeof c, hipMemcpyDeviceToHost, st));
  SR_HIP(hipStreamSynchronize(st));
  const unsigned long long n_second = c[0];
  if (n_second) {
    hipLaunchKernelGGL(k_locate_team, dim3(grid_of((int64_t)n_second * kTeam, kTeam, 4)), dim3(kTeam), 0, st, B,
                       (const uint32_t *)d_list, (int64_t)n_second, d_gx, nx, d_gy, *d_amp, *d_phase, want_tri ? *d_tri : nullptr,
                       d_w + 68);
    SR_HIP(hipGetLastError());
    SR_HIP(hipMemcpyAsync(c, d_w + 68, sizeof c, hipMemcpyDeviceToHost, st));
    SR_HIP(hipStreamSynchronize(st));
  }
  if (c[2]) return sr::fail(SR_ERR_HIP, "%s: %llu nodes were not located (a walk ran past %d steps)", who, c[2], kTeamSteps);
  if (stats) {
    const int64_t s[SR_FRESNEL_STATS] = {nh, (int64_t)n_left, g.nbx, g.nby, (int64_t)c[1], (int64_t)n_second};
    std::copy(s, s + SR_FRESNEL_STATS, stats);
  }
  return SR_OK;
}

// fresnel_propagate on the device field d_u (m0 x m1, overwritten) -> out (nr x nc complex128, host)
int propagate_field(const char *who, double2 *d_u, int m0, int m1, const double *fx, const double *fy, const sr_fresnel_params *p,
                    double *out, sr::CallBuffers &buf) {
  hipStream_t st = sr::ctx().stream;
  sr::Fft *F;
  SR_RC(sr::fft_lib(&F));
  hipfftHandle plan = nullptr;
  SR_RC(sr::fft_plan(F, 2, m0, m1, 0, &plan));
  double *d_f = nullptr;
  double2 *d_out = nullptr;
  SR_RC(buf.alloc(&d_f, (size_t)(m0 + m1)));
  SR_RC(buf.alloc(&d_out, (size_t)p->nr * p->nc));
  SR_HIP(hipMemcpyAsync(d_f, fx, sizeof(double) * m0, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(d_f + m0, fy, sizeof(double) * m1, hipMemcpyHostToDevice, st));
  SR_FFT(who, F->SetStream(plan, st));
  SR_FFT(who, F->ExecZ2Z(plan, d_u, d_u, HIPFFT_FORWARD));
  const int64_t n = (int64_t)m0 * m1;
  hipLaunchKernelGGL(k_transfer, dim3(grid_of(n, 256, 32)), dim3(256), 0, st, d_u, m0, m1, (const double *)d_f,
                     (const double *)(d_f + m0), p->pi_lz, p->psf);
  SR_HIP(hipGetLastError());
  SR_FFT(who, F->ExecZ2Z(plan, d_u, d_u, HIPFFT_BACKWARD));
  const int64_t nout = (int64_t)p->nr * p->nc;
  if (nout) {
    hipLaunchKernelGGL(k_crop, dim3(grid_of(nout, 256, 32)), dim3(256), 0, st, (const double2 *)d_u, m1, p->r0, p->nr, p->c0, p->nc,
                       p->post_re, p->post_im, d_out);
    SR_HIP(hipGetLastError());
    SR_HIP(hipMemcpyAsync(out, d_out, sizeof(double2) * nout, hipMemcpyDeviceToHost, st));
  }
  SR_HIP(hipStreamSynchronize(st));
  return SR_OK;
}

int check_rays(const char *who, int64_t n, const double *rx, const double *ry, const double *amp, const double *phase, int nx,
               const double *gx, int ny, const double *gy) {
  SR_CHECK(rx && ry && amp && phase && gx && gy, "%s: NULL argument", who);
  SR_CHECK(n >= 3 && n < INT32_MAX, "%s: %lld rays (3 .. 2^31-2)", who, (long long)n);
  SR_CHECK(nx >= 1 && ny >= 1 && (int64_t)nx * ny < INT32_MAX, "%s: bad grid %d x %d", who, ny, nx);
  for (int64_t i = 0; i < n; ++i)
    SR_CHECK(std::isfinite(rx[i]) && std::isfinite(ry[i]), "%s: ray %lld has a non-finite position", who, (long long)i);
  return SR_OK;
}

int check_params(const char *who, int m0, int m1, const double *fx, const double *fy, const sr_fresnel_params *p) {
  SR_CHECK(fx && fy && p, "%s: NULL argument", who);
  SR_CHECK(m0 >= 1 && m1 >= 1, "%s: bad field %d x %d", who, m0, m1);
  SR_CHECK(p->nr >= 0 && p->nc >= 0 && p->r0 >= 0 && p->c0 >= 0 && p->r0 + p->nr <= m0 && p->c0 + p->nc <= m1,
           "%s: crop rows %d+%d, columns %d+%d outside the %d x %d field", who, p->r0, p->nr, p->c0, p->nc, m0, m1);
  return SR_OK;
}

}  // namespace

extern "C" int sr_fresnel_grid(int64_t n_rays, const double *rx, const double *ry, const double *amp, const double *phase, int nx,
                               const double *gx, int ny, const double *gy, double *amp_out, double *phase_out, int32_t *tri_out,
                               int64_t *stats) {
  const char *who = "sr_fresnel_grid";
  SR_RC(check_rays(who, n_rays, rx, ry, amp, phase, nx, gx, ny, gy));
  SR_CHECK(amp_out && phase_out, "%s: NULL argument", who);
  SR_RC(sr::ensure_init());
  hipStream_t st = sr::ctx().stream;
  sr::CallBuffers buf;
  double *d_amp = nullptr, *d_phase = nullptr;
  int *d_tri = nullptr;
  SR_RC(scatter_to_grid(who, n_rays, rx, ry, amp, phase, nx, gx, ny, gy, tri_out != nullptr, buf, &d_amp, &d_phase, &d_tri, stats));
  const int64_t n_nodes = (int64_t)nx * ny;
  return sr::stage_out(st, {{amp_out, d_amp, sizeof(double) * n_nodes},
                            {phase_out, d_phase, sizeof(double) * n_nodes},
                            {tri_out, d_tri, sizeof(int32_t) * 3 * n_nodes}});
}

extern "C" int sr_fresnel_propagate(const double *u0, int m0, int m1, const double *fx, const double *fy, const sr_fresnel_params *p,
                                    double *out) {
  const char *who = "sr_fresnel_propagate";
  SR_CHECK(u0 && out, "%s: NULL argument", who);
  SR_RC(check_params(who, m0, m1, fx, fy, p));
  SR_RC(sr::ensure_init());
  sr::CallBuffers buf;
  double2 *d_u = nullptr;
  SR_RC(buf.alloc(&d_u, (size_t)m0 * m1));
  SR_RC(sr::upload_sync(d_u, u0, sizeof(double2) * (size_t)m0 * m1, sr::ctx().stream));
  return propagate_field(who, d_u, m0, m1, fx, fy, p, out, buf);
}

extern "C" int sr_fresnel_rays(int64_t n_rays, const double *rx, const double *ry, const double *amp, const double *phase, int nx,
                               const double *gx, int ny, const double *gy, const int32_t *src0, const int32_t *src1, const double *w0,
                               const double *w1, int m0, int m1, const double *fx, const double *fy, const sr_fresnel_params *p,
                               double *out, int64_t *stats) {
  const char *who = "sr_fresnel_rays";
  SR_RC(check_rays(who, n_rays, rx, ry, amp, phase, nx, gx, ny, gy));
  SR_CHECK(src0 && src1 && w0 && w1 && out, "%s: NULL argument", who);
  SR_RC(check_params(who, m0, m1, fx, fy, p));
  for (int r = 0; r < m0; ++r) SR_CHECK(src0[r] >= 0 && src0[r] < ny, "%s: src0[%d] = %d outside 0..%d", who, r, src0[r], ny - 1);
  for (int c = 0; c < m1; ++c) SR_CHECK(src1[c] >= 0 && src1[c] < nx, "%s: src1[%d] = %d outside 0..%d", who, c, src1[c], nx - 1);
  SR_RC(sr::ensure_init());
  hipStream_t st = sr::ctx().stream;
  sr::CallBuffers buf;
  double *d_amp = nullptr, *d_phase = nullptr, *d_w = nullptr;
  int *d_tri = nullptr, *d_src = nullptr;
  double2 *d_u = nullptr;
  SR_RC(scatter_to_grid(who, n_rays, rx, ry, amp, phase, nx, gx, ny, gy, false, buf, &d_amp, &d_phase, &d_tri, stats));
  SR_RC(buf.alloc(&d_src, (size_t)(m0 + m1)));
  SR_RC(buf.alloc(&d_w, (size_t)(m0 + m1)));
  SR_RC(buf.alloc(&d_u, (size_t)m0 * m1));
  SR_HIP(hipMemcpyAsync(d_src, src0, sizeof(int32_t) * m0, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(d_src + m0, src1, sizeof(int32_t) * m1, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(d_w, w0, sizeof(double) * m0, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(d_w + m0, w1, sizeof(double) * m1, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_pad_window, dim3(grid_of((int64_t)m0 * m1, 256, 32)), dim3(256), 0, st, (const double *)d_amp,
                     (const double *)d_phase, nx, (const int *)d_src, (const int *)(d_src + m0), (const double *)d_w,
                     (const double *)(d_w + m0), m0, m1, d_u);
  SR_HIP(hipGetLastError());
  return propagate_field(who, d_u, m0, m1, fx, fy, p, out, buf);
}
