// What the sightline kernels must share so that they return the same bits (include/synthray.h's sightlines section: clip,
// steps, sample, gather): sightlines.hip (k_sightlines: a line per lane, up to SR_MAX_BANDS bands), sightline_spectra.hip
// (k_sightline_spectra: a frequency per lane) and sightline_lines.hip (k_sightline_lines: a frequency per lane, spectral lines on
// the continuum; its samples also carry Ti and V: FlowSample); after the device code, the host code the entries run around their
// kernels.  Included inside the including unit's anonymous namespace, after emission_march.inc (EmArgs) and <cstdlib>.

struct LineArgs {
  sr::FieldGrid f;      // lo, hi: the box
  const double *o, *d;  // (3, n) origins and directions
  double *column, *chord;
  int32_t *steps;
  int64_t n;
  int max_steps;
  double step;
};

// One sample of a line: where it lies in its cell, and the corners of the fields there (read, not yet blended)
template <typename T, bool HAS_TE, bool HAS_Z>
struct Sample {
  bool in;
  double ux, wx, w00, w01, w10, w11;
  sr::Corners<T> ne, Te, Z;
};

// more(ci, cj, ck): the corner reads of the fields a kernel gathers beside ne, Te, Z, at the cell of a sample inside the box
template <typename T, bool HAS_TE, bool HAS_Z, typename More>
__device__ __forceinline__ void fetch(const EmArgs &A, const sr::FieldGrid &f, int64_t sx, int64_t sy, double px, double py,
                                      double pz, Sample<T, HAS_TE, HAS_Z> &s, More &&more) {
  int ci = 0, cj = 0, ck = 0;
  double wx = 0, wy = 0, wz = 0;
  const bool in_x = sr::locate_in<true>(f.g[0], f.n[0], f.inv_h[0], f.lo[0], f.hi[0], px, ci, wx);
  const bool in_y = sr::locate_in<true>(f.g[1], f.n[1], f.inv_h[1], f.lo[1], f.hi[1], py, cj, wy);
  const bool in_z = sr::locate_in<true>(f.g[2], f.n[2], f.inv_h[2], f.lo[2], f.hi[2], pz, ck, wz);
  s.in = in_x && in_y && in_z;
  if (s.in) {  // locate_in leaves every cell index in [0, n - 2]: the eight corners are nodes of the field
    const double uy = 1.0 - wy, uz = 1.0 - wz;
    s.ux = 1.0 - wx;
    s.wx = wx;
    s.w00 = uy * uz;
    s.w01 = uy * wz;
    s.w10 = wy * uz;
    s.w11 = wy * wz;
    s.ne = sr::corners_load(static_cast<const T *>(A.ne), 1, 0, sx, sy, ci, cj, ck);
    if (HAS_TE) s.Te = sr::corners_load(static_cast<const T *>(A.Te), 1, 0, sx, sy, ci, cj, ck);
    if (HAS_Z) s.Z = sr::corners_load(static_cast<const T *>(A.Z), 1, 0, sx, sy, ci, cj, ck);
    more(ci, cj, ck);
  }
}
template <typename T, bool HAS_TE, bool HAS_Z>
__device__ __forceinline__ void fetch(const EmArgs &A, const sr::FieldGrid &f, int64_t sx, int64_t sy, double px, double py,
                                      double pz, Sample<T, HAS_TE, HAS_Z> &s) {
  fetch<T, HAS_TE, HAS_Z>(A, f, sx, sy, px, py, pz, s, [](int, int, int) {});
}

// the blended (ne, Te, Z) of a fetched sample; outside the box (within rounding of a face): ne = 0, which either node takes for dark
template <typename T, bool HAS_TE, bool HAS_Z>
__device__ __forceinline__ void blend_sample(const EmArgs &A, const Sample<T, HAS_TE, HAS_Z> &s, double &ne, double &Te, double &Z) {
  ne = 0.0, Te = A.uTe, Z = A.uZ;
  if (s.in) {
    ne = sr::corners_blend(s.ne, s.ux, s.wx, s.w00, s.w01, s.w10, s.w11);
    if (HAS_TE) Te = sr::corners_blend(s.Te, s.ux, s.wx, s.w00, s.w01, s.w10, s.w11);
    if (HAS_Z) Z = sr::corners_blend(s.Z, s.ux, s.wx, s.w00, s.w01, s.w10, s.w11);
  }
}

// The clip and the steps of line i
struct Line {
  double o0, o1, o2, d0, d1, d2;
  bool hit;
  int n;                     // samples; 0: a miss
  double t0, chord, dt, h;   // sample k lies at t0 + (k + 0.5)*dt
};

__device__ __forceinline__ Line line_of(const LineArgs &L, int64_t i) {
  const int64_t N = L.n;
  Line l;
  l.o0 = L.o[i], l.o1 = L.o[N + i], l.o2 = L.o[2 * N + i];
  l.d0 = L.d[i], l.d1 = L.d[N + i], l.d2 = L.d[2 * N + i];
  // clip: the half-line t >= 0 against the box, axis by axis
  double t0 = 0.0, t1 = HUGE_VAL;
  bool hit = true;
  auto clip = [&](double o, double d, double lo, double hi) {
    if (d == 0.0) {
      hit = hit && lo <= o && o <= hi;
    } else {
      const double ta = (lo - o) / d, tb = (hi - o) / d;
      const double tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
      t0 = t0 > tn ? t0 : tn;
      t1 = t1 < tf ? t1 : tf;
    }
  };
  clip(l.o0, l.d0, L.f.lo[0], L.f.hi[0]);
  clip(l.o1, l.d1, L.f.lo[1], L.f.hi[1]);
  clip(l.o2, l.d2, L.f.lo[2], L.f.hi[2]);
  l.hit = hit && t1 > t0;
  l.n = 0;
  l.t0 = t0;
  l.chord = l.dt = l.h = 0.0;
  if (l.hit) {
    const double len = sqrt((l.d0 * l.d0 + l.d1 * l.d1) + l.d2 * l.d2);
    l.chord = (t1 - t0) * len;
    const double q = l.chord / L.step;
    if (!(q < (double)L.max_steps)) {  // q >= max_steps, or a NaN q (a direction whose squares underflow)
      l.n = L.max_steps;
    } else {
      l.n = (int)ceil(q);
      l.n = l.n < 1 ? 1 : l.n;
    }
    l.dt = (t1 - t0) / (double)l.n;
    l.h = l.chord / (double)l.n;
  }
  return l;
}

// the cell search and the corner reads of sample k of a line
template <typename T, bool HAS_TE, bool HAS_Z>
__device__ __forceinline__ void fetch_sample(const EmArgs &A, const sr::FieldGrid &f, int64_t sx, int64_t sy, const Line &l, int k,
                                             Sample<T, HAS_TE, HAS_Z> &s) {
  const double t = l.t0 + ((double)k + 0.5) * l.dt;
  fetch<T, HAS_TE, HAS_Z>(A, f, sx, sy, l.o0 + l.d0 * t, l.o1 + l.d1 * t, l.o2 + l.d2 * t, s);
}

// A sample that also carries the ion temperature and the flow (sightline_lines.hip): Sample's cell and weights, and the corners of
// Ti and of the three components of V (a (nx, ny, nz, 3) field) at the same cell.
struct FlowArgs {
  const void *Ti, *V;  // unused where the kernel is instantiated without them
};
template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI, bool HAS_V>
struct FlowSample {
  Sample<T, HAS_TE, HAS_Z> s;
  sr::Corners<T> Ti, V0, V1, V2;
};

template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI, bool HAS_V>
__device__ __forceinline__ void fetch_sample(const EmArgs &A, const FlowArgs &W, const sr::FieldGrid &f, int64_t sx, int64_t sy,
                                             const Line &l, int k, FlowSample<T, HAS_TE, HAS_Z, HAS_TI, HAS_V> &s) {
  const double t = l.t0 + ((double)k + 0.5) * l.dt;
  fetch<T, HAS_TE, HAS_Z>(A, f, sx, sy, l.o0 + l.d0 * t, l.o1 + l.d1 * t, l.o2 + l.d2 * t, s.s, [&](int ci, int cj, int ck) {
    if (HAS_TI) s.Ti = sr::corners_load(static_cast<const T *>(W.Ti), 1, 0, sx, sy, ci, cj, ck);
    if (HAS_V) {
      s.V0 = sr::corners_load(static_cast<const T *>(W.V), 3, 0, sx, sy, ci, cj, ck);
      s.V1 = sr::corners_load(static_cast<const T *>(W.V), 3, 1, sx, sy, ci, cj, ck);
      s.V2 = sr::corners_load(static_cast<const T *>(W.V), 3, 2, sx, sy, ci, cj, ck);
    }
  });
}

// blend_sample's (ne, Te, Z), and Ti (Te where there is no Ti field) and V (0 where there is no V field); outside the box Ti = Te
// and V = 0 beside blend_sample's ne = 0
template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI, bool HAS_V>
__device__ __forceinline__ void blend_sample(const EmArgs &A, const FlowSample<T, HAS_TE, HAS_Z, HAS_TI, HAS_V> &s, double &ne,
                                             double &Te, double &Z, double &Ti, double (&V)[3]) {
  blend_sample<T, HAS_TE, HAS_Z>(A, s.s, ne, Te, Z);
  Ti = Te;
  V[0] = V[1] = V[2] = 0.0;
  if (s.s.in) {
    const Sample<T, HAS_TE, HAS_Z> &c = s.s;
    if (HAS_TI) Ti = sr::corners_blend(s.Ti, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
    if (HAS_V) {
      V[0] = sr::corners_blend(s.V0, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
      V[1] = sr::corners_blend(s.V1, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
      V[2] = sr::corners_blend(s.V2, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
    }
  }
}

// Sample k's cell and weights alone (fetch's search, the same bits) and the corners of the three components of `vec` (a
// (nx, ny, nz, 3) field) there, in the slots a FlowSample keeps for V: how a lane that stages no sample of its own carries a
// second vector field (sightline_zeeman.hip: B) across a march without any lane's live state growing.
template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI>
__device__ __forceinline__ void fetch_vector(const void *vec, const sr::FieldGrid &f, int64_t sx, int64_t sy, const Line &l, int k,
                                             FlowSample<T, HAS_TE, HAS_Z, HAS_TI, true> &s) {
  const double t = l.t0 + ((double)k + 0.5) * l.dt;
  const double px = l.o0 + l.d0 * t, py = l.o1 + l.d1 * t, pz = l.o2 + l.d2 * t;
  int ci = 0, cj = 0, ck = 0;
  double wx = 0, wy = 0, wz = 0;
  const bool in_x = sr::locate_in<true>(f.g[0], f.n[0], f.inv_h[0], f.lo[0], f.hi[0], px, ci, wx);
  const bool in_y = sr::locate_in<true>(f.g[1], f.n[1], f.inv_h[1], f.lo[1], f.hi[1], py, cj, wy);
  const bool in_z = sr::locate_in<true>(f.g[2], f.n[2], f.inv_h[2], f.lo[2], f.hi[2], pz, ck, wz);
  s.s.in = in_x && in_y && in_z;
  if (s.s.in) {
    const double uy = 1.0 - wy, uz = 1.0 - wz;
    s.s.ux = 1.0 - wx;
    s.s.wx = wx;
    s.s.w00 = uy * uz;
    s.s.w01 = uy * wz;
    s.s.w10 = wy * uz;
    s.s.w11 = wy * wz;
    s.V0 = sr::corners_load(static_cast<const T *>(vec), 3, 0, sx, sy, ci, cj, ck);
    s.V1 = sr::corners_load(static_cast<const T *>(vec), 3, 1, sx, sy, ci, cj, ck);
    s.V2 = sr::corners_load(static_cast<const T *>(vec), 3, 2, sx, sy, ci, cj, ck);
  }
}

// the vector fetch_vector read, blended; outside the box 0
template <typename T, bool HAS_TE, bool HAS_Z, bool HAS_TI>
__device__ __forceinline__ void blend_vector(const FlowSample<T, HAS_TE, HAS_Z, HAS_TI, true> &s, double (&B)[3]) {
  B[0] = B[1] = B[2] = 0.0;
  if (s.s.in) {
    const Sample<T, HAS_TE, HAS_Z> &c = s.s;
    B[0] = sr::corners_blend(s.V0, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
    B[1] = sr::corners_blend(s.V1, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
    B[2] = sr::corners_blend(s.V2, c.ux, c.wx, c.w00, c.w01, c.w10, c.w11);
  }
}

// ---- host: what sr_field_sightlines and sr_field_sightline_spectra do around their kernels (`who` names the entry in the error
// text).  An entry keeps its kernel and dispatch, its table's packing and the checks only it has.

// the march: before the table's checks
inline int check_march(const char *who, int toward, double step, int max_steps) {
  SR_CHECK(toward == 1 || toward == -1, "%s: toward must be +1 or -1, got %d", who, toward);
  SR_CHECK(sr::positive(step), "%s: step must be finite and positive", who);
  SR_CHECK(max_steps >= 1, "%s: max_steps must be at least 1, got %d", who, max_steps);
  return SR_OK;
}

// The kernels with a frequency per lane (sightline_spectra.hip, sightline_lines.hip): lanes per workgroup = frequencies per tile,
// 256 or 64, whichever leaves fewer lanes of a line's last tile idle, 256 where they tie.  SYNTHRAY_SPECTRA_FL = 64 | 256 overrides
// the choice (tools/sightline_spectra_rate.py measures the two against each other).
inline int lane_width(int n_freq) {
  if (const char *e = getenv("SYNTHRAY_SPECTRA_FL")) {
    const int v = atoi(e);
    if (v == 64 || v == 256) return v;
  }
  return (n_freq + 255) / 256 * 256 == (n_freq + 63) / 64 * 64 ? 256 : 64;  // 193..256 of every 256
}

// the lines and the fields: an entry's last checks (n == 0 does not skip them)
inline int check_lines(const char *who, int64_t n, const double *origin, const double *dir, const sr_field *ne, const sr_field *Te,
                       const sr_field *Z) {
  for (int64_t k = 0; k < 3 * n; ++k) {
    SR_CHECK(std::isfinite(origin[k]), "%s: non-finite origin of line %lld", who, (long long)(k % n));
    SR_CHECK(std::isfinite(dir[k]), "%s: non-finite direction of line %lld", who, (long long)(k % n));
  }
  for (int64_t k = 0; k < n; ++k)
    SR_CHECK(dir[k] != 0.0 || dir[n + k] != 0.0 || dir[2 * n + k] != 0.0, "%s: the direction of line %lld is zero", who, (long long)k);
  SR_CHECK(ne != nullptr, "%s: NULL ne field", who);
  return sr::check_fields(who, ne, "ne", {{"ne", ne, 1}, {"Te", Te, 1}, {"Z", Z, 1}});
}

// LineArgs but for its pointers, and the head of the call's scratch block from the caller's Carve: I | tau | backlight | origins |
// directions | column | chord | steps, I and tau with `per_line` values a line.  What one entry alone needs goes behind.
inline void take_lines(sr::Carve &carve, EmArgs &A, LineArgs &L, const sr_field *ne, int64_t n, double step, int max_steps,
                       size_t per_line, bool backlight) {
  const size_t N = (size_t)n;
  A.ncol = L.n = n;
  L.f = sr::grid_of(ne);
  L.max_steps = max_steps;
  L.step = step;
  carve.take(&A.I, per_line * N);
  carve.take(&A.tau, per_line * N);
  if (backlight) carve.take(&A.back, per_line * N);
  carve.take(&L.o, 3 * N);
  carve.take(&L.d, 3 * N);
  carve.take(&L.column, N);
  carve.take(&L.chord, N);
  carve.take(&L.steps, N);
}

// origins, directions and the backlight (map_bytes of it) go up
inline int upload_lines(const EmArgs &A, const LineArgs &L, const double *origin, const double *dir, const double *backlight,
                        size_t map_bytes, hipStream_t st) {
  const size_t bytes = sizeof(double) * 3 * (size_t)L.n;
  SR_HIP(hipMemcpyAsync(const_cast<double *>(L.o), origin, bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(L.d), dir, bytes, hipMemcpyHostToDevice, st));
  if (backlight) SR_HIP(hipMemcpyAsync(const_cast<double *>(A.back), backlight, map_bytes, hipMemcpyHostToDevice, st));
  return SR_OK;
}

// After the launch: I, tau and the per-line outputs that were asked for come back, the kernel's time is read.  `more`: further
// maps of map_bytes (device, host), which come back before I (the polarised entries' Q, U and Vs).
inline int finish_lines(const EmArgs &A, const LineArgs &L, size_t map_bytes, double *I, double *tau, double *column, double *chord,
                        int32_t *steps, double *kernel_ms, std::initializer_list<std::pair<const double *, double *>> more = {}) {
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;
  const size_t N = (size_t)L.n;
  SR_HIP(hipGetLastError());
  SR_HIP(hipEventRecord(c.ev[1], st));
  for (const auto &m : more) SR_HIP(hipMemcpyAsync(m.second, m.first, map_bytes, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(I, A.I, map_bytes, hipMemcpyDeviceToHost, st));
  SR_HIP(hipMemcpyAsync(tau, A.tau, map_bytes, hipMemcpyDeviceToHost, st));
  if (column) SR_HIP(hipMemcpyAsync(column, L.column, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  if (chord) SR_HIP(hipMemcpyAsync(chord, L.chord, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  if (steps) SR_HIP(hipMemcpyAsync(steps, L.steps, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
  return sr::finish_timed(c, kernel_ms);
}
