// What the four line-spectra kernels and their entries share beyond the physics of their nodes (sightline_lines.hip,
// sightline_voigt.hip, sightline_zeeman.hip, sightline_stokes.hip): on the device the blocks every kernel of the family runs around
// its own line loop, on the host ONE path under the four entries -- the opening checks in the family's order, the scratch block,
// the packed table, the uploads, the launch and the return of the maps.  A kernel keeps its args struct (kernel-argument layout is
// device code: the helpers are templated on it), its chunk, its line loop and its update; an entry keeps its name, the checks only
// it has, the args members only it has, its LDS size and its kernel's name.  Included inside the including unit's anonymous
// namespace, after sightline_march.inc, line_node.inc, voigt_node.inc and zeeman_node.inc (every unit of the family includes the
// three: the host path reads all their tables); only the four line kernels include it.

// ---- device: the decomposition every kernel of the family has.  A workgroup owns one chord and one tile of FL frequencies, a lane
// one frequency with its Stokes parameters and tau in registers; the chord's samples go through LDS in chunks, in march order, in
// two buffers, and the corner reads of chunk c+1 are issued before the march of chunk c and blended after it.  A staged sample is
// a head -- S[0] = ne*h, S[1] = flags (1: the continuum is dark, 2: the lines are), S[2..8] = node_terms' seven, S[9] padding,
// then what the kernel adds -- and the constants of its lines.  Trip counts are uniform in a workgroup, a missed chord leaves before
// the first barrier, the last tile's idle lanes stage but neither march nor store, tile 0's lane 0 writes column, chord and steps.
// Here are the blocks whose move into a helper left every instruction of every kernel as it was (tools/kernel_diff.py); the
// others the kernels share -- the lattices' staging, the unpacking of a staged continuum, the line constants of the two polarised
// kernels, the final stores -- changed register allocation or block order and stay spelled out in each kernel
// (profiles/line_family_kernels.txt).

// A lane's frequency: its constants and the span of its wavefront's frequencies
struct LaneFreq {
  double om, eph, com, wmin, wmax;
};
// an idle lane of the last tile takes the last frequency's constants and stores nothing; idle lanes widen no span
template <typename Args>
__device__ __forceinline__ LaneFreq lane_freq(const Args &X, int f, bool active) {
  const int fc = active ? f : X.n_freq - 1;
  LaneFreq w;
  w.om = X.omega[fc], w.eph = X.e_ph[fc], w.com = X.c_omega[fc];
  w.wmin = wave_extreme<true>(active ? w.om : HUGE_VAL), w.wmax = wave_extreme<false>(active ? w.om : -HUGE_VAL);
  return w;
}

// The head of a staged sample S from the blended (ne, Te, Z); dark: its lines are (their constants are then not staged)
__device__ __forceinline__ void stage_head(double *S, bool cont, bool dark, double ne, double Te, double Z, double h) {
  int flags = dark ? 2 : 0;
  S[0] = ne * h;
  if (cont) {
    const NodeTerms c = node_terms(ne, Te, Z);
    flags |= c.dark ? 1 : 0;
    S[2] = c.Te, S[3] = c.n, S[4] = c.wp, S[5] = c.L, S[6] = c.num, S[7] = c.zc, S[8] = c.it;
  }
  S[1] = (double)flags;
}

// The update by a sample none of whose lines reached this frequency: the continuum alone, or that update with ac = Sc = 0 --
// exp(-0) = 1 and expm1(-0) = -0 exactly, I*1 + 0*0 and tau + 0
__device__ __forceinline__ void continuum_update(bool cont, double ac, double Sc, double h, double &I, double &tau) {
  if (cont) {
    const double dtau = ac * h;
    I = I * exp(-dtau) + Sc * (-expm1(-dtau));
    tau = tau + dtau;
  } else {
    I = I + 0.0;
    tau = tau + 0.0;
  }
}
// and on four Stokes parameters: one attenuation for all
__device__ __forceinline__ void continuum_update(bool cont, double ac, double Sc, double h, double &I, double &Q, double &U, double &Vs,
                                                 double &tau) {
  if (cont) {
    const double dtau = ac * h;
    const double E = exp(-dtau);
    I = I * E + Sc * (-expm1(-dtau));
    Q = Q * E;
    U = U * E;
    Vs = Vs * E;
    tau = tau + dtau;
  } else {
    I = I + 0.0;
    Q = Q + 0.0;
    U = U + 0.0;
    Vs = Vs + 0.0;
    tau = tau + 0.0;
  }
}

// A chord that misses the box (the whole workgroup; tile 0's lane 0 writes the chord's own): the backlight and no optical depth,
// column, chord or step
__device__ __forceinline__ void store_missed(const EmArgs &A, const LineArgs &L, int64_t i, int64_t at, bool active, int tile, int lane) {
  if (active) {
    A.I[at] = A.back ? A.back[at] : 0.0;
    A.tau[at] = 0.0;
  }
  if (tile == 0 && lane == 0) {
    L.column[i] = 0.0;
    L.chord[i] = 0.0;
    L.steps[i] = 0;
  }
}

// ---- host: one path under the four entries (`who` names the entry in every error text)

// The arguments every entry takes, as it was given them, and from check_family on the shape of the launch
struct Family {
  const char *who;
  const sr_field *ne, *Te, *Ti, *Z, *V;
  const sr_lines_params *m;  // the march: the entry's p or &p->march, NULL where p is
  int64_t n;
  const double *origin, *dir;
  int32_t n_freq;
  const double *omega, *e_ph, *c_omega, *backlight;
  double *I, *tau, *column, *chord;
  int32_t *steps;
  double *kernel_ms;
  int fl = 0;  // lanes per workgroup = frequencies per tile
  int64_t n_tiles = 0;
};
// What the polarised entries take beside them, and the chord frames check_family makes of ref
struct Polarised {
  const sr_field *B;
  const double *ref;
  double *Q, *U, *Vs;
  const sr_zeeman_table *lines;
  std::vector<double> frames;
};
// which members an entry's args struct has beside LinesArgs': kVoigtArgs LG, kPolarisedArgs LG, has_lg, B, frame, comp, off, Q, U, Vs
enum ArgsKind { kLinesArgs, kVoigtArgs, kPolarisedArgs };

inline int check_wing(const char *who, double wing) {
  SR_CHECK(wing > 0.0, "%s: wing must be positive (+inf is allowed), got %g", who, wing);
  return SR_OK;
}

// The family's opening checks, in the family's order.  table(): the checks of the entry's table and, where the entry reads it,
// check_wing.  P: the polarised entries'.  n == 0 and n_freq == 0 skip none of them.
template <typename Table>
inline int check_family(Family &F, Table &&table, Polarised *P = nullptr) {
  const char *who = F.who;
  SR_CHECK(F.m != nullptr && F.origin != nullptr && F.dir != nullptr && F.I != nullptr && F.tau != nullptr, "%s: NULL argument", who);
  if (P) SR_CHECK(P->ref != nullptr && P->Q != nullptr && P->U != nullptr && P->Vs != nullptr, "%s: NULL ref, Q, U or Vs (B is given)", who);
  SR_CHECK(F.omega != nullptr && F.e_ph != nullptr && F.c_omega != nullptr, "%s: NULL omega, e_ph or c_omega", who);
  SR_CHECK(F.n >= 0, "%s: n must not be negative, got %lld", who, (long long)F.n);
  SR_CHECK(F.n_freq >= 0, "%s: n_freq must not be negative, got %d", who, F.n_freq);
  if (F.n_freq != 0) SR_RC(check_bands(who, "frequency", F.n_freq, SR_MAX_FREQS, F.omega, F.e_ph, F.c_omega));
  SR_RC(check_march(who, F.m->toward, F.m->step, F.m->max_steps));
  SR_RC(table());
  F.fl = lane_width(F.n_freq);
  F.n_tiles = (F.n_freq + F.fl - 1) / F.fl;
  SR_CHECK(F.n_tiles == 0 || F.n <= (int64_t)2147483647 / F.n_tiles, "%s: n x frequency tiles exceeds 2^31 - 1 workgroups", who);
  if (P) SR_RC(chord_frames(who, F.n, F.m->toward, F.dir, P->ref, P->frames));  // before check_lines: see there
  SR_RC(check_lines(who, F.n, F.origin, F.dir, F.ne, F.Te, F.Z));
  return sr::check_fields(who, F.ne, "ne", {{"Ti", F.Ti, 1}, {"V", F.V, 3}, {"B", P ? P->B : nullptr, 3}});
}

// A polarised entry without B: sr_field_sightline_voigt's rule, kernel and bits under that entry's name, and exact zeros in Q, U
// and Vs (each may be NULL); the component table and ref are not read
inline int without_field(const Family &F, const Polarised &P, const sr_voigt_params *p) {
  SR_CHECK(P.lines != nullptr, "%s: NULL line table", F.who);
  SR_CHECK(F.n >= 0 && F.n_freq >= 0, "%s: n and n_freq must not be negative, got %lld and %d", F.who, (long long)F.n, F.n_freq);
  SR_RC(sr_field_sightline_voigt(F.ne, F.Te, F.Ti, F.Z, F.V, &P.lines->voigt, p, F.n, F.origin, F.dir, F.n_freq, F.omega, F.e_ph, F.c_omega,
                                 F.backlight, F.I, F.tau, F.column, F.chord, F.steps, F.kernel_ms));
  const size_t bytes = sizeof(double) * (size_t)F.n * (size_t)F.n_freq;
  for (double *out : {P.Q, P.U, P.Vs})
    if (out && bytes) memset(out, 0, bytes);
  return SR_OK;
}

// From the checks' end to the maps' return.  One scratch block: the chords' pieces (take_lines) | Q | U | Vs | frames | omega | e_ph
// | c_omega | table | components | offsets, the polarised entries' pieces only with P.  X comes with the members only its entry
// has and leaves with the family's; t->LG may be NULL (pack_line_table's block).  kernel(f64, te, z, ti, v, narrow), called with
// std::bool_constant's, returns the entry's kernel for these flags: a kernel template cannot be passed itself.
template <ArgsKind KIND, typename Args, typename Kernel>
inline int run_family(const Family &F, const sr_voigt_table *t, const Polarised *P, Args &X, size_t lds, Kernel &&kernel) {
  if (F.kernel_ms) *F.kernel_ms = 0.0;
  if (F.n == 0 || F.n_freq == 0) return SR_OK;
  SR_RC(sr::ensure_init());
  sr::Context &c = sr::ctx();
  hipStream_t st = c.stream;

  const sr_line_table *lt = &t->lines;
  const sr_lines_params *m = F.m;
  const std::vector<double> pack = pack_voigt_table(t);
  const size_t nl = (size_t)lt->n_line, entries = (size_t)lt->nT * lt->nD * nl;
  const size_t nf = (size_t)F.n_freq, map = nf * (size_t)F.n, map_bytes = sizeof(double) * map, freq_bytes = sizeof(double) * nf;
  std::vector<int> off(nl + 1, 0);  // line l's components are off[l] .. off[l+1]-1
  if constexpr (KIND == kPolarisedArgs)
    for (size_t q = 0; q < nl; ++q) off[q + 1] = off[q] + P->lines->n_comp[q];
  const size_t n_comp = (size_t)off[nl];

  EmArgs A{};
  LineArgs L{};
  FlowArgs W{};
  double *tab = nullptr;
  sr::Carve carve;
  take_lines(carve, A, L, F.ne, F.n, m->step, m->max_steps, nf, F.backlight != nullptr);
  if constexpr (KIND == kPolarisedArgs) {
    carve.take(&X.Q, map);
    carve.take(&X.U, map);
    carve.take(&X.Vs, map);
    carve.take(&X.frame, P->frames.size());
  }
  carve.take(&X.omega, nf);
  carve.take(&X.e_ph, nf);
  carve.take(&X.c_omega, nf);
  carve.take(&tab, pack.size());
  if constexpr (KIND == kPolarisedArgs) {
    carve.take(&X.comp, 3 * n_comp);
    carve.take(&X.off, off.size());
  }
  if (!carve.alloc()) return SR_ERR_HIP;
  fill_fields(A, F.ne, F.Te, F.Z, m->toward, m->Te, m->Z, 0, nullptr, nullptr, nullptr);  // the frequencies' constants are X's
  W.Ti = F.Ti ? F.Ti->data : nullptr;
  W.V = F.V ? F.V->data : nullptr;
  X.n_freq = F.n_freq;
  X.n_tiles = (int)F.n_tiles;
  X.LT = tab;
  X.LD = X.LT + lt->nT;
  X.w0 = X.LD + lt->nD;
  X.ci = X.w0 + nl;
  X.LJ = X.ci + nl;
  X.LK = X.LJ + entries;  // not read where has_lk is false
  X.nT = lt->nT;
  X.nD = lt->nD;
  X.n_line = lt->n_line;
  X.has_lk = lt->LK != nullptr;
  X.continuum = m->continuum != 0;
  if constexpr (KIND != kLinesArgs) X.LG = lt->LK ? X.LK + entries : X.LK;  // not read where there is no LG
  if constexpr (KIND == kPolarisedArgs) {
    X.has_lg = t->LG != nullptr;
    X.B = P->B->data;
  }

  SR_RC(upload_lines(A, L, F.origin, F.dir, F.backlight, map_bytes, st));
  if constexpr (KIND == kPolarisedArgs)
    SR_HIP(hipMemcpyAsync(const_cast<double *>(X.frame), P->frames.data(), sizeof(double) * P->frames.size(), hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(X.omega), F.omega, freq_bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(X.e_ph), F.e_ph, freq_bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(const_cast<double *>(X.c_omega), F.c_omega, freq_bytes, hipMemcpyHostToDevice, st));
  SR_HIP(hipMemcpyAsync(tab, pack.data(), sizeof(double) * pack.size(), hipMemcpyHostToDevice, st));
  if constexpr (KIND == kPolarisedArgs) {
    SR_HIP(hipMemcpyAsync(const_cast<double *>(X.comp), P->lines->comp, sizeof(double) * 3 * n_comp, hipMemcpyHostToDevice, st));
    SR_HIP(hipMemcpyAsync(const_cast<int *>(X.off), off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, st));
  }
  SR_HIP(hipEventRecord(c.ev[0], st));
  const unsigned grid = (unsigned)(F.n * F.n_tiles);
  sr::with_flags(
      [&](auto f64, auto te, auto z, auto ti, auto v, auto narrow) {
        const auto k = kernel(f64, te, z, ti, v, narrow);
        hipLaunchKernelGGL(k, dim3(grid), dim3(decltype(narrow)::value ? 64 : 256), lds, st, A, L, W, X);
      },
      (bool)F.ne->is_f64, F.Te != nullptr, F.Z != nullptr, F.Ti != nullptr, F.V != nullptr, F.fl == 64);
  if constexpr (KIND == kPolarisedArgs)
    return finish_lines(A, L, map_bytes, F.I, F.tau, F.column, F.chord, F.steps, F.kernel_ms, {{X.Q, P->Q}, {X.U, P->U}, {X.Vs, P->Vs}});
  else
    return finish_lines(A, L, map_bytes, F.I, F.tau, F.column, F.chord, F.steps, F.kernel_ms);
}
