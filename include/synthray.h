/*
 * synthray.h — C ABI of libsynthray.so: the MI355X (gfx950) engine for synthPy's
 * ray-propagation → detector hot path.
 *
 * The reference (MAGPIE-ICL/synthPy) is pure Python and has no FFI of its own; the
 * boundary sits directly beneath its Python API and each entry point below replaces
 * the body of one reference function (cited as path:line in the reference tree).
 * Plain pointers and sizes only.  Conventions follow the reference's NumPy layouts:
 *   rays     (9, N) float64 row-major: x y z vx vy vz amplitude phase polarisation
 *   rf       (4, N) float64: x theta y phi         Jf (2, N) complex128 (re, im interleaved)
 *   volumes  C-order [ix][iy][iz] (z fastest), coordinates float32 as ScalarDomain keeps them
 *   images   [y_bin][x_bin]
 *
 * Ownership: the caller owns every host buffer; the library owns device memory behind
 * opaque handles and keeps no host pointer after a call returns.
 * Errors: 0 on success, a negative SR_ERR_* otherwise, text via sr_last_error()
 * (thread-local).  A ray that fails (rejected by an aperture, NaN input) is NaN in the
 * output, never an error — as in the reference.
 * Threading: one device per process/thread; calls are serialised on one HIP stream.
 */
#ifndef SYNTHRAY_H
#define SYNTHRAY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR_OK 0
#define SR_ERR_INVALID (-1)  /* bad argument */
#define SR_ERR_HIP (-2)      /* a HIP runtime call failed (no device, out of memory, launch) */
#define SR_ERR_RCCL (-3)     /* RCCL missing or a collective failed */
#define SR_ERR_STATE (-4)    /* handle used before the data it needs exists */

typedef struct sr_volume sr_volume; /* device-resident fields of one ScalarDomain */
typedef struct sr_rays sr_rays;     /* device-resident ray bundle: s0, then sf / rf / Jf */
typedef struct sr_image sr_image;   /* device-resident detector image */
typedef struct sr_comm sr_comm;     /* RCCL communicator (one rank per GPU) */

/* ---- runtime ------------------------------------------------------------------ */
/* Threading and processes: ONE device per process, and the library is NOT thread-safe -- its context (device, the two
 * streams, the selected stream, timing events) is process-global, and sr_init(other_device) re-creates the streams, so
 * no handle made on the first device may be live across it.  Multi-GPU = one process per GPU (bench.py, run_trace,
 * distributed.py), as the reference runs one MPI rank per device.  Calls from one thread at a time. */
int sr_init(int device);            /* select the GPU and create the stream; idempotent per device */
/* >= 0, or SR_ERR_HIP.  0 only when the machine has no amdgpu driver node (/dev/kfd) this process may open.  Before the
 * process's first HIP call the device is opened in a bounded retry (open(/dev/kfd) + hsa_init, 6 tries, 50 ms doubling):
 * ranks of one job start in the same instant, and HIP's once-per-process initialisation cannot be repeated after it found
 * no agent.  A failure keeps the runtime's own words (errno / HSA status / hipError name) in sr_last_error(). */
int sr_device_count(void);
int sr_synchronize(void);            /* waits for every stream of the library */
/* HBM free / in all on the selected device (hipMemGetInfo): what ScalarDomain's auto_batching sizes its regions from
 * (the reference asks psutil / pynvml, src/simulator/domain.py:140-165) */
int sr_device_memory(int64_t *free_bytes, int64_t *total_bytes);
/* Every launch that covers its work with a grid-stride loop takes min(the blocks the work needs, n_cu * k) blocks (k = 4 .. 64
 * per site, at least one block).  sr_grid_cus sets the n_cu those caps are sized for -- a measurement and test knob, like
 * SYNTHRAY_RESAMPLE_BRICK: fewer compute units make the loops take their later trips at small sizes, and it is an occupancy
 * knob for timing.  n_cu > 0: as on a device of n_cu compute units; 0: back to the device's own count (the default; results
 * and grids are then exactly what they are without this call); -1: read only; anything else is SR_ERR_INVALID.  *in_force
 * (may be NULL) receives the count now in force.  No kernel needs a minimum grid: results do not depend on the count, bit for
 * bit, except where an entry point says that it adds with floating-point atomics. */
int sr_grid_cus(int n_cu, int *in_force);
/* out[0]: launches sized by such a cap since the last reset; out[1]: those of them that got fewer blocks than they wanted,
 * i.e. whose loop takes a second trip.  reset != 0 zeroes both after reading; out may be NULL. */
int sr_grid_stats(int64_t out[2], int reset);
/* Every call queues its GPU work on the library's SELECTED stream (0 by default; 1 = a second one).  Work on different
 * streams may overlap: a job of many small ray bundles alternates them so that one bundle's tail runs beside the next
 * one's start-up (the reference's drivers trace 5e5-ray chunks one after the other, pvti_trace_mpi.py:144-163).  The
 * caller orders what the streams share: sr_synchronize() after creating volumes / zeroing images and before reading
 * images; a ray bundle is used with one stream at a time. */
int sr_stream_select(int index);
/* Orders the two streams without stopping the host: work queued on stream `waiting` AFTER this call starts once everything
 * queued on stream `on` BEFORE it is done.  The slab pipeline traces on stream 0 and moves the hand-off records (ncclSend /
 * ncclRecv) on stream 1, so that the send of chunk i runs beside the trace of chunk i+1 (distributed.SlabPipeline). */
int sr_stream_wait(int waiting, int on);
/* Page-locked host memory (hipHostMalloc): copies between it and the GPU run at the speed of the link and beside GPU work,
 * where pageable memory is staged by the driver at a third of that.  For the arrays sr_trace / sr_rays_download fill
 * (the reference returns fresh NumPy arrays from ScalarDomain.solve, full_solver.py:391-400; engine.trace hands out
 * arrays over such blocks and returns them when the arrays are collected). */
int sr_host_alloc(void **out, size_t bytes);
void sr_host_free(void *p);
/* SYNTHRAY_ALLOC_FILL=<0..255>, a test knob read at every allocation: every device buffer of the library, the whole staging block
 * of the selected stream at every hand-out, and every block of sr_host_alloc is filled with that byte before it is used (unset or
 * empty: nothing is filled).  No result may depend on it.  sr_alloc_probe shows the knob at work: `bytes` of a fresh device buffer
 * and `bytes` of the selected stream's staging block, as they are handed out, copied to the caller (either may be NULL). */
int sr_alloc_probe(size_t bytes, unsigned char *from_alloc, unsigned char *from_scratch);
/* sr_trace on a large host bundle keeps its device-side working set (three chunk-sized ray bundles and two staging blocks,
 * ~1.5 GB of HBM at the default chunk) between calls, so that a loop of solve() calls does not allocate and release it
 * every time (trace_pipeline.hip).  This releases it (SYNTHRAY_TRACE_CACHE=0: never kept). */
int sr_release_caches(void);
const char *sr_last_error(void);
const char *sr_version(void);         /* "synthray <ver> (gfx950) src:<hash of the library's sources>" */

/* ---- A1 + A5: ScalarDomain.calc_dndr / n_refrac -------------------------------
 * replaces src/solvers-legacy/full_solver.py:211-234 (calc_dndr), :271-274 (n_refrac),
 *          src/simulator/propagator.py:63-91 (n_refrac, dndr's per-call np.gradient).
 * omega = 2*pi*c/lwl, n_c = 3.14207787e-4*omega^2, ne_nc = float32(ne/n_c),
 * dnd{x,y,z} = float32(-c^2/2) * np.gradient(ne_nc, coord, axis) in float32 exactly as
 * numpy evaluates it (non-uniform 2nd-order interior, 1st-order edges), and with
 * SR_VOL_PHASE the refractive index n = sqrt(1-(5.64e4*sqrt(ne*1e-6)/omega)^2) in float64.
 * ne: nx*ny*nz values, float64 (ne_is_f64 != 0) or float32.  probing_axis (0 x,1 y,2 z)
 * fixes the on-device layout (that axis is made the fastest one). */
#define SR_VOL_PHASE 1
int sr_volume_create(sr_volume **out, const void *ne, int ne_is_f64, int nx, int ny, int nz,
                     const float *x, const float *y, const float *z, double lwl,
                     int probing_axis, int flags);
/* same, from gradient volumes the caller already holds (float32, C-order) and an optional
 * float64 refractive index: the state calc_dndr leaves in ScalarDomain.dndx/dndy/dndz */
int sr_volume_create_from_fields(sr_volume **out, const float *dndx, const float *dndy,
                                 const float *dndz, const double *nref, double omega, int nx,
                                 int ny, int nz, const float *x, const float *y, const float *z,
                                 int probing_axis);
/* read the fields back in the reference's layout (any pointer may be NULL);
 * nref_minus_1 is n-1 in float64 */
int sr_volume_fields(const sr_volume *v, float *dndx, float *dndy, float *dndz, double *nref_minus_1);
/* A3/A4 at given points: the RegularGridInterpolator gathers of dsdt (full_solver.py:317-347, :538-541).
 * pts is (N, 3) [x, y, z]; out is (4, N): dndx, dndy, dndz, n-1 (0 where the volume has no phase field);
 * out-of-bounds points give the fill values (0, 0, 0, 0), NaN points give NaN. */
int sr_volume_sample(const sr_volume *v, const double *pts, int64_t n_pts, double *out);
/* The optional terms of dsdt: inverse-bremsstrahlung attenuation d(amp) = kappa(x)*amp (full_solver.py:334-339,
 * the field of ScalarDomain.kappa() :243-268) and Faraday rotation d(pol) = VerdetConst*ne(x)*(B(x).v)
 * (:356-374).  Replaces set_up_interps() (:276-289): float64 volumes in the reference's layout, kappa and ne
 * (nx, ny, nz), B (nx, ny, nz, 3); kappa may be NULL (inv_brems off), ne and B may both be NULL (B_on off).
 * Rays traced through a volume with these fields carry amp and pol (rows 6 and 8 of sf) through the same RK4
 * steps, in float64 throughout: the fields are held per ray as bilinear coefficient planes beside the gradient planes
 * (k_trace_f64<., AUX, .>); SR_PREC_MIXED asked for on such a volume runs the same float64 kernel. */
int sr_volume_attach_aux(sr_volume *v, const double *kappa, const double *ne, const double *B, double verdet);
/* the gathers of atten()/get_ne()/get_B() at given points: out is (5, N): kappa, ne, Bx, By, Bz (fill 0) */
int sr_volume_sample_aux(const sr_volume *v, const double *pts, int64_t n_pts, double *out);
/* A12 (the reference's region loop + back_propogate, propagator.py:300-349, 366-452; BASELINE config 5): the node
 * planes k_lo..k_hi of the probing axis as a volume of their own, for domains cut into slabs across GPUs.
 * nx, ny, nz, x, y, z describe the WHOLE domain; ne_slab holds the planes max(k_lo-1, 0)..min(k_hi+1, n-1) of the
 * probing axis (one halo plane each side for np.gradient's central difference; C order, that axis shortened), so the
 * slab's gradient values equal the whole domain's bit for bit.  Consecutive slabs share a node plane
 * (k_hi of one = k_lo of the next); rays go from slab to slab with SR_HANDOFF_* and the sr_rays_handoff_* calls. */
int sr_volume_create_slab(sr_volume **out, const void *ne_slab, int ne_is_f64, int nx, int ny, int nz,
                          const float *x, const float *y, const float *z, double lwl, int probing_axis,
                          int flags, int k_lo, int k_hi);
/* No reference counterpart: the line integrals of the volume along its probing axis, the thin-plasma predictions of what the
 * tracer integrates along the true path (d(phase) = omega (n-1), d(v) = dndr, d(amp) = kappa amp, d(pol) = V n_e (B.v)):
 *   phase = omega/c * NM1,  N_e = NE,  deflection = GRAD/c^2,  ln(amp) = KAPPA/c,  rotation = verdet * NEB.
 * maps is a HOST array (SR_PROJ_MAPS, n_u, n_v), float64, C order; (n_u, n_v) is the domain's shape with the probing axis
 * dropped -- for y-probing (nx, nz), although the device's lateral order there is (z, x).  Bit i of *have (may be NULL) says
 * that map i exists; an absent map is filled with 0.0.  The integral is the trapezoid rule on the volume's own float64 node
 * coordinates g of the probing axis, sum_k w_k f_k with w_0 = (g_1-g_0)/2, w_k = (g_{k+1}-g_{k-1})/2, w_{n-1} = (g_{n-1}-g_{n-2})/2;
 * a slab volume (sr_volume_create_slab) integrates its own planes k_lo..k_hi by the same rule, so the sum over the slabs of a
 * domain is the whole domain's integral.  A NaN node makes its column NaN and no other.  Each lane sums its plane of every
 * octet in float64 and a fixed tree adds the eight planes of a column (project.hip): no atomics, a repeated call returns the
 * identical bits.  Arguments are checked before the device is touched: NULL v or maps, a volume with fewer than 2 planes. */
#define SR_PROJ_GRAD1 0  /* integral of dnd_u dl: u, v = the two lateral axes in x<y<z order           */
#define SR_PROJ_GRAD2 1  /* integral of dnd_v dl                                                        */
#define SR_PROJ_NM1   2  /* integral of (n-1) dl, n-1 = hi + lo                  needs SR_VOL_PHASE     */
#define SR_PROJ_NE    3  /* integral of n_e dl, n_e = -m(2+m)*omega^2*1e6/5.64e4^2, m = n-1 (the n
                            formula of sr_volume_create inverted)                needs SR_VOL_PHASE     */
#define SR_PROJ_KAPPA 4  /* integral of kappa dl                                 needs attached kappa   */
#define SR_PROJ_NEB   5  /* integral of n_e*B_a dl, a = probing axis             needs attached ne, B   */
#define SR_PROJ_MAPS  6
int sr_volume_project(const sr_volume *v, double *maps, uint32_t *have);
double sr_volume_omega(const sr_volume *v);
int64_t sr_volume_bytes(const sr_volume *v); /* HBM held by the handle */
void sr_volume_destroy(sr_volume *v);

/* ---- oblique lines of sight: a field rotated onto a new grid ------------------------
 * No reference counterpart (its users turn the cube with scipy.ndimage before they build the domain).  sr_field is a scalar or
 * 3-vector field on a rectilinear grid, resident in HBM: data is (nx, ny, nz) or (nx, ny, nz, 3) (as B is), C order, float64
 * (is_f64 != 0) or float32; x, y, z are its float32 node coordinates.  sr_field_resample evaluates it, trilinearly, at the
 * nodes of a VIEW grid (mx, my, mz; float32 coordinates ox, oy, oz) whose node q sits at the lab position p = M q + t, and
 * writes out, a HOST array (mx, my, mz[, n_comp]) in C order and the source's dtype.  Every output node follows one rule
 * (resample.hip is compiled with -ffp-contract=off: every product and sum below rounds on its own, in float64):
 *   positions  the coordinates are widened to float64, q = (ox[i], oy[j], oz[k]), and
 *              p_a = ((M[a][0]*q0 + M[a][1]*q1) + M[a][2]*q2) + t[a]                          (M row-major).
 *   cell       per source axis with float64-widened nodes g[0..n-1]: the largest i with g[i] <= p, clipped to n-2 -- so
 *              p == g[n-1] lies in the last cell -- and w = (p - g[i]) / (g[i+1] - g[i]).  Axes may be non-uniform.
 *   outside    p < g[0] or p > g[n-1] on any axis (or a NaN p): the output is fill[c] for component c.
 *   blend      with u = 1 - w per axis, w00 = uy*uz, w01 = uy*wz, w10 = wy*uz, w11 = wy*wz and f(di, dj, dk) the corner
 *              values widened to float64, for di = 0, 1 (node plane i + di of x):
 *                  s_di = ((f(di,0,0)*w00 + f(di,0,1)*w01) + f(di,1,0)*w10) + f(di,1,1)*w11
 *              and the value is ux*s_0 + wx*s_1: the corner order of sr_volume_sample's gather (the four corners of a node
 *              plane, then the two planes), with (1 - w) and w as the factors -- weight 0 returns the low node and weight 1
 *              the high node exactly.  A float32 source is blended in float64 and rounded once on store.  A NaN corner
 *              makes NaN every output whose cell holds it, zero weights included, and no other output.
 *   vectors    n_comp == 3: the three components are interpolated as above, b = (b0, b1, b2); with use_V the output
 *              components are ((V[r][0]*b0 + V[r][1]*b1) + V[r][2]*b2), r = 0, 1, 2 (V row-major).
 * No atomics: a repeated call returns the identical bits.  *kernel_ms (may be NULL) is the HIP-event time of the kernel alone.
 * Arguments are checked before the device is touched -- sr_field_create: a NULL pointer, n_comp not 1 or 3, an axis with fewer
 * than 2 nodes or not strictly ascending; sr_field_resample: a NULL pointer, a view axis without nodes, a non-finite entry of
 * M, t or (with use_V) V. */
typedef struct sr_field sr_field;
int sr_field_create(sr_field **out, const void *data, int is_f64, int n_comp, int nx, int ny, int nz,
                    const float *x, const float *y, const float *z);
typedef struct {
  double M[9], t[3];     /* row-major; lab position of view node q:  p = M q + t                         */
  double V[9];           /* n_comp == 3 and use_V: out components = V * (interpolated components)        */
  double fill[3];        /* value per component where p lies outside the source grid on any axis         */
  int32_t use_V, reserved;
} sr_resample_params;
int sr_field_resample(const sr_field *f, const sr_resample_params *p, int mx, int my, int mz,
                      const float *ox, const float *oy, const float *oz, void *out, double *kernel_ms);
int64_t sr_field_bytes(const sr_field *f); /* HBM held by the handle */
void sr_field_destroy(sr_field *f);

/* ---- self-emission: emission with self-absorption along a grid axis -------------------
 * No reference counterpart.  The plasma's own light on a detector that looks along grid axis `axis`: per band (an angular
 * frequency omega; up to SR_MAX_BANDS in one pass) and per lateral column, the formal solution of dI/ds = alpha (S - I) from
 * the far plane to the plane nearest the detector.  ne [m^-3], Te [eV], Z are scalar sr_fields on ONE grid (the node
 * coordinates are compared bit for bit) and of one dtype; Te or Z may be NULL: the field is then the uniform value p->Te / p->Z
 * and is not read.  emission.hip is compiled with -ffp-contract=off: every operation below rounds on its own, in float64; max(a, b)
 * is numpy's maximum (a NaN operand gives NaN).
 *   node     ne, Te, Z are widened to float64.  Te <= 0 or ne <= 0: alpha = 0 and S = 0.  Otherwise, per band,
 *              n = ne*1e-6;  w = max(5.64e4*sqrt(n), omega);  q = sqrt(Te)
 *              L = max(Z*1.602176634e-19/Te, 2.760428269727312e-10/q)
 *              lnL = max(2.0, log(4.19e5*q / (w*L)));  r = n/omega
 *              alpha = (((((3.1e-5*Z)*c)*(r*r))*lnL) * (1.0/(Te*q))) / c           c = 299792458   [1/m]
 *            -- propagator.kappa(ne, Te, Z, omega) / c in its order of operations, Te**-1.5 written 1/(Te*sqrt(Te)): the NRL
 *            low-frequency (inverse-bremsstrahlung) coefficient the tracer uses, trustworthy for hbar*omega <~ Te -- and
 *              S = c_omega / expm1(e_ph / Te)
 *            the Planck function B_omega(Te): the host gives e_ph = hbar*omega/e [eV] and c_omega = hbar*omega^3/(4 pi^3 c^2)
 *            per band.  The emissivity alpha*S (Kirchhoff) is never formed.  A NaN input stays NaN.
 *   column   toward = +1 marches planes 0 -> n-1 (the direction the rays travel), toward = -1 the reverse.  Start from
 *            I = backlight (0 when NULL), tau = 0; for each cell between consecutive planes k, k' of the march, on the float64
 *            values g of the float32 node coordinates:
 *              h = |g[k'] - g[k]|;  dtau = (0.5*(alpha_k + alpha_k'))*h
 *              I <- I*exp(-dtau) + (0.5*(S_k + S_k'))*(-expm1(-dtau));   tau <- tau + dtau
 *            A cell's update is an affine map I -> I*a + b with a in [0, 1] and b >= 0, and composing two of them,
 *            (a1, b1) then (a2, b2) -> (a1*a2, b1*a2 + b2), is associative in exact arithmetic: the kernel may compose the
 *            cells of a column (and add their dtau) in any FIXED order.  No atomics: a repeated call returns identical bits.
 *            A NaN node makes its own column NaN and no other.
 * I, tau and backlight are HOST arrays (n_band, n_u, n_v), float64, C order; (u, v) are the lateral axes in x < y < z order, as
 * sr_volume_project lays its maps out.  *kernel_ms (may be NULL) is the HIP-event time of the kernel alone.
 * Arguments are checked before the device is touched: a NULL p, I or tau, n_band outside 1..SR_MAX_BANDS, a non-finite or
 * non-positive omega (or non-finite e_ph, c_omega), toward not +-1, axis outside 0..2, a NULL ne, a vector field, fields of
 * different dtypes, grids that differ. */
#define SR_MAX_BANDS 4
typedef struct {
  int32_t axis, toward, n_band, reserved;
  double omega[SR_MAX_BANDS];   /* angular frequency [rad/s]                                             */
  double e_ph[SR_MAX_BANDS];    /* hbar*omega/e [eV]                                                     */
  double c_omega[SR_MAX_BANDS]; /* hbar*omega^3/(4 pi^3 c^2) [W m^-2 sr^-1 (rad/s)^-1]                   */
  double Te, Z;                 /* the uniform field values where the handle is NULL                     */
} sr_emission_params;
int sr_field_emission(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_params *p,
                      const double *backlight, double *I, double *tau, double *kernel_ms);

/* ---- self-emission from tabulated opacities ----------------------------------------------
 * sr_field_emission with the node's absorption and emission taken from an opacity table over temperature x ion number density
 * (PROPACEOS tables, or anything laid out that way) instead of the NRL coefficient: the bands where bound-free and line opacity
 * dominate.  Fields, columns, outputs, units and layouts are sr_field_emission's; only the node differs.  float64 throughout,
 * every operation rounds on its own (emission_table.hip is compiled with -ffp-contract=off); max and min are numpy's (a NaN
 * operand gives NaN).
 *   host     the table arrives as logarithms, float64, C order: LT[i] = log(temperature i [eV]), LD[j] = log(ion number density j
 *            [cm^-3]), both strictly increasing, nT and nD nodes (2..512 each); per band b of p->n_band,
 *            LA[b][i][j] = log(absorption opacity [cm^2/g]) and LE[b][i][j] = log(emission opacity [cm^2/g]); LE may be NULL:
 *            LTE, emission opacity = absorption opacity.  p->e_ph[b] and p->c_omega[b] are sr_emission_params' (made from the
 *            angular frequency of the band's photon energy); p->omega is ignored.  m_ion = A * 1.66053906660e-24 [g].
 *   node     Te <= 0, ne <= 0 or Z <= 0: alpha = 0 and S = 0.  Otherwise
 *              ni = (ne*1e-6)/Z;  lt = log(Te);  ld = log(ni)
 *              i = the largest index with LT[i] <= lt, clamped to [0, nT-2];  ft = min(max((lt - LT[i])/(LT[i+1] - LT[i]), 0), 1)
 *              j, fd the same from LD and ld
 *            -- outside the table the edge value holds, there is no extrapolation -- and per band, on a table T (LA or LE),
 *              p0 = T[i][j] + fd*(T[i][j+1] - T[i][j]);  p1 = T[i+1][j] + fd*(T[i+1][j+1] - T[i+1][j]);  l(T) = p0 + ft*(p1 - p0)
 *              la = l(LA);  alpha = (exp(la)*(ni*m_ion))*100.0                                                       [1/m]
 *              S = exp(l(LE) - la) * (c_omega/expm1(e_ph/Te))            LE NULL: S = c_omega/expm1(e_ph/Te), LE is not read
 *            The interpolant is continuous across lattice nodes, so an lt within rounding of LT[i] may land in the cell on
 *            either side.  A NaN input stays NaN.
 *   column   sr_field_emission's, word for word: dtau = (0.5*(alpha_k + alpha_k'))*h,
 *            I <- I*exp(-dtau) + (0.5*(S_k + S_k'))*(-expm1(-dtau)), tau <- tau + dtau, composed in any FIXED order; toward = +-1;
 *            backlight, Te or Z may be NULL (0, or the uniform value p->Te / p->Z).  No atomics: a repeated call returns identical
 *            bits.  A NaN node makes its own column NaN and no other.
 * I is the spectral radiance per unit angular frequency at the band's photon energy [W m^-2 sr^-1 (rad/s)^-1].  Not modelled:
 * Z from the table's own ionisation (the solve ne = ni*zf(T, ni)), group-integrated Planck functions, refraction, detector optics.
 * Arguments are checked before the device is touched: everything sr_field_emission checks except omega, a NULL table or a NULL
 * LT, LD or LA, nT or nD outside 2..512, a lattice that is not finite or not strictly increasing, a non-finite table entry, an
 * m_ion that is not finite and positive. */
typedef struct {
  int32_t nT, nD;        /* lattice nodes: temperature, ion number density                              */
  const double *LT, *LD; /* log of the lattice [eV], [cm^-3]: nT, nD values                             */
  const double *LA, *LE; /* log opacities [cm^2/g], (n_band, nT, nD); LE NULL: LTE                      */
  double m_ion;          /* ion mass [g]                                                                */
} sr_emission_table;
int sr_field_emission_table(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_table *t,
                            const sr_emission_params *p, const double *backlight, double *I, double *tau, double *kernel_ms);

/* ---- sightlines: emission and absorption along arbitrary chords ---------------------------------
 * No reference counterpart.  The recurrence of sr_field_emission marched along n half-lines x(t) = o + d t, t >= 0, that need not
 * be parallel to a grid axis: the converging lines of a pinhole camera, the diverging ones of a point backlighter, single chords
 * of a diode or a spectrometer.  ne, Te, Z are sr_field_emission's fields (one grid, one dtype; a NULL Te or Z is the uniform value
 * p->Te / p->Z and is not read); table NULL: the node is sr_field_emission's (the NRL node), otherwise sr_field_emission_table's with
 * that table (p->omega is then ignored).  origin and dir are HOST arrays (3, n), float64, C order; dir need not be a unit vector.
 * Everything is float64 and every operation below rounds on its own (sightlines.hip is compiled with -ffp-contract=off); lo_a and
 * hi_a are the first and the last node coordinate of axis a, widened from float32.  Per line:
 *   clip     t0 = 0, t1 = +inf; for a = x, y, z in that order: d_a == 0: the line misses unless lo_a <= o_a <= hi_a; otherwise
 *              ta = (lo_a - o_a)/d_a;  tb = (hi_a - o_a)/d_a             (a division, not a reciprocal: 0*inf cannot arise)
 *              t0 = max(t0, min(ta, tb));  t1 = min(t1, max(ta, tb))
 *            and the line misses unless t1 > t0.  The origin may lie inside the box (t0 stays 0).
 *   miss     I = backlight (0 when NULL), tau = 0, column = 0, chord = 0, steps = 0.
 *   steps    len = sqrt((d0*d0 + d1*d1) + d2*d2);  chord = (t1 - t0)*len;  q = chord/step
 *              n = q >= max_steps ? max_steps : max(1, (int)ceil(q));  dt = (t1 - t0)/n;  h = chord/n
 *            (a q that is not below max_steps, NaN included, takes max_steps).
 *   march    start from I = backlight (0 when NULL), tau = 0, column = 0; visit the samples k = 0 .. n-1 in that order for
 *            toward = +1 (the light travels along +d, away from the origin: a backlighter) and k = n-1 .. 0 for toward = -1 (towards
 *            the origin: a pinhole).  Per sample
 *              t = t0 + (k + 0.5)*dt;  p_a = o_a + d_a*t
 *            ne, Te, Z at p follow sr_field_resample's `cell`, `outside` and `blend` lines word for word (the same corner order,
 *            u = 1 - w as the factors); the blended value of a float32 field stays float64.  A sample whose p lies outside the box
 *            on any axis -- possible only within rounding of a face -- is dark: alpha = S = 0, and its ne counts as 0.  Otherwise
 *            alpha and S per band are the node's, from the blended (ne, Te, Z), with the node's own dark conditions.  Then
 *              dtau = alpha*h;  I <- I*exp(-dtau) + S*(-expm1(-dtau));  tau <- tau + dtau;  column <- column + ne*h
 *            A NaN corner makes NaN the lines whose samples fall in its cell, zero weights included, and no other line.
 * No atomics: a repeated call returns identical bits.  I, tau and backlight are HOST arrays (n_band, n); column [m^-2, the integral
 * of ne dl], chord [m] and steps are HOST arrays (n) and may be NULL.  *kernel_ms (may be NULL) is the HIP-event time of the kernel.
 * Not modelled: a finite pinhole or source, the cos^4 and solid-angle factors between radiance and film exposure, refraction, the
 * detector's response, a table's own ionisation.
 * Arguments are checked before the device is touched: a NULL p, origin, dir, I or tau; n < 0 (n == 0 succeeds and writes nothing);
 * n_band, omega (table NULL), e_ph and c_omega as sr_field_emission checks them; toward not +-1; a step that is not finite and
 * positive; max_steps < 1; everything sr_field_emission_table checks of a table; a non-finite entry of origin or dir; a dir column
 * that is all zero; a NULL ne, a vector field, fields of different dtypes, grids that differ. */
typedef struct {
  int32_t toward;      /* +1: the light travels along +d (backlighter); -1: towards the origin (pinhole)    */
  int32_t n_band;      /* 1..SR_MAX_BANDS                                                                    */
  int32_t max_steps;   /* >= 1                                                                               */
  int32_t reserved;
  double step;         /* target sample spacing [m], finite, > 0                                            */
  double omega[SR_MAX_BANDS], e_ph[SR_MAX_BANDS], c_omega[SR_MAX_BANDS]; /* as sr_emission_params          */
  double Te, Z;        /* the uniform field values where the handle is NULL                                  */
} sr_sightline_params;
int sr_field_sightlines(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_table *table /* or NULL */,
                        const sr_sightline_params *p, int64_t n, const double *origin, const double *dir,
                        const double *backlight /* or NULL */, double *I, double *tau, double *column /* or NULL */,
                        double *chord /* or NULL */, int32_t *steps /* or NULL */, double *kernel_ms);

/* ---- sightline spectra: many frequencies along each chord ----------------------------------------
 * sr_field_sightlines for a spectrum: n_freq frequencies (1..SR_MAX_FREQS) along every line in one call -- a spectrometer chord's
 * continuum, the photon-energy groups of an opacity table, a filtered diode.  THE RULE IS sr_field_sightlines' (the section
 * above: clip, miss, steps, march, sample, gather, node, update, NaN behaviour, what is not modelled), with "per band" read as
 * "per frequency": for every line i and frequency f, I[i][f] and tau[i][f] are the same bits sr_field_sightlines returns for line
 * i with frequency f as one of its bands, and column, chord and steps are the same bits too (sightline_spectra.hip is compiled with
 * -ffp-contract=off from the same inline functions, and visits a line's samples in the same order per frequency).  The differences:
 *   frequencies  omega, e_ph and c_omega are HOST arrays (n_freq), as sr_emission_params' per band; with a table omega is ignored and
 *                may be NULL, and table->LA, table->LE are (n_freq, nT, nD): one band of the table per frequency.
 *   layout       I, tau and backlight are HOST arrays (n, n_freq), float64, C order: a line's spectrum is contiguous.
 *   params       sr_spectra_params carries toward, max_steps, step and the uniform Te, Z of sr_sightline_params.
 * Arguments are checked before the device is touched: everything sr_field_sightlines checks; a NULL e_ph or c_omega; a NULL omega
 * without a table; n_freq outside 1..SR_MAX_FREQS; an omega (table NULL) that is not finite and positive, a non-finite e_ph or
 * c_omega; a table whose packed size, or an n times the frequency tiles of a line, that does not fit the launch's 32-bit counts (an
 * error, not a cap).  n == 0 succeeds and writes nothing. */
#define SR_MAX_FREQS 16384
typedef struct {
  int32_t toward;      /* +1 | -1, as sr_sightline_params                                                    */
  int32_t max_steps;   /* >= 1                                                                               */
  double step;         /* target sample spacing [m], finite, > 0                                            */
  double Te, Z;        /* the uniform field values where the handle is NULL                                  */
} sr_spectra_params;
int sr_field_sightline_spectra(const sr_field *ne, const sr_field *Te, const sr_field *Z, const sr_emission_table *table /* or NULL */,
                               const sr_spectra_params *p, int64_t n, const double *origin, const double *dir, int32_t n_freq,
                               const double *omega, const double *e_ph, const double *c_omega,
                               const double *backlight /* (n, n_freq) or NULL */, double *I, double *tau /* (n, n_freq) */,
                               double *column, double *chord, int32_t *steps /* (n), may be NULL */, double *kernel_ms);

/* ---- line spectra along sightlines: Doppler-shifted, thermally broadened spectral lines ----------
 * No reference counterpart.  What a spectrometer chord reads: for every line of sight (below a CHORD; a LINE is a spectral line) and
 * every one of n_freq frequencies (1..SR_MAX_FREQS), the spectral radiance and the optical depth of n_line (1..SR_MAX_LINES)
 * Gaussian lines whose centre follows the flow along the chord and whose width follows the ion temperature, sample by sample,
 * optionally on top of the NRL continuum sr_field_sightline_spectra computes.  ne, Te, Z are sr_field_sightlines' fields (a NULL Te
 * or Z is the uniform p->Te / p->Z); Ti [eV] is a scalar field, NULL: Ti = Te; V [m/s] is a 3-vector field, NULL: no shift, nothing
 * of V is read and beta = 0.  All fields lie on ONE grid and have one dtype, checked as sr_field_thomson checks them.  Everything is
 * float64 and every operation below rounds on its own (sightline_lines.hip is compiled with -ffp-contract=off); sqrt and / are the
 * correctly rounded ones, exp, expm1 and log the device library's.
 *   table    sr_line_table: nT, nD, LT, LD are exactly sr_emission_table's lattice, ln Te [eV] and ln ni [cm^-3] with
 *            ni = (ne*1e-6)/Z, searched by the table section's rule (i, ft, j, fd; the edge value holds outside the table); w0[l] is
 *            the rest angular frequency [rad/s] and A[l] the mass number of the emitting ion of line l; LJ[l][i][j] = ln of the
 *            frequency-integrated emission coefficient [W m^-3 sr^-1]; LK[l][i][j] = ln of the frequency-integrated absorption
 *            coefficient [m^-1 rad s^-1], or LK NULL: optically thin lines, LK is never read and aK = 0.  l(T) is the table
 *            section's bilinear interpolant.
 *   chord    clip, miss, steps, the sample positions, the gather (Ti and the components of V by the same cell and weights) and the
 *            march order are sr_field_sightlines', word for word: column, chord and steps are the bits that entry returns.
 *   sample   with c = 299792458.0, e = 1.602176634e-19, m_p = 1.67262192369e-27, ISP = 0.5641895835477563 and, per line,
 *            ci_l = (2.0*e)/(A_l*m_p) (formed on the host):
 *              su = toward/len;  vpar = ((V0*d0 + V1*d1) + V2*d2)*su;  beta = vpar/c
 *            -- vpar is the flow's component along the direction the light travels; toward and len are sr_field_sightlines'.
 *            The sample is DARK FOR LINES when Te <= 0, ne <= 0 or Z <= 0 (the table section's dark node), when Ti <= 0, or when
 *            it lies outside the box.  Otherwise, per line l,
 *              wc = w0_l*(1.0 + beta);  wd = w0_l*(sqrt(ci_l*Ti)/c);  iw = 1.0/wd;  g = ISP*iw
 *              aJ = exp(l(LJ_l))*g;  aK = exp(l(LK_l))*g                                      (LK NULL: aK = 0)
 *   term     per sample and frequency f: j = 0, aL = 0, counted = false; for l ascending
 *              x = (omega_f - wc)*iw;  x2 = x*x;  the term is dropped when x2 > 40.0 (a NaN is not dropped); otherwise
 *              phi = exp(-x2);  j = j + aJ*phi;  aL = aL + aK*phi;  counted = true
 *            A dark sample counts nothing.  (ac, Sc) = the NRL node's alpha and S at omega_f (the self-emission section, with its own
 *            dark condition) when p->continuum != 0, otherwise 0, 0.
 *   update   not counted:  dtau = ac*h;  I <- I*exp(-dtau) + Sc*(-expm1(-dtau));  tau <- tau + dtau      (sr_field_sightlines')
 *            counted:      a = ac + aL;  dtau = a*h
 *              dtau == 0:  I <- I + j*h
 *              otherwise:  I <- I*exp(-dtau) + ((ac*Sc + j)/a)*(-expm1(-dtau));  tau <- tau + dtau   (dtau > 0, or a NaN)
 *            then column <- column + ne*h.  With the continuum off the first case is I <- I*1 + 0*0, tau <- tau + 0: the kernel
 *            writes I + 0.0 and tau + 0.0, the same bits.  Dropping is exact, so the kernel may skip a line for a whole wavefront
 *            whose frequencies all lie outside it: x and x2 are monotone in omega_f as rounded.
 * At a frequency where every term of a chord is dropped, I and tau are the bits of sr_field_sightline_spectra there (continuum on) or
 * the backlight and 0 (off).  The result for a frequency does not depend on the others or on their order.  A NaN Ti or V makes wc or
 * iw NaN, x2 NaN and the term counted: the chords through that cell are NaN at every frequency; a NaN ne poisons column, the
 * continuum, and the frequencies at which a term of that sample is counted.  No atomics: a repeated call returns identical bits.
 * I, tau and backlight are HOST arrays (n, n_freq) as sr_field_sightline_spectra's; omega, e_ph, c_omega (n_freq) as there, all three
 * always given.  I is the spectral radiance per unit angular frequency [W m^-2 sr^-1 (rad/s)^-1].  sr_lines_chunk() is the number of
 * samples the kernel stages at a time (for tests that place sample counts on its boundaries).
 * Not modelled: Lorentzian, Stark and Voigt wings; Zeeman splitting; line blending through the cutoff at exp(-40); partial
 * redistribution; refraction; the instrument function (the host applies it, as thomson.py does); one GPU only.
 * Arguments are checked before the device is touched: everything sr_field_sightline_spectra checks (omega always); a NULL line table
 * or a NULL LT, LD, w0, A or LJ; n_line outside 1..SR_MAX_LINES; nT or nD outside 2..512; a w0 or an A that is not finite and
 * positive; a lattice that is not finite or not strictly increasing; a non-finite LJ or LK entry; a Ti with n_comp != 1 or a V with
 * n_comp != 3, or of another dtype or grid.  n == 0 or n_freq == 0 succeeds and writes nothing. */
#define SR_MAX_LINES 32
typedef struct {
  int32_t nT, nD;        /* lattice nodes, as sr_emission_table                                           */
  int32_t n_line;        /* 1..SR_MAX_LINES                                                               */
  int32_t reserved;
  const double *LT, *LD; /* log of the lattice [eV], [cm^-3]: nT, nD values                               */
  const double *w0, *A;  /* rest angular frequency [rad/s], mass number of the emitter: n_line values     */
  const double *LJ, *LK; /* (n_line, nT, nD): log emission [W m^-3 sr^-1], log absorption or NULL (thin)  */
} sr_line_table;
typedef struct {
  int32_t toward;      /* +1 | -1, as sr_sightline_params                                                    */
  int32_t max_steps;   /* >= 1                                                                               */
  int32_t continuum;   /* != 0: the lines sit on the NRL continuum                                           */
  int32_t reserved;
  double step;         /* target sample spacing [m], finite, > 0                                            */
  double Te, Z;        /* the uniform field values where the handle is NULL                                  */
} sr_lines_params;
int sr_lines_chunk(void);
int sr_field_sightline_lines(const sr_field *ne, const sr_field *Te, const sr_field *Ti /* or NULL */, const sr_field *Z,
                             const sr_field *V /* or NULL */, const sr_line_table *lines, const sr_lines_params *p, int64_t n,
                             const double *origin, const double *dir, int32_t n_freq, const double *omega, const double *e_ph,
                             const double *c_omega, const double *backlight /* (n, n_freq) or NULL */, double *I,
                             double *tau /* (n, n_freq) */, double *column, double *chord, int32_t *steps /* (n), may be NULL */,
                             double *kernel_ms);

/* ---- Voigt lines along sightlines: Stark and Lorentz wings on the Doppler-shifted lines ----------
 * No reference counterpart.  sr_field_sightline_lines with a Lorentzian half-width per line from the table, so that every line is a
 * Voigt profile -- what a Stark-broadened line of a dense plasma looks like, and what an electron density is read from.  Wherever
 * nothing is said here the rule is sr_field_sightline_lines', word for word: the chord, the clip, the samples, the gather, the dark
 * conditions, beta, wc, wd, iw, g, aJ, aK, the continuum, the update, column, chord and steps.  Everything is float64 and every
 * operation rounds on its own (sightline_voigt.hip is compiled with -ffp-contract=off); exp, sin, cos and rint are the device
 * library's.
 *   table    sr_voigt_table: `lines` is that entry's table; LG[l][i][j] = ln of the Lorentzian half width at half maximum of line l
 *            [rad/s] on the same lattice, finite.
 *   sample   per line l of a sample that is not dark:  gam = exp(l(LG_l));  a = gam*iw, with l(.) the table section's bilinear
 *            interpolant at the same (i, ft, j, fd).
 *   term     cut = wing*wing, formed once on the host (wing = p->wing > 0 in Doppler 1/e widths, +inf allowed).  Per sample and
 *            frequency f, for l ascending:
 *              x = (omega_f - wc)*iw;  x2 = x*x;  the term is dropped when x2 > cut (a NaN is not dropped); otherwise
 *              phi = V(a, x);  j = j + aJ*phi;  aL = aL + aK*phi;  counted = true
 *   V(a, x)  the Voigt function H(a, x) = Re w(x + i a), w the Faddeeva function, normalised so that H(0, x) = exp(-x^2): with
 *            aJ = exp(l(LJ))*ISP*iw the line integrates to exp(l(LJ)) over omega, exactly as the Gaussian does.  With
 *            z2 = x*x + a*a the regions are tested in this order:
 *              not z2 < 1e17 (a NaN or an infinity too):   V = (ISP*a)/z2
 *              z2 >= 100.0:                                V = CF(10)
 *              a >= 2.0:                                   V = CF(40)
 *              a <= 0.5:                                   V = R(0.25, 2.0, 0.5, CA, 13)
 *              otherwise (0.5 < a < 2):                    V = R(0.1875, 2.6666666666666665, 0.375, CB, 18)
 *            CF(K), Laplace's continued fraction of w(z) truncated at K levels, as one rational function:
 *              Nr = x;  Ni = a;  Dr = 1;  Di = 0;  for k = K, K-1, ..., 1 in this order, with c = 0.5*k:
 *                  tr = (Nr*x - Ni*a) - c*Dr;   ti = (Nr*a + Ni*x) - c*Di;   Dr = Nr;  Di = Ni;  Nr = tr;  Ni = ti
 *              V = (ISP*(Dr*Ni - Di*Nr))/(Nr*Nr + Ni*Ni)
 *            -- t_K = z, t_(k-1) = z - (k/2)/t_k as t = N/D, w = (i/sqrt(pi))/t_0 = (i/sqrt(pi)) D/N.
 *            R(h, ih2, h2, C, NP), Rybicki's sampling form of Dawson's function (the Thomson section's D) at z = x + i a:
 *              n0 = 2.0*rint(ih2*x);  xp = x - h*n0;  a2 = a*a;  g = exp(a2 - xp*xp);  th = (2.0*a)*xp
 *              Gr = g*cos(th);  Gi = -(g*sin(th));  pe = exp(h2*xp);  me = 1.0/pe;  ca = cos(h2*a);  sa = sin(h2*a)
 *              pr = pe*ca;  pi = pe*sa;  mr = me*ca;  mi = -(me*sa)
 *              p2r = pr*pr - pi*pi;  p2i = (2.0*pr)*pi;  m2r = mr*mr - mi*mi;  m2i = (2.0*mr)*mi
 *              d0 = n0*n0;  Sr = 0;  Si = 0;  for k = 0, 1, ..., NP-1 in this order, with n = 2k + 1:
 *                  q = C[k]/(d0 - n*n)
 *                  Sr = Sr + q*(pr*(n0 - n) + mr*(n0 + n));   Si = Si + q*(pi*(n0 - n) + mi*(n0 + n))
 *                  (pr, pi) = (pr*p2r - pi*p2i, pr*p2i + pi*p2r);   (mr, mi) = (mr*m2r - mi*m2i, mr*m2i + mi*m2r)
 *              imF = (Gr*Si + Gi*Sr)*ISP;   V = exp(a2 - x*x)*cos((2.0*a)*x) - (2.0*ISP)*imF
 *            -- H = Re e^(-z^2) - (2/sqrt(pi)) Im F(z), F(z) = (1/sqrt(pi)) e^(-z'^2) sum_(n odd) C_n e^(2 h n z')/(n0 + n) with
 *            z' = z - h n0; the terms n and -n over one denominator, the powers of e^(2 h z') by complex multiplication.
 *            CA[k] = exp(-((2k+1)/4)^2) is the Thomson section's C[n]; CB[k] = exp(-(3(2k+1)/16)^2): 0.9654545521978378,
 *            0.7287633299194912, 0.4152368286818413, 0.17859113461243561, 0.0579800525002544, 0.014208622931196246,
 *            0.002628330960567707, 0.0003669972327972938, 3.8681223753184774e-05, 3.0774591584232196e-06, 1.8481578772048032e-07,
 *            8.378003053124454e-09, 2.866794996873118e-10, 7.404699497933558e-12, 1.4436865682659833e-13, 2.1246777523216493e-15,
 *            2.3603037795421644e-17, 1.9792352186549065e-19.  The step 3/16 keeps the sampling form's aliasing term,
 *            exp(-(pi/(2h))^2 + pi*a/h), under 1.2e-16 up to a = 2 (with h = 1/4 it is 4e-15 at a = 0.5 and 6e-7 at a = 2).
 *            Accuracy, measured against the real part of scipy.special.wofz on a in {1e-10, ..., 1e7} x x in [0, 1e7] with points
 *            a hair on either side of every boundary above (tests/test_sightline_voigt.py states the grid): the worst error
 *            RELATIVE TO H ITSELF is 1.6e-13, at a just under 2 where exp(a2) = 55 is cancelled; elsewhere 7e-14 or less.  The only
 *            absolute floor is the continued fractions': they drop the Gaussian core Re e^(-z^2), at most exp(a2 - x*x) <=
 *            exp(-(z2 - 2 a2)).  In CF(10)'s region that is exp(-100) = 3.7e-44 for a -> 0 against H >= ISP*a/z2 = 5.6e-13 at
 *            a = 1e-10, z2 = 100 (6.6e-32 of H, and less for every larger a of the grid up to a = 5, beyond which CF(40)'s bound
 *            holds); in CF(40)'s region a >= 2 and the core is exp(a2 - x*x)|cos| against H ~ ISP/a: it is part of what the 40
 *            levels converge to, not dropped.  ISP*a/z2 errs by 1/(2 z2) <= 5e-18.
 *   wing     dropping is exact for the reason it is in the line section: x and x2 are monotone in omega_f as rounded, so a
 *            wavefront may skip a line whose window [-wing, wing] holds none of its frequencies (that section's test of the two
 *            ends, against cut).  With wing = +inf nothing is ever dropped or skipped.  Where every term of a chord is dropped, I and
 *            tau are the bits of sr_field_sightline_spectra (continuum on) or the backlight and 0 (off).
 *   LG NULL  Gaussian lines: the entry computes sr_field_sightline_lines' rule with its cut at 40 and returns that entry's bits in
 *            I, tau, column, chord and steps; wing is not read.
 * NaN, poisoning and repeatability are the line section's: a NaN a or x gives a NaN term that is counted; no atomics; a repeated
 * call returns identical bits.  sr_voigt_chunk() is the number of samples this kernel stages at a time.
 * Not modelled: Zeeman splitting; asymmetric and shifted Stark profiles (a line's Stark shift can go into w0 only as a constant);
 * ion-dynamics corrections; blending through wing; partial redistribution; refraction; the instrument function; one GPU only.
 * Arguments are checked before the device is touched: everything sr_field_sightline_lines checks; a non-finite LG entry; a wing
 * that is NaN or <= 0 (where LG is given). */
typedef struct {
  sr_line_table lines;
  const double *LG; /* (n_line, nT, nD): ln of the Lorentzian HWHM [rad/s], finite; or NULL: Gaussian lines */
} sr_voigt_table;
typedef struct {
  sr_lines_params march;
  double wing;      /* > 0, may be +inf; in Doppler 1/e widths: a term with |x| > wing is dropped */
} sr_voigt_params;
int sr_voigt_chunk(void);
int sr_field_sightline_voigt(const sr_field *ne, const sr_field *Te, const sr_field *Ti /* or NULL */, const sr_field *Z,
                             const sr_field *V /* or NULL */, const sr_voigt_table *lines, const sr_voigt_params *p, int64_t n,
                             const double *origin, const double *dir, int32_t n_freq, const double *omega, const double *e_ph,
                             const double *c_omega, const double *backlight /* (n, n_freq) or NULL */, double *I,
                             double *tau /* (n, n_freq) */, double *column, double *chord, int32_t *steps /* (n), may be NULL */,
                             double *kernel_ms);

/* ---- Zeeman-split lines along sightlines: Stokes I, Q, U, V of lines in a magnetic field ----------
 * No reference counterpart.  sr_field_sightline_voigt with every line split by the magnetic field B [T] of the sample into its
 * Zeeman components (the weak-field, LS-coupling pattern the table gives), and four Stokes parameters marched along the chord
 * instead of one intensity -- what a polarisation-resolved spectrometer reads of a magnetised plasma.  Wherever nothing is said
 * here the rule is sr_field_sightline_voigt's, word for word: the chord, the clip, the samples, the gather, the dark conditions,
 * beta, wc, wd, iw, g, aJ, aK, gam, a, V(a, x), cut = wing*wing, the continuum, column, chord and steps.  Everything is float64
 * and every operation rounds on its own (sightline_zeeman.hip is compiled with -ffp-contract=off); exp, expm1, sqrt are the
 * device library's.  There is no trigonometry anywhere in what this section adds.
 *   table    sr_zeeman_table: `voigt` is that entry's table; n_comp[l] in 1..SR_MAX_ZEEMAN (24: every pattern up to
 *            J = 7/2 <-> 7/2, whose three groups hold 7 + 8 + 7 = 22) is the number of components of line l, and comp holds, line
 *            after line, (q, g, s) per component: q in {-1, 0, +1} is m_upper - m_lower, g the component's shift in units of the
 *            Larmor frequency (finite), s > 0 its strength relative to its q group.  The strengths of every q group that is
 *            present sum to 1 within 1e-9 (the sum taken in the table's order), checked on the host.  voigt.LG NULL here means
 *            a = 0 for every line -- Gaussian components through the same V(a, x) -- and does NOT delegate.
 *   frame    per chord, on the host, in float64, once (ref is (3, n), one reference direction per chord, any length):
 *              su = toward/sqrt((d0*d0 + d1*d1) + d2*d2);   nk = dk*su  (k = 0, 1, 2): n^ is the direction the light travels
 *              p = (r0*n0 + r1*n1) + r2*n2;   tk = rk - p*nk;   t = sqrt((t0*t0 + t1*t1) + t2*t2);   e1k = tk/t
 *              e2 = n^ x e1 = (n1*e12 - n2*e11, n2*e10 - n0*e12, n0*e11 - n1*e10)
 *            A ref with a non-finite component, or with not t > 1e-6*sqrt((r0*r0 + r1*r1) + r2*r2) (parallel to the chord within
 *            1e-6 rad, or zero), is an argument error.
 *   sample   B is gathered with the same cell and weights as the other fields (each component as V's: a (nx, ny, nz, 3) field);
 *            outside the box (within rounding of a face) B = 0 beside ne = 0.  With kL = e/(2.0*m_e), formed on the host from
 *            e = 1.602176634e-19 and m_e = 9.1093837015e-31:
 *              Bn = (B0*n0 + B1*n1) + B2*n2;   Bu = (B0*e10 + B1*e11) + B2*e12;   Bv = (B0*e20 + B1*e21) + B2*e22
 *              T = Bu*Bu + Bv*Bv;   B2 = T + Bn*Bn
 *              B2 == 0:   wL = 0;  sP = 1;  cS = 0.5;  cQ = cU = cV = 0
 *              otherwise (B2 > 0 or a NaN):   r = sqrt(B2);  wL = kL*r;  sP = T/B2;  cS = 0.5*(1.0 + (Bn*Bn)/B2)
 *                                             cQ = (Bu*Bu - Bv*Bv)/B2;  cU = ((2.0*Bu)*Bv)/B2;  cV = Bn/r
 *            sP is sin^2 of the angle between B and the light, cS = (1 + cos^2)/2, (cQ, cU) = sin^2 (cos 2chi, sin 2chi) with chi
 *            the azimuth of B's transverse part from e1, cV = cos.  The dark conditions are the line section's: B plays no part
 *            in them, and a NaN B is not dark: it poisons every frequency of the sample.
 *   term     per sample that is not dark and frequency f, for lines l ascending and, within a line, components k ascending:
 *              sh = g_k*wL;   x = ((omega_f - wc) - sh)*iw;   the term is dropped when x*x > cut (a NaN is not dropped); otherwise
 *              P_q = P_q + s_k*V(a, x)  (q = q_k; P0, Pp, Pm start at 0 for every line);   the line has a term
 *            and after the components of a line that has a term (a line all of whose components were dropped adds nothing):
 *              Ps = Pp + Pm;   eI = 0.5*(sP*P0) + (0.5*cS)*Ps;   eP = 0.5*(P0 - 0.5*Ps);   eV = 0.5*(Pp - Pm)
 *              jI = jI + aJ*eI;   jQ = jQ + aJ*(eP*cQ);   jU = jU + aJ*(eP*cU);   jV = jV + aJ*(eV*cV);   aL = aL + aK*eI
 *              counted = true
 *            Over omega every q group integrates to 1/ISP/iw, so the line's jI integrates to exp(l(LJ))*0.5*(sP + 2 cS) =
 *            exp(l(LJ)) at any angle, and jQ, jU, jV to 0.
 *   signs    A component with q = +1 (m_upper - m_lower = +1) emitted along +B has positive helicity, and Vs > 0 there: with B
 *            along the light (cV = +1) the q = +1 components give Vs = +I.  Q > 0 is linear polarisation along e1, U > 0 along
 *            the bisector of e1 and e2: seen across B (B along e1) the pi components are polarised along B, Q = +I, the sigma
 *            components across it, Q = -I.
 *   update   the line section's, on four parameters with ONE scalar attenuation.  Counted:  a = ac + aL;  dtau = a*h;
 *              dtau == 0:   I = I + jI*h;  Q = Q + jQ*h;  U = U + jU*h;  Vs = Vs + jV*h
 *              otherwise:   E = exp(-dtau);  F = -expm1(-dtau);  I = I*E + ((ac*Sc + jI)/a)*F;  Q = Q*E + (jQ/a)*F;
 *                           U = U*E + (jU/a)*F;  Vs = Vs*E + (jV/a)*F;  tau = tau + dtau
 *            Not counted, continuum on:  dtau = ac*h;  E = exp(-dtau);  I = I*E + Sc*(-expm1(-dtau));  Q = Q*E;  U = U*E;
 *            Vs = Vs*E;  tau = tau + dtau.  Not counted, continuum off:  each of the five + 0.0.  The backlight is unpolarised: I
 *            starts at it (or 0), Q = U = Vs = tau = 0.  The cone I*I >= Q*Q + U*U + Vs*Vs is closed under this update: the
 *            emitted (jI, jQ, jU, jV) lies in it line by line, the continuum adds to I alone, and all four decay alike.
 *   wing     dropping is exact and x stays monotone in omega_f as rounded (two subtractions and a product by iw >= 0), so a
 *            wavefront may skip a component whose window holds none of its frequencies: that section's test of the two ends with
 *            x as above.
 *   B NULL   the entry is sr_field_sightline_voigt: it returns that entry's bits in I, tau, column, chord and steps and exact
 *            zeros in those of Q, U, Vs that are not NULL; n_comp, comp and ref are not read.
 * A chord that misses the box: I = the backlight (or 0), Q = U = Vs = tau = 0.  NaN, poisoning and repeatability are the line
 * section's; no atomics; a repeated call returns identical bits.  sr_zeeman_chunk() is the number of samples this kernel stages at
 * a time.
 * Not modelled: dichroism and magneto-optical (anomalous-dispersion) rotation in the absorption matrix -- absorption acts equally
 * on all four parameters; Faraday rotation of the continuum (sr_field_sightline_stokes has all three); the Paschen-Back regime and
 * hyperfine structure; and what sr_field_sightline_voigt does not model.
 * Arguments are checked before the device is touched: everything sr_field_sightline_voigt checks (wing also where LG is NULL); with
 * B given a NULL table, n_comp, comp, ref, Q, U or Vs; an n_comp outside 1..SR_MAX_ZEEMAN; a q that is not -1, 0 or +1; a
 * non-finite g; an s that is not finite and positive; a q group whose strengths do not sum to 1; a ref as above; a B that is not a
 * 3-vector field on ne's grid and of its dtype.  n == 0 or n_freq == 0 succeeds after the checks and writes nothing. */
#define SR_MAX_ZEEMAN 24
typedef struct {
  sr_voigt_table voigt;
  const int32_t *n_comp; /* (n_line): components of each line, 1..SR_MAX_ZEEMAN */
  const double *comp;    /* (sum of n_comp, 3): q, g, s of every component, line after line */
} sr_zeeman_table;
int sr_zeeman_chunk(void);
int sr_field_sightline_zeeman(const sr_field *ne, const sr_field *Te, const sr_field *Ti /* or NULL */, const sr_field *Z,
                              const sr_field *V /* or NULL */, const sr_field *B /* or NULL: sr_field_sightline_voigt */,
                              const sr_zeeman_table *lines, const sr_voigt_params *p, int64_t n, const double *origin,
                              const double *dir, const double *ref /* (3, n) */, int32_t n_freq, const double *omega,
                              const double *e_ph, const double *c_omega, const double *backlight /* (n, n_freq) or NULL */,
                              double *I, double *Q, double *U, double *Vs, double *tau /* (n, n_freq) */, double *column,
                              double *chord, int32_t *steps /* (n), may be NULL */, double *kernel_ms);

/* ---- Polarised transfer along sightlines: dichroism, magneto-optical and Faraday rotation ----------
 * No reference counterpart.  sr_field_sightline_zeeman with the whole 4 x 4 absorption matrix of the polarised transfer equation in
 * place of its one scalar attenuation, and a backlight that may be polarised -- what a polarisation-resolved spectrometer reads of
 * a backlit or optically thick magnetised plasma.  Wherever nothing is said here the rule is sr_field_sightline_zeeman's, word for
 * word: the chord, the frame, the samples, the gather, the dark conditions, zeeman_sample (Bn, Bu, Bv, wL, sP, cS, cQ, cU, cV), the
 * component loop, x, cut = wing*wing, the wavefront skip, the continuum, column, chord and steps.  Everything is float64 and every
 * operation rounds on its own (sightline_stokes.hip is compiled with -ffp-contract=off); exp, expm1, sqrt, sin, cos and rint are
 * the device library's.
 *   profiles  (H, L) = W(a, x): H = Re w(x + i a) is V(a, x) of the Voigt section, the same operations and bits; L = Im w(x + i a),
 *             the dispersion (Faraday-Voigt) profile, comes from the same intermediates, region by region:
 *               not z2 < 1e17:   L = (ISP*x)/z2
 *               CF(K):           L = (ISP*(Dr*Nr + Di*Ni))/(Nr*Nr + Ni*Ni)
 *               R(...):          reF = (Gr*Sr - Gi*Si)*ISP;   L = (2.0*ISP)*reF - exp(a2 - x*x)*sin((2.0*a)*x)
 *             -- w = (i/sqrt(pi)) D/N, and w = e^(-z^2) + (2i/sqrt(pi)) F(z).  L is odd in x and cancels at the centre, so its
 *             accuracy is stated relative to |w| = sqrt(H*H + L*L): measured against scipy.special.wofz on the Voigt section's grid
 *             with both signs of x (tests/test_sightline_stokes.py), the worst error of L relative to |w| is 1.6e-13, at a just
 *             under 2 as H's is.
 *   term      per line, R0, Rp, Rm start at 0 beside P0, Pp, Pm, and a term that is not dropped adds to both:
 *               (H, L) = W(a, x);   P_q = P_q + s_k*H;   R_q = R_q + s_k*L
 *             A term is dropped, and a component skipped by a wavefront, for both profiles together.  After the components of a
 *             line that has a term, with Ps, eI, eP, eV the Zeeman section's:
 *               Rs = Rp + Rm;   fP = 0.5*(R0 - 0.5*Rs);   fV = 0.5*(Rp - Rm)
 *               jI, jQ, jU, jV:  the Zeeman section's four sums, with aJ;     hI = hI + aK*eI  (that section's aL)
 *               hQ = hQ + aK*(eP*cQ);   hU = hU + aK*(eP*cU);   hV = hV + aK*(eV*cV)
 *               rQ = rQ + aK*(fP*cQ);   rU = rU + aK*(fP*cU);   rV = rV + aK*(fV*cV);   counted = true
 *             All eleven start at 0 for every sample and frequency.
 *   faraday   with faraday = 1, for every sample (dark or not, counted or not), after the lines:
 *               rV = rV + ((kF2*(neh/h))*Bn)/(omega_f*omega_f)
 *             neh = ne*h is the sample's staged column (the number `column` sums), h the chord's sample length, Bn zeeman_sample's
 *             (B0*n0 + B1*n1) + B2*n2 -- B . n^ itself, 0 outside the box, not |B|*cV -- and kF2 = 2.0*kF,
 *             kF = ((e*e)*e)/((((2.0*eps0)*m_e)*m_e)*c) = e^3/(2 eps0 m_e^2 c), formed on the host from the Zeeman section's e and
 *             m_e, eps0 = 8.8541878128e-12 and c = 299792458.0: the plane of polarisation turns by kF*ne*(B . n^)*s/omega^2, the
 *             cold-plasma Faraday rotation for omega far above the plasma and cyclotron frequencies.
 *   matrix    eI = ac + hI;   eps = (ac*Sc + jI, jQ, jU, jV);
 *               K = [[eI, hQ, hU, hV], [hQ, eI, rV, -rU], [hU, -rV, eI, rQ], [hV, rU, -rQ, eI]]
 *             and dX/ds = -K X + eps for X = (I, Q, U, Vs).
 *   signs     This layout means d(Q + iU)/ds = i*rV*(Q + iU): the plane of polarisation turns from e1 towards e2 = n^ x e1 by
 *             rV*s/2.  (a) Free electrons with B along the light's travel turn the plane from e1 towards e2: the circular mode
 *             whose field turns in the electrons' sense about B (e1 -> e2 in time, positive helicity, Vs > 0) has the smaller
 *             refractive index, n^2 = 1 - wp^2/(omega*(omega + wc)) against 1 - wp^2/(omega*(omega - wc)), so it is the faster
 *             one, and the sum of two counter-rotating fields points along half the difference of their phases, (k_- - k_+) s/2
 *             > 0.  Hence the + of the faraday term.  (b) A normal triplet far to the blue of its centre is a classical bound
 *             electron and turns the plane as (a) does for the same B: with B along the light (cV = +1) the q = +1, g = +1
 *             component is the one of positive helicity, shifted to the blue, so at omega above both x_(+1) < x_(-1), and
 *             L ~ ISP/x gives Rp > Rm: the refractive index of the positive-helicity mode deviates from 1 by -(const)*Rp, the
 *             greater deviation, so it is the faster one, as in (a), and rV must be positive: rV = +aK*(0.5*(Rp - Rm)*cV).  The
 *             overall sign of rQ, rU, rV is therefore +1.  (c) hQ, hU, hV carry the signs of jQ, jU, jV.
 *   update    A sample and frequency whose six numbers hQ, hU, hV, rQ, rU, rV are all == 0.0 (a -0.0 is; a NaN is not) takes
 *             sr_field_sightline_zeeman's update, the same operations, with aL = hI, including its two not-counted branches.
 *             Otherwise, counted or not, the exact solution for coefficients constant over the sample, X <- O X + p with
 *             O = exp(-K h) and p = (integral_0^h exp(-K s) ds) eps, by scaling and squaring with +, -, *, / alone:
 *               r_i = ((|K_i0| + |K_i1|) + |K_i2|) + |K_i3|  (K's entries in the layout above);   nrm = the greatest r_i
 *               t = nrm*h;  hs = h;  s = 0;   while t > 0.25:  t = 0.5*t;  hs = 0.5*hs;  s = s + 1
 *                 (theta = 1/4; a t that is NaN or infinite takes s = 0, and all five come out NaN)
 *               g0 = -(eI*hs);  gQ = -(hQ*hs);  gU = -(hU*hs);  gV = -(hV*hs);  fQ = -(rQ*hs);  fU = -(rU*hs);  fV = -(rV*hs)
 *               b = ((ac*Sc + jI)*hs, jQ*hs, jU*hs, jV*hs);   O = the 4 x 4 identity;   p = (0, 0, 0, 0)
 *               for k = 13, 12, ..., 1 in this order (Horner, order 13), with c = (double)k:
 *                 A = [[g0/c, gQ/c, gU/c, gV/c], [gQ/c, g0/c, fV/c, -(fU/c)], [gU/c, -(fV/c), g0/c, fQ/c], [gV/c, fU/c, -(fQ/c), g0/c]]
 *                 N_ij = ((A_i0*O_0j + A_i1*O_1j) + A_i2*O_2j) + A_i3*O_3j
 *                 q_i = (((A_i0*p_0 + A_i1*p_1) + A_i2*p_2) + A_i3*p_3) + b_i/c
 *                 O = N with 1.0 + N_ii on the diagonal;   p = q
 *               s times:   q_i = p_i + (((O_i0*p_0 + O_i1*p_1) + O_i2*p_2) + O_i3*p_3)
 *                          N_ij = ((O_i0*O_0j + O_i1*O_1j) + O_i2*O_2j) + O_i3*O_3j;   p = q;   O = N
 *               X_i = (((O_i0*I + O_i1*Q) + O_i2*U) + O_i3*Vs) + p_i  (i = I, Q, U, Vs; from the old four);   tau = tau + eI*h
 *             -- the Taylor sum of exp of the 5 x 5 matrix [[-K hs, eps hs], [0, 0]], whose blocks are O and p.  With
 *             theta = 1/4 and order 13 the truncation is theta^14/14! = 4.3e-20, under u/4 = 2.8e-17.  The closed form in the
 *             eigenvalues of K is not used: it is singular where |eta| = |rho| with eta . rho = 0, and K^-1 eps loses everything
 *             where a sigma component is completely polarised (K singular to rounding).  Errors of this scheme against a
 *             50-digit matrix exponential, relative to the larger of the norms of X and p, measured on the grid of
 *             tests/test_sightline_stokes.py (eI*h from 1e-6 to 1e3, complete dichroism, |rho| up to 30 eI, the degenerate
 *             case): at most 2.9 u where s = 0, and (4 + 2*s + 4.2*nrm*h) u everywhere -- the last term is set by modes that
 *             do not decay and is the conditioning of exp itself, which the scalar rule has through the rounding of dtau; it
 *             grows with nrm*h because every squaring doubles the error of the scaled step.  The symmetric part of K has the eigenvalues eI +- |(hQ, hU, hV)| >= 0, so the update is a
 *             contraction in the 2-norm and the cone I*I >= Q*Q + U*U + Vs*Vs is kept up to rounding.
 *   backlight pol: (3) or NULL, (q, u, v) with q*q + u*u + v*v <= 1 (up to 1 + 1e-12: a unit vector as rounded).  The march
 *             starts at I = I0, Q = I0*q, U = I0*u, Vs = I0*v with I0 the backlight (or 0); NULL: Q = U = Vs = 0, unpolarised.  A
 *             chord that misses the box returns this start and tau = 0.
 *   zeeman    So with the table's LK NULL (aK = 0) and faraday = 0 every sample takes the scalar update, and with pol NULL the
 *             entry returns sr_field_sightline_zeeman's bits in I, Q, U, Vs, tau (and column, chord, steps).
 *   B NULL    the entry is sr_field_sightline_voigt, as sr_field_sightline_zeeman is: its bits in I, tau, column, chord and
 *             steps, exact zeros in those of Q, U, Vs that are not NULL; faraday = 1 or a pol is then an argument error.
 * NaN, poisoning and repeatability are the Zeeman section's: a NaN B is not dark and poisons every frequency of its sample (on
 * either update); no atomics; a repeated call returns identical bits.  sr_stokes_chunk() is the number of samples this kernel
 * stages at a time (a staged sample holds one word more than the Zeeman kernel's, B . n^, and one of padding).
 * Not modelled: the Paschen-Back regime; hyperfine structure; cyclotron dichroism of the continuum (the continuum absorbs all four
 * parameters alike and only rotates); scattering polarisation; the Hanle effect; and what sr_field_sightline_voigt does not model.
 * Arguments are checked before the device is touched: a faraday that is not 0 or 1; a pol that is not finite or lies outside the
 * unit ball; faraday = 1 or a pol with B NULL; then everything sr_field_sightline_zeeman checks. */
int sr_stokes_chunk(void);
int sr_field_sightline_stokes(const sr_field *ne, const sr_field *Te, const sr_field *Ti /* or NULL */, const sr_field *Z,
                              const sr_field *V /* or NULL */, const sr_field *B /* or NULL: sr_field_sightline_voigt */,
                              const sr_zeeman_table *lines, const sr_voigt_params *p, int64_t n, const double *origin,
                              const double *dir, const double *ref /* (3, n) */, int32_t n_freq, const double *omega,
                              const double *e_ph, const double *c_omega, const double *backlight /* (n, n_freq) or NULL */,
                              const double *pol /* (3): q, u, v of the backlight, or NULL */, int32_t faraday,
                              double *I, double *Q, double *U, double *Vs, double *tau /* (n, n_freq) */, double *column,
                              double *chord, int32_t *steps /* (n), may be NULL */, double *kernel_ms);

/* ---- proton radiography: charged particles pushed through prescribed E and B ----------------
 * No reference counterpart.  n independent particles of charge/mass qm are pushed through the fields E [V/m] and B [T], 3-vector
 * sr_fields (n_comp == 3) on ONE grid (when both are given the node coordinates are compared bit for bit, and the dtypes must be
 * equal), with a fixed step dt, until they leave the grid box or have made max_steps steps, and are then projected ballistically
 * onto a detector plane.  E or B may be NULL: that field is zero, it is never read, and its line of the rule is skipped (um = u
 * and u = up without E; up = um without B).  The state is x [m] and u = gamma*v [m/s]; s0 and sf are HOST arrays (6, n): rows
 * x y z ux uy uz.  push.hip is compiled with -ffp-contract=off: every operation below rounds on its own, in float64; sqrt is the
 * correctly rounded one.
 * With c = 299792458.0, ic2 = 1.0/(c*c), hq = (qm*dt)*0.5, hd = dt*0.5 and |a|^2 = (a0*a0 + a1*a1) + a2*a2, per particle:
 *   do {
 *     g  = sqrt(1.0 + |u|^2*ic2);  d = hd/g;          xm_a = x_a + u_a*d                (half drift)
 *     (E, B) at xm: sr_field_resample's cell / outside / blend rule with fill 0 (same corner order, u = 1 - w factors)
 *     um_a = u_a + hq*E_a                                                               (half kick)
 *     gm = sqrt(1.0 + |um|^2*ic2);  k = hq/gm;  t_a = k*B_a;  f = 2.0/(1.0 + |t|^2);  s_a = t_a*f
 *     w  = um + um x t;   up = um + w x s            (cross: (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0))
 *     u_a = up_a + hq*E_a                                                               (half kick)
 *     gn = sqrt(1.0 + |u|^2*ic2);   x_a = xm_a + u_a*(hd/gn)                            (half drift)
 *     steps += 1
 *   } while (x inside the grid box on every axis: g[0] <= x_a <= g[n-1]; a NaN is outside) && steps < max_steps
 * -- the Boris push in its relativistic, position-centred form.  The test is made after a step, never before the first.  A
 * particle whose midpoint xm lies outside the box on any axis sees E = B = 0 (these zeros go through the arithmetic above), so a
 * step taken outside the box is a free flight; moving a particle to the entry plane of the box is the caller's job.  A step's gn
 * is the next step's g (same inputs, same operations).  SR_PUSH_UNFINISHED is set when the loop ends by steps == max_steps with x
 * still inside.
 *   detector  a = axis: tau = (det_pos - x_a)/u_a; SR_PUSH_MISSED is set unless tau is finite and > 0.  For the two other axes
 *             b in x < y < z order (sr_volume_project's (u, v) convention), hits[j] = (x_b + u_b*tau)*hit_scale, whatever the flags.
 *   image     a particle with flags == 0 is binned into img (SR_IMG_COUNTS; x = hits[0], y = hits[1]) by the A9 binning of sr_hist2d;
 *             the counts are ADDED to what the image holds.  With img given and every host output NULL nothing but the stats
 *             comes back.
 * Counts are integer atomics and nothing else is atomic: a repeated call returns identical bits everywhere.  sf (6, n), hits
 * (2, n), steps (n) and flags (n) are HOST arrays in the order of s0; each may be NULL.  stats (may be NULL): kernel_ms is the
 * HIP-event time of the push kernel alone; finished + unfinished == n; missed counts SR_PUSH_MISSED; deposited the particles
 * binned inside img.
 * Validity: prescribed fields only (no self-fields), no scattering or stopping in the plasma (sr_particles_push_matter has
 * both), a fixed step, trilinear fields (div B is only as good as the input's).
 * Arguments are checked before the device is touched: a NULL p or s0, n < 0, a non-finite or non-positive dt, a non-finite qm,
 * det_pos or hit_scale, max_steps < 1, an axis outside 0..2, an img of another kind, E and B both NULL, a field with n_comp != 3,
 * E and B of different dtypes or on grids that differ.  n == 0 succeeds. */
typedef struct {
  double qm;            /* charge / mass [C/kg] */
  double dt;            /* step [s], > 0, finite */
  int32_t max_steps;    /* >= 1 */
  int32_t axis;         /* 0,1,2: the detector plane is  coordinate[axis] == det_pos */
  double det_pos;       /* [m] */
  double hit_scale;     /* hits are multiplied by this (1e3: mm, the detector's unit elsewhere in the project) */
} sr_push_params;
typedef struct { double kernel_ms; int64_t finished, unfinished, missed, deposited; } sr_push_stats;
#define SR_PUSH_UNFINISHED 1   /* still inside the grid after max_steps */
#define SR_PUSH_MISSED     2   /* does not reach the detector plane */
int sr_particles_push(const sr_field *E, const sr_field *B, const sr_push_params *p, int64_t n,
                      const double *s0 /* host (6, n): x y z [m], ux uy uz = gamma*v [m/s] */,
                      double *sf /* host (6, n) or NULL */, double *hits /* host (2, n) or NULL */,
                      int32_t *steps /* host (n) or NULL */, uint8_t *flags /* host (n) or NULL */,
                      sr_image *img /* SR_IMG_COUNTS or NULL */, sr_push_stats *stats /* or NULL */);

/* ---- proton radiography through matter: sr_particles_push with collisional stopping and scattering moments ----------------
 * No reference counterpart.  sr_particles_push's particles, fields, step, detector, image and host outputs; E and B may now both
 * be NULL (matter only).  ne [m^-3] (required) and Z, the mean ionisation, are scalar sr_fields (n_comp == 1) on the grid and of
 * the dtype of E / B (node coordinates compared bit for bit).  Z NULL: the uniform p->Z, and nothing is read.  The projectile has
 * the mass `mass` and the charge number z (p->push.qm stays what E and B act on); the material the nuclear charge Zn, the mean
 * excitation energy I [J] and the scattering logarithm lnLs.  push_matter.hip is compiled with -ffp-contract=off: every operation
 * below rounds on its own, in float64; sqrt and / are the correctly rounded ones, log is the device library's.
 * Constants, each formed in float64 on the host exactly as written: c, ic2, hq, hd as sr_particles_push's; e = 1.602176634e-19,
 * m_e = 9.1093837015e-31, eps0 = 8.8541878128e-12, hbar = 1.054571817e-34, pi = 3.141592653589793; e2 = e*e, mc2 = mass*(c*c),
 * A2 = (2.0*m_e)*(c*c), HW = hbar*sqrt(e2/(eps0*m_e)), ze = (z*e2)/((4.0*pi)*eps0), KS = ((z*z)*(e2*e2))/((((4.0*pi)*eps0)*eps0)*m_e),
 * KT = (((8.0*pi)*(Zn*(Zn + 1.0)))*(ze*ze))*lnLs.  Per particle, with s = M0 = M1 = M2 = 0.0 at the start:
 *   do {
 *     sr_particles_push's step up to its second half kick: xm, (E, B) at xm, um, up, u_a = up_a + hq*E_a
 *     (ne, Z) at xm: the same cell, weights and corner order as E and B, fill 0 (Z: p->Z when no field is given)
 *     uu = |u|^2;  q = uu*ic2;  gn = sqrt(1.0 + q);  un = sqrt(uu);  v = un/gn;  ds = v*dt
 *     matter = xm inside the box on every axis && ne > 0.0 && Z > 0.0                      (a NaN fails a comparison)
 *     if (matter && !(uu > 0.0)) stopped                                                   (at rest in matter)
 *     else if (matter) {                                                                   (scattering power, Fermi-Eyges moments)
 *       pv = (mass*uu)/gn;  Ts = (KT*(ne/Z))/(pv*pv);  sm = s + 0.5*ds;  t = Ts*ds
 *       M0 = M0 + t;  M1 = M1 + t*sm;  M2 = M2 + (t*sm)*sm }
 *     s = s + ds                                                                           (every step, matter or not)
 *     if (matter && !stopped) {                                                            (Bethe stopping as a drag on u)
 *       aq = A2*q;  b2 = q/(gn*gn);  Lf = log(aq/(HW*sqrt(ne))) - b2;  Lb = log(aq/I) - b2
 *       dz = Zn - Z;  nb = (ne*(dz > 0.0 ? dz : 0.0))/Z
 *       N = ne*(Lf > 0.0 ? Lf : 0.0) + nb*(Lb > 0.0 ? Lb : 0.0);  S = (KS/(v*v))*N;  fac = 1.0 - ((S/mass)*dt)/un
 *       u_a = fac > 0.0 ? u_a*fac : 0.0;  q = |u|^2*ic2;  gn = sqrt(1.0 + q)
 *       stopped = !(fac > 0.0) || (mc2*q)/(gn + 1.0) < stop_energy }
 *     steps += 1
 *     if (stopped) { x_a = xm_a; leave the loop }
 *     x_a = xm_a + u_a*(hd/gn)                                                             (half drift)
 *   } while (x inside the grid box on every axis && steps < max_steps)
 * S = z^2 e^4/(4 pi eps0^2 m_e v^2) [ne Lf + nb Lb] is Bethe's stopping power of the free electrons (hbar*omega_p in the
 * logarithm's place of I) and of the nb = ne (Zn - Z)/Z bound ones, a logarithm that is not positive dropped (the projectile is
 * then no faster than those electrons); q/gn^2 = beta^2.  Ts = 8 pi (ne/Z) Zn (Zn + 1) (z e^2/(4 pi eps0))^2/(p v)^2 lnLs is the
 * scattering power d<theta^2>/ds (Jackson 13.6 in SI, the electrons' share through Zn + 1), from the values before the drag.
 * M0, M1, M2 are the moments of Ts over the path length s (midpoint rule), from which the caller forms the Fermi-Eyges
 * variances on a plane; the kernel draws no random numbers and the scattering does not act on the path.  A stopped particle
 * gets SR_PUSH_STOPPED, stays at the midpoint with the u the drag left it (0 when fac <= 0), is not binned, and is not
 * SR_PUSH_UNFINISHED; the detector line is applied to it as to any other.  Where ne = 0 everywhere, sf, hits, steps and flags
 * are sr_particles_push's bits.
 * energy (n): (mc2*(|u|^2*ic2))/(gn + 1.0) of the final u [J].  moments (4, n): rows M0 [rad^2], M1 [rad^2 m], M2 [rad^2 m^2]
 * and s of the last step [m].  Both are HOST arrays and may be NULL, as sf, hits, steps and flags.  stats: sr_push_stats'
 * members, and stopped, the particles with SR_PUSH_STOPPED (they count as finished).
 * Validity: sr_particles_push's, and a cold target or v >> the electrons' thermal speed, no nuclear reactions, no straggling (every
 * particle loses the mean), a single material, small-angle scattering that does not feed back on the path.
 * Arguments are checked before the device is touched: sr_particles_push's checks (E and B both NULL is allowed), a NULL ne, mass,
 * Zn or I not finite and positive, a non-finite z, lnLs or stop_energy negative or not finite, Z NULL with p->Z not finite and
 * positive, a field with the wrong n_comp, of another dtype or on another grid than ne.  n == 0 succeeds. */
typedef struct {
  sr_push_params push;
  double mass;          /* the projectile's mass [kg], > 0 */
  double z;             /* its charge number */
  double Zn;            /* the material's nuclear charge, > 0 */
  double I;             /* its mean excitation energy [J], > 0 */
  double lnLs;          /* the scattering logarithm, >= 0 */
  double Z;             /* the uniform mean ionisation, read when the Z field is NULL; then > 0 */
  double stop_energy;   /* [J], >= 0: a particle whose kinetic energy falls below it is stopped */
} sr_push_matter_params;
typedef struct { double kernel_ms; int64_t finished, unfinished, missed, deposited, stopped; } sr_push_matter_stats;
#define SR_PUSH_STOPPED    4   /* stopped in the matter */
int sr_particles_push_matter(const sr_field *E /* or NULL */, const sr_field *B /* or NULL */, const sr_field *ne,
                             const sr_field *Z /* or NULL */, const sr_push_matter_params *p, int64_t n,
                             const double *s0 /* host (6, n) */, double *sf, double *hits, int32_t *steps, uint8_t *flags,
                             double *energy /* host (n) or NULL */, double *moments /* host (4, n) or NULL */,
                             sr_image *img /* SR_IMG_COUNTS or NULL */, sr_push_matter_stats *stats /* or NULL */);

/* ---- optical Thomson scattering: the spectral density function summed over scattering volumes ----------------
 * No reference counterpart.  n_vol scattering volumes, each a quadrature of n_quad points p_q [m] with weights w_q [m] along the
 * probe inside the collection cone, scatter a probe of wavelength lambda_i from unit direction ki (per volume) into the unit
 * direction ks (per volume); the scattered power is evaluated at n_lambda wavelengths.  The model is non-relativistic and
 * unmagnetised: Maxwellian electrons and ONE Maxwellian ion species (charge Z, mass number A) that share the flow V, vacuum
 * wavenumbers -- valid for ne << n_crit (Sheffield; Froula et al.).  ne [m^-3], Te [eV], Ti [eV], Z are scalar sr_fields and V
 * [m/s] a 3-vector sr_field on ONE grid (node coordinates compared bit for bit) and of one dtype.  Ti NULL: Ti = Te.  Z NULL: the
 * uniform p->Z.  V NULL: no flow, nothing of V is read and the Doppler line reads wp = w.  thomson.hip is compiled with
 * -ffp-contract=off: every operation below rounds on its own, in float64; sqrt and / are the correctly rounded ones, rint rounds
 * half to even, exp is the device library's.
 * Constants, each formed in float64 on the host exactly as written: c = 299792458.0, e = 1.602176634e-19, m_e = 9.1093837015e-31,
 * m_p = 1.67262192369e-27, eps0 = 8.8541878128e-12, pi = 3.141592653589793; tpc = (2.0*pi)*c, ce = (2.0*e)/m_e,
 * ci = (2.0*e)/(A*m_p), ee0 = e/eps0, SP = 1.7724538509055159 (sqrt(pi)), TSP = 3.5449077018110318, ISP = 0.5641895835477563.
 *   volume m      cth = (ki0*ks0 + ki1*ks1) + ki2*ks2;  wi = tpc/lambda_i;  kin = wi/c
 *   wavelength l  ws = tpc/lambda_l;  w = ws - wi;  ksc = ws/c;  k2 = (ksc*ksc + kin*kin) - ((2.0*ksc)*kin)*cth
 *                 k = sqrt(k2);  rk = 1.0/k;  rk2 = 1.0/k2;  f_l = (1.0 + (2.0*w)/wi) * (c/(lambda_l*lambda_l))
 *   point q       ne, Te, Ti, Z and the three components of V at p_q: sr_field_resample's cell / outside / blend rule (same corner
 *                 order, u = 1 - w factors).  The point is DROPPED -- it adds nothing to P or to weight -- when p_q lies outside
 *                 the box on any axis (a point on a face is inside; a NaN coordinate is outside), when ne <= 0, Te <= 0 or Ti <= 0,
 *                 or when any gathered value is NaN.  Otherwise
 *                   wn = w_q*ne;  ivte = 1.0/sqrt(ce*Te);  ivti = 1.0/sqrt(ci*Ti);  pe = (ne*ee0)/Te;  zt = (Z*Te)/Ti
 *                   vs = (V0*ks0 + V1*ks1) + V2*ks2;  vi = (V0*ki0 + V1*ki1) + V2*ki2
 *   sample (l, q) wp = w - (ksc*vs - kin*vi);  a = wp*rk;  xe = a*ivte;  xi = a*ivti;  al = pe*rk2;  az = al*zt
 *                 (Fe, Ee) = D(xe);  (Fi, Ei) = D(xi)                                       (below)
 *                 cer = al*(1.0 - (2.0*xe)*Fe);  cei = al*((SP*xe)*Ee);  cir = az*(1.0 - (2.0*xi)*Fi);  cii = az*((SP*xi)*Ei)
 *                 er = (1.0 + cer) + cir;  ei = cei + cii;  ie2 = 1.0/(er*er + ei*ei)
 *                 n1 = (1.0 + cir)*(1.0 + cir) + cii*cii;  n2 = cer*cer + cei*cei
 *                 S = (TSP*rk) * (((n1*ie2)*Ee)*ivte + ((Z*(n2*ie2))*Ei)*ivti)
 *               -- chi_e = alpha^2 W(xi_e), chi_i = alpha^2 (Z Te/Ti) W(xi_i), eps = 1 + chi_e + chi_i with alpha^2 = al and
 *               W(x) = 1 - 2x F(x) + i sqrt(pi) x exp(-x^2), F Dawson's function.
 *   D(x)          Dawson's function by Rybicki's sampling form with h = 0.25, and exp(-x^2):
 *                   n0 = 2.0*rint(2.0*x);  xp = x - 0.25*n0;  g = exp(-(xp*xp));  p = exp(0.5*xp);  m = 1.0/p;  p2 = p*p;  m2 = m*m
 *                   d0 = n0*n0;  s = 0;  for n = 1, 3, 5, ..., 25 in this order:
 *                       s = s + C[n]*((p*(n0 - n) + m*(n0 + n))/(d0 - n*n));   p = p*p2;   m = m*m2
 *                   F = (g*s)*ISP;   E = exp(-(x*x))
 *                 -- the terms n and -n of sum_{n odd} C[n] e^{2 xp h n}/(n0 + n) over one denominator, the powers by repeated
 *                 multiplication; C[n] = exp(-(n h)^2): 0.9394130628134758, 0.569782824730923, 0.2096113871510978,
 *                 0.04677062238395898, 0.006329715427485747, 0.0005195746821548384, 2.586810022265412e-05, 7.811489408304491e-07,
 *                 1.4307241918567688e-08, 1.5893910094516368e-10, 1.0709232382508077e-12, 4.37661850287085e-15,
 *                 1.0848552640429378e-17.  Truncation at |n| <= 25 leaves less than 1e-16; three exp per D.
 *   output        P[m][l] = (sum over the kept q, ascending, of wn*S) * f_l;   weight[m] = sum over the kept q, ascending, of wn
 *                 -- P is (1/2pi) int ne S(k, w) dl (1 + 2w/wi) |dw/dlambda|; the caller multiplies by r_e^2 and the polarisation
 *                 factor.  A volume whose points are all dropped gives exact zeros.  No atomics: a repeated call returns identical
 *                 bits.
 * pts (n_vol, n_quad, 3), wts (n_vol, n_quad), ki and ks (n_vol, 3), lambda (n_lambda), P (n_vol, n_lambda) and weight (n_vol) are
 * HOST arrays, float64, C order.  *kernel_ms (may be NULL) is the HIP-event time of the kernel alone.
 * Arguments are checked before the device is touched: a NULL p, pts, wts, ki, ks, lambda, P or weight; n_vol, n_quad or n_lambda
 * below 0; lambda_i, A or an entry of lambda not finite and positive; a non-finite p->Z where the Z field is NULL; a direction
 * that is not finite or whose squared length is further than 1e-12 from 1; ki == ks exactly, or cth >= 1 (k can then be 0); more
 * than 2^31 - 1 workgroups; a NULL ne or Te; a field of the wrong n_comp; fields of differing dtypes or on grids that differ.
 * n_vol == 0 or n_lambda == 0 succeeds and writes nothing; with n_quad == 0 every output is 0. */
typedef struct {
  double lambda_i;      /* probe wavelength [m] */
  double A;             /* ion mass number (m_i = A*m_p) */
  double Z;             /* the uniform ion charge where the Z field is NULL */
} sr_thomson_params;
int sr_field_thomson(const sr_field *ne, const sr_field *Te, const sr_field *Ti /* or NULL */, const sr_field *Z /* or NULL */,
                     const sr_field *V /* or NULL */, const sr_thomson_params *p, int64_t n_vol, int32_t n_quad,
                     const double *pts, const double *wts, const double *ki, const double *ks, int32_t n_lambda,
                     const double *lambda, double *P, double *weight, double *kernel_ms);

/* ---- optical Thomson scattering with several ion species and drifting electrons --------------------------------
 * No reference counterpart.  sr_field_thomson's model with n_species = 1 .. SR_MAX_SPECIES Maxwellian ion species in place of one
 * and, optionally, electrons that drift against the ions.  Species j = 0 .. n_species-1 has the mass number p->A[j] (uniform), the
 * charge Z_j and the relative abundance f_j -- each either the scalar sr_field Zs[j] / fracs[j] or, where that entry (or the whole
 * array) is NULL, the uniform p->Z[j] / p->frac[j].  The f_j are relative ion NUMBER fractions and need not sum to 1.  Ti and the
 * flow V are shared by all species.  Vd [m/s] is a 3-vector sr_field: the drift of the electrons relative to the ions,
 * Vd = -J/(e ne); NULL: no drift, nothing of Vd is read and the electron line reads ae = a.  All fields lie on ONE grid and have
 * one dtype.  Everything sr_field_thomson states holds unchanged -- the constants, the `volume` and `wavelength` lines, the gather
 * rule, D(x), the `output` line, float64 throughout, thomson_multi.hip compiled with -ffp-contract=off -- with
 * ci_j = (2.0*e)/(A_j*m_p) formed on the host and
 *   point q       ne, Te, Ti and V as sr_field_thomson gathers them; every Z_j and f_j that is a field and the three components of
 *                 Vd with the same cell and weights.  The point is DROPPED under sr_field_thomson's conditions, when any gathered
 *                 Z_j, f_j or component of Vd is NaN, or when any Z_j < 0 or f_j < 0.  Otherwise wn, ivte, pe, vs, vi as there and
 *                   zb = 0.0;  for j ascending: zb = zb + f_j*Z_j
 *                   c_j = zb > 0.0 ? (f_j*Z_j)/zb : 0.0;  g_j = Z_j*c_j;  zt_j = (g_j*Te)/Ti;  ivti_j = 1.0/sqrt(ci_j*Ti)
 *                   ds = (D0*ks0 + D1*ks1) + D2*ks2;  di = (D0*ki0 + D1*ki1) + D2*ki2         (D = Vd; only when Vd is given)
 *                 -- c_j is the share of the electrons that species j supplies, g_j = Z_j^2 n_j/ne.
 *   sample (l, q) wp = w - (ksc*vs - kin*vi)  (V given, else wp = w);  a = wp*rk
 *                 ae = (wp - (ksc*ds - kin*di))*rk  (Vd given, else ae = a)
 *                 xe = ae*ivte;  al = pe*rk2;  (Fe, Ee) = D(xe);  cer = al*(1.0 - (2.0*xe)*Fe);  cei = al*((SP*xe)*Ee)
 *                 er = 1.0 + cer;  ei = cei;  sr = 1.0;  si = 0.0
 *                 for j ascending:  xi = a*ivti_j;  az = al*zt_j;  (Fi, Ei_j) = D(xi)
 *                                   cir = az*(1.0 - (2.0*xi)*Fi);  cii = az*((SP*xi)*Ei_j)
 *                                   er = er + cir;  ei = ei + cii;  sr = sr + cir;  si = si + cii
 *                 ie2 = 1.0/(er*er + ei*ei);  n1 = sr*sr + si*si;  n2 = cer*cer + cei*cei;  t = n2*ie2
 *                 ion = 0.0;  for j ascending: ion = ion + ((g_j*t)*Ei_j)*ivti_j
 *                 S = (TSP*rk) * (((n1*ie2)*Ee)*ivte + ion)
 *               -- S = (2 pi/k) [ |1 + sum_j chi_j|^2/|eps|^2 f_e + sum_j (Z_j^2 n_j/ne) |chi_e|^2/|eps|^2 f_j ] with
 *               chi_j = alpha^2 (Z_j^2 n_j/ne)(Te/Ti) W(xi_j), the electrons' argument moved by k.Vd.  A species whose g_j is 0
 *               at a point adds exact zeros (the kernel skips it).  One species with f = 1 and Z >= 0 gives sr_field_thomson's
 *               bits: c = 1 exactly, and every added 0.0 + and 1.0 + is exact.
 * Arguments are checked before the device is touched: everything sr_field_thomson checks; n_species outside 1 .. SR_MAX_SPECIES;
 * an A[j] not finite and positive; a uniform Z[j] or frac[j] that is read (its field is NULL) and is not finite or is negative;
 * Vd with n_comp != 3; a Zs or fracs entry with n_comp != 1 (named Z0.., f0.. in the text); differing dtypes or grids.
 * n_vol == 0 or n_lambda == 0 succeeds and writes nothing. */
#define SR_MAX_SPECIES 4
typedef struct {
  double lambda_i;      /* probe wavelength [m] */
  int32_t n_species;    /* 1 .. SR_MAX_SPECIES */
  int32_t reserved;
  double A[SR_MAX_SPECIES];     /* mass numbers (m_j = A_j*m_p) */
  double Z[SR_MAX_SPECIES];     /* the uniform charge of species j where Zs[j] is NULL */
  double frac[SR_MAX_SPECIES];  /* the uniform relative abundance of species j where fracs[j] is NULL */
} sr_thomson_multi_params;      /* 112 bytes */
int sr_field_thomson_multi(const sr_field *ne, const sr_field *Te, const sr_field *Ti /* or NULL */, const sr_field *V /* or NULL */,
                           const sr_field *Vd /* or NULL */, const sr_field *const *Zs /* NULL, or n_species entries each field or NULL */,
                           const sr_field *const *fracs /* likewise */, const sr_thomson_multi_params *p, int64_t n_vol,
                           int32_t n_quad, const double *pts, const double *wts, const double *ki, const double *ks,
                           int32_t n_lambda, const double *lambda, double *P, double *weight, double *kernel_ms);

/* ---- optical Thomson scattering from super-Gaussian (Langdon) electrons ----------------------------------------
 * No reference counterpart.  sr_field_thomson_multi's model -- species, flow V, drift Vd, one Ti -- with the electron distribution
 *   f(v) = m/(4 pi Gamma(3/m) v_m^3) exp(-(v/v_m)^m),   v_m^2 = 3 (k Te/m_e) Gamma(3/m)/Gamma(5/m)
 * in place of the Maxwellian (m = 2), the shape inverse-bremsstrahlung heating drives (Langdon 1980; Matte et al. 1988).  Te keeps
 * its meaning as 2/3 of the mean energy.  The order m is LOCAL: either the scalar sr_field `order`, on the grid and of the dtype of
 * the other fields and gathered with the same cell and weights, or, where `order` is NULL, the uniform p->order.  Everything
 * sr_field_thomson_multi states holds unchanged -- the constants, the `volume`, `wavelength` and `output` lines, the gather rule,
 * the `point` lines, D(x), float64 throughout, thomson_sg.hip compiled with -ffp-contract=off -- with, in sr_field_thomson_multi's
 * names al, ae, ivte, xe:
 *   point q       mo = the gathered order (or p->order).  The point is DROPPED under sr_field_thomson_multi's conditions or when mo
 *                 is NaN.  Otherwise m = min(max(mo, 2.0), 5.0) (an infinite mo is clamped like any other), and
 *                 when m - 2.0 <= 2^-30 the sample (l, q) follows sr_field_thomson_multi's `sample` lines exactly (a trilinear
 *                 blend of nodes that all hold 2 need not round to 2, hence the threshold).  Else, with GAM below,
 *                   im = 1.0/m;  z2 = 2.0*im;  G1 = GAM(im);  G2 = GAM(z2);  G3 = GAM(3.0*im);  G5 = GAM(5.0*im)
 *                   r = sqrt((2.0*G5)/(3.0*G3));  b = m/(2.0*G1);  c = (G1*G5)/((3.0*G3)*G3);  T = pow(40.0, im)
 *                   fe = (SP*r)/(2.0*G3);  pib = pi*b;   for i = 0 .. 47:  g_i = exp(-pow(T*S2[i], m))
 *                 -- r = v_te/v_m (v_te^2 = 2 k Te/m_e), b = m/(2 Gamma(1/m)) normalises b int exp(-|t|^m) dt = 1, and
 *                 al*c = omega_pe^2 Gamma(1/m)/(k^2 v_m^2 Gamma(3/m)).  At m = 2: r = c = 1, b = 1/sqrt(pi).
 *   sample (l, q) wp, a, ae, xe, al as in sr_field_thomson_multi;  xs = xe*r;  x = |xs|;  y = pow(x, m);  gx = exp(-y);  x2 = x*x
 *                 (R, below);  ac = al*c;  cer = ac*R;  cei = ac*((pib*xs)*gx);  (Q, below);  Ee = fe*Q
 *                 and from `er = 1.0 + cer` on the lines of sr_field_thomson_multi with these cer, cei and Ee.
 *               -- chi_e = al c [R_m(xs) + i pi b xs exp(-|xs|^m)], R_m(xs) = b P int t exp(-|t|^m)/(t - xs) dt = 1 - xs W_m(xs)
 *               (W_2 = 2 Dawson), from chi = -(omega_pe^2/k^2) int f1'(u)/(u - w/k) du with the 1-D projection
 *               f1(u) = Gamma(2/m, (|u|/v_m)^m)/(2 Gamma(3/m) v_m); the electron term of S is (2 pi/k) f1(w/k), so exp(-xe^2)*ivte
 *               of the Maxwellian becomes sqrt(pi) Gamma(2/m, y)/(2 Gamma(3/m)) * r * ivte = Ee*ivte.
 *   R             Both signs of t folded onto t > 0, the integral cut at T (exp(-T^m) = e^-40), t = T s^2 on the 48-point
 *                 Gauss-Legendre rule (s_i, w_i) of [0, 1] -- the square removes the t^(m-1) behaviour of exp(-t^m) at 0 -- and,
 *                 inside, exp(-x^m) subtracted so that the principal value is a logarithm.  S2[i] = s_i^2 and V[i] = 2 w_i s_i,
 *                 ascending, are the float64 constants kS2 and kV of thomson_sg.hip.  x < T:
 *                   tx = 2.0*x;  L = log((T - x)/(T + x));  s = 0;  for i ascending:  t = T*S2[i];  e = t - x;  dg = g_i - gx
 *                       |e| < 1e-6 ?  pm1 = m*pow(x, m - 1.0);  g1 = -(pm1*gx);  g2 = gx*(pm1*pm1 - (m*(m - 1.0))*pow(x, m - 2.0))
 *                                     h = (g1 + (0.5*g2)*e) - dg/(t + x)
 *                                  :  h = (dg*tx)/(t*t - x2)
 *                       s = s + V[i]*h
 *                   R = 1.0 + (x*b)*(T*s + gx*L)
 *                 x >= T (no cancellation against 1):
 *                   s = 0;  for i ascending:  t = T*S2[i];  tt = t*t;  s = s + V[i]*((g_i*(2.0*tt))/(tt - x2))
 *                   R = (b*T)*s
 *                 -- one division per node serves t and -t; g1, g2 are the first two derivatives of exp(-x^m), which replace the
 *                 1/(t - x) half of a node's term where the node collides with x.  R is even in xs and cei odd, bit for bit;
 *                 R(0) = 1 exactly.  Against 34-digit quadrature max |R - R_ref| (1 + xs^2) = 1.5e-11 (m = 2.05, xs = 1.61).
 *   Q             Gamma(z2, y), the upper incomplete gamma function, with y^z2 exp(-y) = x2*gx:  xg = x2*gx
 *                 y < z2 + 1.0, the series:  ap = z2;  de = 1.0/z2;  sm = de;  at most 100 times:
 *                       ap = ap + 1.0;  de = de*(y/ap);  sm = sm + de;  stop when |de| < |sm|*1e-16
 *                   Q = G2 - sm*xg
 *                 else the continued fraction by the modified Lentz scheme:  bb = (y + 1.0) - z2;  cc = 1.0/1e-300;  d = 1.0/bb
 *                   h = d;  for i = 1 .. 100 (none when y is infinite):  an = -i*(i - z2);  bb = bb + 2.0
 *                       d = an*d + bb;  |d| < 1e-300 ? d = 1e-300;  cc = bb + an/cc;  |cc| < 1e-300 ? cc = 1e-300;  d = 1.0/d
 *                       de = d*cc;  h = h*de;  stop when |de - 1.0| < 1e-16
 *                   Q = xg*h
 *                 -- 1.1e-13 relative against scipy.special.gammaincc*gamma, at most 85 terms.
 *   GAM(z)        The gamma function for 0.2 <= z <= 2.5 by its Chebyshev series on [1, 2] (24 coefficients GC[k], the float64
 *                 constants kGC of thomson_sg.hip; the next is below 1e-18) and one step of the recurrence, so that host and
 *                 device agree bit for bit (+, * and / only):
 *                   w = z < 1.0 ? z + 1.0 : (z > 2.0 ? z - 1.0 : z);  tau = 2.0*w - 3.0;  t2 = 2.0*tau;  b1 = b2 = 0
 *                   for k = 23 down to 1:  b0 = (GC[k] + t2*b1) - b2;  b2 = b1;  b1 = b0
 *                   P = (GC[0] + tau*b1) - b2;   GAM = z < 1.0 ? P/z : (z > 2.0 ? (z - 1.0)*P : P)
 * pow, exp and log are the device library's.  order NULL with p->order == 2, and an order field of 2.0 everywhere, return
 * sr_field_thomson_multi's bits.  Arguments are checked before the device is touched: everything sr_field_thomson_multi checks; a
 * uniform order (order NULL) outside [2, 5] or NaN; an order field with n_comp != 1, of another dtype or on another grid.
 * Not modelled: per-species Ti, magnetised and relativistic corrections, anisotropic or otherwise non-isotropic distortions of
 * the electron distribution, m outside [2, 5] (clamped), more than one GPU. */
typedef struct {
  double lambda_i;      /* probe wavelength [m] */
  int32_t n_species;    /* 1 .. SR_MAX_SPECIES */
  int32_t reserved;
  double A[SR_MAX_SPECIES];     /* mass numbers (m_j = A_j*m_p) */
  double Z[SR_MAX_SPECIES];     /* the uniform charge of species j where Zs[j] is NULL */
  double frac[SR_MAX_SPECIES];  /* the uniform relative abundance of species j where fracs[j] is NULL */
  double order;                 /* the uniform order m in [2, 5] where the order field is NULL */
} sr_thomson_sg_params;         /* 120 bytes */
int sr_field_thomson_sg(const sr_field *ne, const sr_field *Te, const sr_field *Ti /* or NULL */, const sr_field *V /* or NULL */,
                        const sr_field *Vd /* or NULL */, const sr_field *const *Zs /* NULL, or n_species entries each field or NULL */,
                        const sr_field *const *fracs /* likewise */, const sr_field *order /* or NULL: p->order */,
                        const sr_thomson_sg_params *p, int64_t n_vol, int32_t n_quad, const double *pts, const double *wts,
                        const double *ki, const double *ks, int32_t n_lambda, const double *lambda, double *P, double *weight,
                        double *kernel_ms);

/* ---- wave optics: a paraxial split-step march of a complex field through a domain ----------
 * No counterpart in the reference's sources (its authors compare the tracer with a CPU beam-propagation library,
 * evaluation/c.f._diffraction).  A complex scalar field U on a uniform lateral FRAME of mu x mv pixels is carried through the
 * electron density of a domain along grid axis `axis`: a thin phase (and absorption) screen per cell between two node planes and a
 * free-space (Fresnel) step between the screens' mid-planes, by 2-D transforms on the frame.  The field varies as
 * exp(+i(kz - wt)), the carrier exp(i k0 z) is dropped, so a plasma screen (n < 1) has NEGATIVE phase.  Paraxial and scalar; the
 * frame is periodic (leave a guard band, or absorb at the edges with wu, wv); nothing is reflected where ne approaches critical.
 * ne [m^-3], and optionally Te [eV] and Z, are scalar sr_fields on ONE grid (node coordinates compared bit for bit) and of one
 * dtype.  Te NULL: no absorption, Z is not looked at.  Z NULL: the uniform p->Z.  wave.hip is compiled with -ffp-contract=off:
 * every operation below rounds on its own, in float64; the transforms are hipFFT's (Z2Z, unnormalised), cos, sin, exp and log the
 * device library's.
 *   frame     pixel (i, j), i < mu, j < mv, sits at (pu, pv) = (u0 + i*du, v0 + j*dv) on the two lateral axes (u, v) in x < y < z
 *             order (axis 0: y, z; 1: x, z; 2: x, y), i*du and j*dv being float64 products.  U is (mu, mv) complex128, C order.
 *   planes    g = the float64 values of the float32 nodes on `axis`; toward = +1 marches planes 0 -> n-1, -1 the reverse.  Cell c,
 *             c = 0 .. n_c - 1 with n_c = n - 1, lies between consecutive planes k, k' of the march, h_c = |g[k'] - g[k]|.
 *             d_0 = 0.5*h_0;  d_c = 0.5*(h_{c-1} + h_c);  d_{n_c} = 0.5*h_{n_c - 1}.
 *   sequence  for c = 0 .. n_c - 1: D(d_c), then S_c; finally D(d_{n_c}).  U_out is the field on the last plane of the march.
 *   D(d)      forward transform; per mode (i, j), with pd = pi_l*d formed once:
 *               th = -(pd * (fu[i]*fu[i] + fv[j]*fv[j]));  co = cos(th);  si = sin(th)
 *               (re, im) <- ((re*co - im*si) * s, (re*si + im*co) * s),   s = 1.0/((double)mu*(double)mv)
 *             -- four products, two sums, then the scale; inverse transform.  fu, fv: the frame's spatial frequencies [1/m]
 *             (np.fft.fftfreq(mu, du), np.fft.fftfreq(mv, dv)); pi_l = pi*lambda.
 *   S_c       per pixel: on each lateral axis sr_field_resample's `cell` rule gives the cell (iu | iv) and the weight (wu_ | wv_)
 *             of pu | pv; a pixel with pu or pv below the first or above the last node of its axis is VACUUM (ne = 0, alpha = 0
 *             on both planes; no field is read); a pixel exactly on the last node is inside.  With uu = 1 - wu_, uv = 1 - wv_,
 *             w00 = uu*uv, w01 = uu*wv_, w10 = wu_*uv, w11 = wu_*wv_ and f(a, b) the node (iu + a, iv + b) of a node plane
 *             widened to float64, a field's value on that plane is sr_field_resample's blend of ONE node plane,
 *               ((f(0,0)*w00 + f(0,1)*w01) + f(1,0)*w10) + f(1,1)*w11                       (ne, and with Te given: Te, Z).
 *             index   ne <= 0: m = 0.  Otherwise wp = 5.64e4*sqrt(ne*1e-6);  r = wp/omega;  q = r*r;  q >= 1.0 on either plane:
 *                     the pixel is OPAQUE for this screen, U <- (0, 0).  Otherwise m = -q/(1.0 + sqrt(1.0 - q))  ( = n - 1 ).
 *             phase   ph = (k0*h_c) * (0.5*(m_k + m_k'))
 *             absorb  with Te: alpha per plane by sr_field_emission's `node` rule on the plane's (ne, Te, Z) and this omega;
 *                     dtau = (0.5*(alpha_k + alpha_k'))*h_c;  a = exp(-(0.5*dtau)).  Without Te: a = 1.0.
 *             update  co = cos(ph);  si = sin(ph);  t = (a*wu[i])*wv[j];  (re, im) <- ((re*co - im*si)*t, (re*si + im*co)*t)
 *             -- wu, wv: the edge absorber's windows (NULL: 1.0).  A NaN node makes NaN the pixels whose cell holds it, and after
 *             the next transform the whole field: it is not guarded against.
 *   power[c]  (may be NULL; n_c values) the sum of re*re + im*im over the pixels after S_c, in a FIXED order: pixels in C order
 *             in groups of 1024, a group's sum by one fixed tree (per lane four pixels 256 apart, a shuffle tree over each
 *             wavefront, the four wavefronts in order), the groups' sums added in ascending order.  No atomics: a repeated call
 *             returns identical bits, U_out included.
 * fu (mu), fv (mv), wu (mu), wv (mv), U_in and U_out (mu, mv, 2) are HOST arrays, float64.  kernel_ms (may be NULL) points to
 * THREE values: the HIP-event time of the whole march [ms], and -- only with p->time_parts != 0, which puts an event between all
 * the launches; 0 otherwise -- the part of it spent in hipFFT and the part in the library's own two kernels.
 * Arguments are checked before the device is touched: a NULL p, fu, fv, U_in or U_out; mu or mv below 2, or mu*mv above 2^30;
 * lambda, omega, k0, pi_l, du or dv not finite and positive; a non-finite u0 or v0; toward not +-1; axis outside 0..2; a NULL ne;
 * a vector field; fields of differing dtypes or on grids that differ; with Te given and Z NULL, a non-finite p->Z. */
typedef struct {
  int32_t axis, toward;           /* 0 | 1 | 2;  +1 | -1 */
  int32_t mu, mv;                 /* the frame */
  double u0, du, v0, dv;          /* pixel (i, j) at (u0 + i*du, v0 + j*dv) [m] */
  double lambda;                  /* vacuum wavelength [m] */
  double omega, k0, pi_l;         /* 2 pi c/lambda, omega/c, pi*lambda: formed by the host */
  double Z;                       /* the uniform ion charge where Te is given and the Z field is NULL */
  int32_t time_parts, reserved;   /* != 0: kernel_ms[1], [2] are measured */
} sr_wave_params;
int sr_field_wave(const sr_field *ne, const sr_field *Te /* or NULL */, const sr_field *Z /* or NULL */, const sr_wave_params *p,
                  const double *fu, const double *fv, const double *wu /* or NULL */, const double *wv /* or NULL */,
                  const double *U_in, double *U_out, double *power /* or NULL */, double *kernel_ms /* [3] or NULL */);
/* The exit field on the detector of an ideal one-to-one relay with a mask in the Fourier plane of a lens of focal length f and a
 * defocus: forward transform; per mode (i, j), with pd = pi_l*defocus and s = 1.0/((double)mu*(double)mv),
 *     th = -(pd * (fu[i]*fu[i] + fv[j]*fv[j]));  (re, im) <- ((re*cos(th) - im*sin(th))*s, (re*sin(th) + im*cos(th))*s)
 *     xf = lf*fu[i];  yf = lf*fv[j];  r2 = xf*xf + yf*yf                 (lf = lambda*f: the mode's place in the focal plane)
 *     (re, im) <- (0.0, 0.0) where a mask that is switched on rejects (xf, yf), as the ray optics do (SR_OP_CIRC_AP, _CIRC_STOP,
 *     _KNIFE):  SR_WAVE_APERTURE: r2 > Ra*Ra;  SR_WAVE_STOP: r2 < Rs*Rs;  SR_WAVE_KNIFE: with x = xf (knife_axis 0) or yf (1),
 *     x > knife_offset where knife_dir > 0, x < knife_offset where knife_dir < 0
 * -- inverse transform.  Without a mask and with defocus 0 the output is the input to the transforms' rounding; defocus = d on its
 * own is D(d) of sr_field_wave.  U_in, U_out: HOST (mu, mv, 2) float64.  *kernel_ms (may be NULL): the HIP-event time.  Checked
 * before the device is touched: a NULL p, fu, fv, U_in or U_out; mu or mv below 2, or mu*mv above 2^30; non-finite pi_l, defocus
 * or lf; flags outside the three bits; with its mask on, a non-finite Ra, Rs or knife_offset, knife_axis not 0 | 1, knife_dir 0
 * or NaN. */
#define SR_WAVE_APERTURE 1
#define SR_WAVE_STOP 2
#define SR_WAVE_KNIFE 4
typedef struct {
  int32_t mu, mv, flags, knife_axis;
  double pi_l, defocus, lf;       /* pi*lambda [m], defocus [m], lambda*f [m^2] */
  double Ra, Rs;                  /* aperture and stop radii in the focal plane [m] */
  double knife_offset, knife_dir; /* [m]; > 0 rejects above the offset, < 0 below */
} sr_wave_image_params;
int sr_wave_image(const sr_wave_image_params *p, const double *fu, const double *fv, const double *U_in, double *U_out,
                  double *kernel_ms);

/* ---- the step before the path: volume synthesis ------------------------------------
 * gaussian3D.domain_fft (src/field_generator/gaussian3D.py:215-271): out = Re(ifftn(noise * amp)) [/ max|.| when
 * normalise], noise complex128 (n0, n1, n2) interleaved (the caller's seeded np.random draws), amp = sqrt(S(k))
 * float32, out float64; C order.  3-D inverse FFT by hipFFT (bound at first use). */
int sr_field_ifft_real(const double *noise, const float *amp, int n0, int n1, int n2, int normalise, double *out);
/* gaussian1D/2D/3D.cos (src/field_generator/gaussian{1,2,3}D.py): for every cell (i, j, l) of shape[ndim] (C order),
 *   out = sum_m amp[m] * sum_s cos(k[0][m]*x0[i] + sg1(s)*k[1][m]*x1[j] + sg2(s)*k[2][m]*x2[l] + phase[s][m]),
 * s over the reference's 2^(ndim-1) terms in its order (3-D: ++, +-, -+, -- with psi_1..psi_4; 2-D: +phi, -psi;
 * 1-D: +phi).  coords: per axis, the cell centres (shape[0] + ... + shape[ndim-1] values); k: ndim x nmodes;
 * amp: nmodes (A_m*sqrt(2)); phase: 2^(ndim-1) x nmodes.  float64 throughout; the sum over modes is in a fixed order,
 * so a repeated call returns the identical field.  Arguments are checked before the device is touched. */
int sr_field_modesum(int ndim, const int64_t *shape, const double *coords, int nmodes, const double *k,
                     const double *amp, const double *phase, double *out);
/* ---- the step after the path: radially binned power spectrum of a detector image -----------
 * radial_2Dspectrum (src/utils/power_spectrum.py:372-421): |fft2(img)|^2/(n0*n1)^2 summed and counted over the
 * wavenumber bins [edges[b], edges[b+1]); k0 (n0), k1 (n1): wavenumber of each index of the unshifted transform.
 * The 2-D case of sr_power_spectrum's edges rule. */
int sr_radial_spectrum2d(const double *img, int n0, int n1, const double *k0, const double *k1,
                         const double *edges, int n_edges, double *sum, uint64_t *count);
/* The power spectra of src/utils/power_spectrum.py (radial_*Dspectrum, scalar*D_fft, scalar*D_knyquist): one forward
 * Z2Z transform of a float64 field of ndim = 1, 2 or 3 axes (shape[ndim], C order; hipFFT, cached plan) and one pass
 * that bins every mode.  coords holds shape[0] + ... + shape[ndim-1] values: per axis, the coordinate of each index of
 * the UNSHIFTED transform; a NaN coordinate drops the mode.  Mode (i, j, l) has m = sqrt((a0[i]^2 + a1[j]^2) + a2[l]^2),
 * rounded as numpy rounds that expression, and power p = (re^2 + im^2) / norm.  rule:
 *   SR_SPECTRUM_EDGES: edges (n_bins + 1, ascending); sum[b], count[b] over edges[b] <= m < edges[b+1];
 *   SR_SPECTRUM_SHELL: edges unused; sum[k], count[k] over the shells rint(m) = k < n_bins; *overflow (may be NULL)
 *                      = the number of modes whose shell is >= n_bins (0 under the edges rule).
 * sum and count hold n_bins values; the caller divides (an empty bin is NaN there, as np.mean of nothing). */
#define SR_SPECTRUM_EDGES 0
#define SR_SPECTRUM_SHELL 1
int sr_power_spectrum(const double *field, int ndim, const int64_t *shape, const double *coords, int rule,
                      const double *edges, int n_bins, double norm, double *sum, uint64_t *count, uint64_t *overflow);

/* ---- after the path: Fresnel propagation of the traced field (src/simulator/fresnel_integral.py) -------------
 * Scatter to grid (fresnel_integral.py:69-78, propagate's two LinearNDInterpolators): the rays (rx[i], ry[i]) carry
 * amp[i] and phase[i]; node (j, i) of the (ny, nx) grid sits at (gx[i], gy[j]) (np.meshgrid(x, y)).  A node inside the
 * rays' convex hull gets the linear interpolation of amp and phase in the Delaunay triangle of all rays that holds it
 * (barycentric weights, float64), a node outside gets 0 -- scipy's LinearNDInterpolator(..., fill_value=0) evaluated at
 * every node, without building the triangulation.  Nodes on the hull's boundary, its vertices included, are inside, as
 * scipy treats them.  tri_out (may be NULL): the triangle's three ray indices per node,
 * ascending, (ny, nx, 3), -1 outside.  stats (may be NULL): SR_FRESNEL_STATS values (hull vertices, rays left by the hull
 * pre-filter, bins along x and y, nodes outside, nodes the second pass resolved).  Rays must have finite positions and be
 * at least 3 (checked before the device is touched); collinear rays span no triangle: every node is outside. */
#define SR_FRESNEL_STATS 6
int sr_fresnel_grid(int64_t n_rays, const double *rx, const double *ry, const double *amp, const double *phase, int nx,
                    const double *gx, int ny, const double *gy, double *amp_out, double *phase_out, int32_t *tri_out,
                    int64_t *stats);
/* fresnel_propagate (fresnel_integral.py:25-59) on an (m0, m1) complex128 field: forward 2-D Z2Z FFT, times
 * H = exp(-i pi_lz (fx^2 + fy^2)) (fx: m0 values, fy: m1), times exp(-psf (fx^2 + fy^2)) when psf > 0 (the LANEX PSF,
 * psf = 2 (pi sigma)^2), inverse FFT, times post (the caller folds numpy's 1/(m0 m1) into it), then the rows r0..r0+nr
 * and columns c0..c0+nc go to out (nr x nc complex128, interleaved). */
typedef struct {
  double pi_lz;            /* pi * wavelength * z */
  double psf;              /* 2 (pi sigma)^2, or 0: no PSF */
  double post_re, post_im; /* exp(i 2 pi z / wavelength) / (i wavelength z) / (m0 m1) */
  int32_t r0, nr, c0, nc;  /* the crop */
} sr_fresnel_params;
int sr_fresnel_propagate(const double *u0, int m0, int m1, const double *fx, const double *fy, const sr_fresnel_params *p,
                         double *out);
/* propagate (fresnel_integral.py:61-94) in one call: the rays gridded as sr_fresnel_grid does, U0 = amp exp(-i phase),
 * padded and windowed (prepare_field_for_propagation, :7-22): U[r][c] = U0[src0[r]][src1[c]] * (w0[r] * w1[c]) over the
 * (m0, m1) padded frame (src0, src1: numpy's reflect-pad source index of each padded row / column; w0, w1: the Tukey
 * windows), then propagated as sr_fresnel_propagate does.  stats (may be NULL) as sr_fresnel_grid's. */
int sr_fresnel_rays(int64_t n_rays, const double *rx, const double *ry, const double *amp, const double *phase, int nx,
                    const double *gx, int ny, const double *gy, const int32_t *src0, const int32_t *src1, const double *w0,
                    const double *w1, int m0, int m1, const double *fx, const double *fy, const sr_fresnel_params *p,
                    double *out, int64_t *stats);

/* ---- A2 + A3 + A4 + A6: ScalarDomain.solve / propagator.solve -----------------
 * replaces full_solver.py:376-403 (solve), :516-544 (dsdt), :317-347 (dndr, phase: the
 * RegularGridInterpolator gathers), :838-894 (ray_to_Jonesvector);
 * src/simulator/propagator.py:351-702 (solve), :94-175, :178-298.
 * Integrates ds/dt = dsdt(s) over [0, t_end] per ray with RK4 stepping from node plane to
 * node plane of the probing axis (`substeps` per cell), keeps the final state sf (at t_end,
 * as the reference), back-projects to the plane `extent` on the probing axis (rf) and forms
 * the Jones vector (Jf). */
#define SR_ROWS_LEGACY 0 /* y-probing rf rows (x, z): full_solver.py:866-872 */
#define SR_ROWS_JAX 1    /* y-probing rf rows (z, x): propagator.py:223-243 */
#define SR_PREC_F64 0
#define SR_PREC_MIXED 1
typedef struct {
  double t_end;         /* s; the reference uses sqrt(8)*extent/c (full_solver.py:381) */
  double extent;        /* m; exit plane coordinate for the back-projection */
  double dt;            /* s; step of the time-stepping fallback (rays the plane form cannot take);
                           <= 0 selects one probing-axis cell / c */
  int32_t probing_axis; /* 0 x, 1 y, 2 z; must equal the volume's */
  int32_t row_order;    /* SR_ROWS_* */
  int32_t substeps;     /* RK4 steps per cell (>= 1) */
  int32_t sort_rays;    /* bin rays by entry cell before the launch (results do not depend on it) */
  int32_t precision;    /* SR_PREC_F64: every operation float64 (differs from the oracle by fused
                           multiply-adds only).  SR_PREC_MIXED: float64 state, stage positions and
                           accumulation; float32 interpolation weights, blend and RK4 slopes (one step per
                           cell, no optional terms; otherwise the float64 kernels run) */
  int32_t handoff;      /* 0, or SR_HANDOFF_* when the volume is a slab of node planes (sr_volume_create_slab) */
} sr_trace_params;
#define SR_HANDOFF_ENTER 1 /* the rays' state arrives on the slab's first node plane (sr_rays_handoff_upload / _recv) */
#define SR_HANDOFF_EXIT 2  /* leave the state on the slab's last node plane for the next slab instead of sf / rf / Jf */

typedef struct {
  int64_t ray_steps;      /* RK4 steps taken, summed over rays */
  int64_t fallback_rays;  /* rays the first kernel passed on: precision f64 -> the time-stepping form; mixed -> the
                             float64 plane kernel (and from there, if not plane-form rays, the time-stepping form) */
  double trace_kernel_ms; /* HIP-event time of the plane-stepping kernel alone */
  double total_ms;        /* HIP-event time of the whole call on the stream */
} sr_trace_stats;

/* host buffers in and out (any of sf, rf, Jf, stats may be NULL) */
int sr_trace(const sr_volume *v, const double *s0, int64_t n_rays, const sr_trace_params *p,
             double *sf, double *rf, double *Jf, sr_trace_stats *stats);

/* A6 alone on a host (9, N) state: ray_to_Jonesvector (full_solver.py:838-894; propagator.py:178-298).
 * Jf may be NULL. */
int sr_ray_to_jones(const double *sf, int64_t n_rays, double extent, int probing_axis, int row_order,
                    double *rf, double *Jf);

/* device-resident form: rays stay in HBM between trace and deposit */
int sr_rays_create(sr_rays **out, int64_t n_rays);
int sr_rays_upload(sr_rays *r, const double *s0);                 /* (9, N) */
/* A bundle put together from several host chunks: s0 is (9, n) and becomes the rays first .. first + n - 1 of the bundle (rows at
 * the bundle's pitch N).  The reference's drivers trace chunks of 5e5 rays one after the other (pvti_trace_mpi.py:27, 144-163); a
 * GPU traces a dense bundle faster per ray, the rays are independent and the detector images are sums over rays, so the driver
 * merges consecutive chunks -- each still its own seeded draw -- into one bundle before the trace (run_trace.chunked_trace).  The
 * parts may come in any order and must cover 0 .. N - 1 between them; `last` != 0 on the final call: the launch positions' bounding
 * box is found over the whole bundle and the bundle counts as uploaded. */
int sr_rays_upload_part(sr_rays *r, const double *s0, int64_t n, int64_t first, int last);
/* The bundle drawn ON the device instead of uploaded: init_beam's distributions (full_solver.py:547-835; beam_type 0
 * 'circular' radius size_a, 1 'square' / 'rectangular' half-sizes size_a x size_b, 2 'linear' (:707-721: a line of
 * half-length size_a in x, angles in the x-z plane, launched at z = -ne_extent as written there), 3 'circular' with the JAX
 * generation's radial law np.random.power(2) (src/simulator/beam.py:66-77); launch plane -ne_extent on the probing
 * axis) from a counter-based Philox stream keyed by (seed, first_ray + ray index): reproducible across GPUs and chunk
 * sizes, but NOT NumPy's sample -- the host path (init_beam + sr_rays_upload) is the one that reproduces the reference's
 * seeded rays. */
int sr_rays_generate(sr_rays *r, int beam_type, double size_a, double size_b, double divergence, double ne_extent,
                     int probing_axis, uint64_t seed, uint64_t first_ray);
/* stats != NULL waits for the stream and reads the counters.  stats == NULL returns as soon as the work is queued and
 * the counters of this call are carried into the next one: a chunked driver passes NULL in its loop (no host round trip
 * per chunk) and reads the totals once with sr_rays_trace_stats. */
int sr_rays_trace(sr_rays *r, const sr_volume *v, const sr_trace_params *p, sr_trace_stats *stats);
/* ray_steps and fallback_rays summed over every trace of this bundle since its counters were last read (by this call
 * or by a trace with stats != NULL); the two times are those of the last trace.  Waits for the stream. */
int sr_rays_trace_stats(sr_rays *r, sr_trace_stats *stats);

/* Which kernel carried the last trace of the bundle: the number of node-plane segments of the tile path (trace_tile.inc:
 * dense float64 bundles -- >= 8 rays per lateral cell of the beam's bounding box, whole volumes and slabs, with or without
 * the optional terms -- the coefficient records of a lateral cell built once per workgroup in LDS; then
 * sr_trace_stats.trace_kernel_ms is the sum of its launches), or 0 for the per-ray kernels.  Same results either way. */
int sr_rays_tile_segments(const sr_rays *r);
/* 1 when that tile path ran the RECORDS kernel (round 5: the coefficient records ready-made in HBM, 128 bytes per node plane and
 * lateral cell, built with the volume's own arithmetic at the first such trace and brought into the tile's ring by LDS-DMA; four
 * workgroups per CU), 0 for the producers' kernel (records that do not fit in HBM, SYNTHRAY_TILE_RECORDS=0, the optional terms) or
 * when the tile path did not run.  Same results either way, bit for bit. */
int sr_rays_tile_records(const sr_rays *r);
/* The launch order of the bundle's last trace, read-only (for tests of the ray binning; never on a timed path): waits for the
 * library's stream and copies N uint32 to the host, order[j] = index (as uploaded) of the ray in launch slot j.  What it holds:
 *   - after a trace with sort_rays = 0: the identity;
 *   - after a trace with sort_rays = 1 on the per-ray kernels: the rays by the Morton key of their entry cell, rays outside the
 *     lateral grid and NaN rays last; on the tile path with ONE segment: by the band key of their entry cell;
 *   - after a tile-path trace of several segments: the order of the LAST segment's re-binning -- by the band key of the cell a ray
 *     is in on that segment's first node plane; rays the tiles have lost by then, and dead rays, last;
 *   - after a slab entry (SR_HANDOFF_ENTER): on the per-ray kernels the sender's order (row 9 of the records as they arrived); on
 *     the tile path the arrivals binned by the band key of the cell they arrive in (then as above when the slab has several segments).
 * The order of the rays inside one cell (one key) is not defined.  SR_ERR_STATE before any trace (a slab entry is one) has been
 * queued for the bundle; N = 0 copies nothing. */
int sr_rays_launch_order(const sr_rays *r, uint32_t *order);
/* The lateral cells the tile path's LAST binning found for the rays, read-only (for tests; never on a timed path): waits for the
 * library's stream and copies N uint32, each ib | ic << 16 (cell indices along the volume's axes b = (axis + 1) % 3 and
 * c = (axis + 2) % 3), 0xFFFFFFFF for a ray outside the lateral grid or dead.  The tile kernel places its tiles from these words
 * instead of searching again.  Entry k belongs to
 *   - the ray with index k (as uploaded), where it meets the entry plane, after a tile-path trace of ONE segment from s0;
 *   - place k of the records the last segment was binned from, after a trace of several segments or a slab entry.
 * SR_ERR_STATE while the bundle has not been traced on the tile path since it was made / resized. */
int sr_rays_binned_cells(const sr_rays *r, uint32_t *cells);
/* The bundle holds n rays from now on, 0 <= n <= the count it was created with (its capacity; SR_ERR_INVALID otherwise): what
 * sr_trace's pipeline does for a shorter last chunk.  Every device buffer keeps its size; the rows of s0 and of the results are at
 * pitch n afterwards, so whatever the bundle held (rays, results, hand-off records, bounding box, launch order) is forgotten:
 * upload or generate again. */
int sr_rays_set_count(sr_rays *r, int64_t n);
/* The density from which sr_rays_trace takes the tile path: rays per lateral cell of the beam's bounding box (sr_rays_get_bbox).
 * What a job that cuts its rays into chunks sizes them by (distributed.plan_chunks: the slab pipeline's chunk is the smallest
 * that every rank still traces with the tile kernel; the reference's drivers use a fixed 5e5, pvti_trace_mpi.py:27). */
double sr_tile_min_density(void);
int sr_rays_download(const sr_rays *r, double *sf, double *rf, double *Jf); /* original ray order */
int sr_rays_download_s0(const sr_rays *r, double *s0);            /* the bundle as uploaded / generated, (9, N) */
/* Per ray (original order), a bound [rad] on how far the exit angles of the last trace may be from the SR_PREC_F64
 * build's: 0 for rays a float64 kernel wrote (SR_PREC_F64, the mixed build's second level, rays an exact-counts deposit
 * has traced again, SR_PREC_MIXED with sub-steps or optional terms: the float64 kernels ran), the mixed kernel's own estimate
 * otherwise (8 * 2^-24 * [sum of |lateral velocity changes| + sum over node planes of h * largest |bilinear coefficient| / v_a]
 * / v_a: trace_mx.inc).  Positions: the bound times the volume's length along the
 * probing axis plus the distance from its last node plane to the plane `extent`.  This is what sr_deposit_params.exact_counts
 * works from. */
int sr_rays_error_bound(const sr_rays *r, float *bound);
int64_t sr_rays_count(const sr_rays *r);
/* A12 hand-off records, (10, N) float64 in launch order: p_b, p_c, v_a, v_b, v_c, phase, t, amp, pol, ray index
 * (the plane form's state on the shared node plane; v_a = NaN: ray lost).  Written by a trace with
 * SR_HANDOFF_EXIT, consumed by a trace with SR_HANDOFF_ENTER; between GPUs they travel host-side
 * (download / upload) or device to device over RCCL (send / recv, on the library stream). */
int sr_rays_handoff_download(const sr_rays *r, double *rec);
/* The bounding box of the BEAM a bundle's rays belong to, (min x, y, z, max x, y, z) of their launch positions [m]: what the
 * library judges the ray density by when it picks the kernel (rays per lateral cell of the beam, trace.hip: tile_plan).  It is
 * found at sr_rays_upload / known from the parameters at sr_rays_generate; rays that ARRIVE by hand-off (sr_rays_handoff_upload /
 * _recv: ranks > 0 of a slab pipeline, the reference's region loop propagator.py:366-452) have none and are judged by the whole
 * lateral grid -- unless the caller, who knows which beam the job traces, says so here: a box given with sr_rays_set_bbox stays
 * with the bundle across hand-offs until the next upload / generate (bbox = NULL takes it back).  sr_rays_get_bbox: *known = 0
 * when the bundle has no box. */
int sr_rays_set_bbox(sr_rays *r, const double *bbox);
int sr_rays_get_bbox(const sr_rays *r, double *bbox, int *known);
int sr_rays_handoff_upload(sr_rays *r, const double *rec);
int sr_rays_handoff_send(sr_rays *r, sr_comm *comm, int peer);
int sr_rays_handoff_recv(sr_rays *r, sr_comm *comm, int peer);
void sr_rays_destroy(sr_rays *r);

/* ---- A7 + A8: ray-transfer-matrix optics --------------------------------------
 * replaces src/solvers-legacy/rtm_solver.py:48-136 (m_to_mm, lens, distance, apertures) and
 * the chains :197-286, :376-422; src/simulator/diagnostics.py:122-245, :388-481, :614-638.
 * r is (4, N) in mm.  A rejected ray becomes a NaN column.  kwave > 0 also propagates the
 * field: after every SR_OP_DIST, E *= exp(1j*kwave*sqrt(dx^2+dy^2)) (rtm_solver.py:380-418). */
enum {
  SR_OP_DIST = 0,      /* a = d:  x += d*theta, y += d*phi; iarg = 1: without the field factor (see sr_optics) */
  SR_OP_LENS = 1,      /* a = f1, b = f2: theta -= x/f1, phi -= y/f2 */
  SR_OP_CIRC_AP = 2,   /* a = R: reject x^2+y^2 > R^2 */
  SR_OP_CIRC_STOP = 3, /* a = R: reject x^2+y^2 < R^2 */
  SR_OP_RECT_AP = 4,   /* a = Lx, b = Ly: reject x^2 > Lx^2 AND y^2 > Ly^2 (rtm_solver.py:114-117) */
  SR_OP_KNIFE = 5,     /* a = offset, b = direction (>0 rejects above, <0 below), iarg = row (0 x, 2 y) */
  SR_OP_SCALE = 6,     /* a = s: x *= s, y *= s  (m_to_mm: s = 1e3, rtm_solver.py:48-51; mm_to_m: 1e-3) */
  SR_OP_PHASE = 7      /* a = d: the field factor of SR_OP_DIST(d) without moving the ray (diagnostics.py:505-511) */
};
typedef struct {
  int32_t op;
  int32_t iarg;
  double a;
  double b;
} sr_optic;
#define SR_MAX_OPTICS 32
int sr_optics(const sr_optic *chain, int n_ops, double kwave, int64_t n_rays, const double *r_in,
              const double *E_in, double *r_out, double *E_out);

/* ---- A9: Rays.histogram (np.histogram2d) --------------------------------------
 * replaces rtm_solver.py:156-178, diagnostics.py:323-353.  Exact integer counts,
 * H[ny_bins][nx_bins]; numpy's edge rules (linspace edges, right-open bins, last edge closed,
 * NaN and outliers dropped). */
int sr_hist2d(const double *x, const double *y, int64_t n_rays, int nx_bins, int ny_bins,
              double x_lo, double x_hi, double y_lo, double y_hi, uint32_t *H);

/* ---- A10: Interferometry.interferogram ----------------------------------------
 * replaces rtm_solver.py:424-453, diagnostics.py:358-379.  n?_edges = pix // bin_scale edges,
 * n?_edges-1 bins, idx = digitize-1 (right edge open); amp is [2][ny_edges-1][nx_edges-1]
 * complex128: the per-pixel sums of E_x and E_y before H = sqrt(Re(Ax)^2 + Re(Ay)^2). */
int sr_interferogram(const double *x, const double *y, const double *E, int64_t n_rays,
                     int nx_edges, int ny_edges, double x_lo, double x_hi, double y_lo,
                     double y_hi, double *amp /* may be NULL */, double *H /* may be NULL: [ny-1][nx-1] */);

/* ---- A11: Interferometry.interfere_ref_beam (diagnostics.py:559-581) ----------- */
int sr_interfere_ref_beam(const double *x, const double *y, int64_t n_rays, double n_fringes,
                          double deg, double *E /* (2, N) complex128, in place */);

/* ---- fused, device-resident deposit -------------------------------------------
 * trace output (rf, Jf in HBM) -> m_to_mm -> [reference beam] -> optic chain -> image. */
#define SR_IMG_COUNTS 0  /* uint32 [ny][nx], A9 binning; nx, ny = number of bins */
#define SR_IMG_COMPLEX 1 /* float64 [2][ny-1][nx-1][2], A10 binning; nx, ny = number of EDGES */
int sr_image_create(sr_image **out, int kind, int nx, int ny, double x_lo, double x_hi,
                    double y_lo, double y_hi);
int sr_image_zero(sr_image *img);
int sr_image_download(const sr_image *img, void *host); /* uint32 or float64 buffer, see kind */
/* SR_IMG_COUNTS only: the counts as float64 [ny][nx] -- the dtype np.histogram2d hands back (rtm_solver.py:171-174);
 * converted on the device, so the host does not pay an astype over the 8.9e6 pixels of the default detector */
int sr_image_counts_f64(const sr_image *img, double *H);
/* SR_IMG_COMPLEX only: H = sqrt(Re(Ax)^2 + Re(Ay)^2), [ny-1][nx-1] float64 (rtm_solver.py:450) */
int sr_image_amplitude(const sr_image *img, double *H);
int64_t sr_image_bytes(const sr_image *img);
void sr_image_destroy(sr_image *img);

#define SR_MAX_REF_BEAMS 4
typedef struct {
  double kwave;         /* > 0: propagate E through the chain (interferometry) */
  /* reference beams (A11, diagnostics.py:559-581) added to E_y before the chain, in this order: the first ref_on entries.
   * The JAX generation's two_lens_solve adds (10, 20) by itself (diagnostics.py:616) after whatever the caller added. */
  double ref_n_fringes[SR_MAX_REF_BEAMS];
  double ref_deg[SR_MAX_REF_BEAMS];
  int32_t ref_on;       /* number of reference beams, 0..SR_MAX_REF_BEAMS */
  int32_t lds_tiles;    /* 1: LDS-privatised detector tiles; 0: global atomics only */
  int32_t exact_counts; /* SR_IMG_COUNTS, rays traced with SR_PREC_MIXED on a whole volume: 1 (the default with p == NULL) =
                           every ray whose bin, or the decision of a mask of the chain, could differ from the float64
                           build's inside the tracer's per-ray error bound is traced AGAIN in float64 (from s0, same
                           slots of sf / rf / Jf) and counted after that: the image equals the SR_PREC_F64 image integer
                           for integer (np.histogram2d of the reference's rays, rtm_solver.py:156-178).  Needs the
                           volume of that trace to be alive.  0 = count the mixed build's coordinates as they are. */
  int32_t reserved;
} sr_deposit_params;
typedef struct {
  double kernel_ms;     /* HIP-event time of the deposit (with exact_counts: the re-trace included) */
  int64_t deposited;    /* rays that landed inside the detector */
  int64_t retraced;     /* exact_counts: rays traced again in float64 by this deposit */
} sr_deposit_stats;
int sr_rays_deposit(const sr_rays *r, const sr_optic *chain, int n_ops, const sr_deposit_params *p,
                    sr_image *img, sr_deposit_stats *stats);
/* The same front end without the detector: exit-plane rays in HBM -> m_to_mm -> [reference beams] -> chain, written to HOST
 * arrays in the ORIGINAL ray order -- what Rays.rf (rtm_solver.py:197-286) / Diagnostic.rf, .Jf (diagnostics.py:388-481,
 * 614-638) hold after a *_solve().  The mirror classes keep the bundle ScalarDomain.solve left in HBM, deposit from it
 * (sr_rays_deposit) and call this only when a caller READS .rf / .rE.  n_ops == 0: r0 = m_to_mm(rf) itself.  p: kwave and
 * the reference beams (may be NULL); E_out (2, N) complex128 may be NULL. */
int sr_rays_optics(const sr_rays *r, const sr_optic *chain, int n_ops, const sr_deposit_params *p,
                   double *rf_out, double *E_out);
/* The edge guard of exact_counts for SEVERAL counts diagnostics at once: every ray of a mixed-precision trace whose bin or
 * mask decision is uncertain for ANY of the n_diag (chain, image) pairs is traced again in float64, ONE re-trace for all of
 * them (a re-trace costs the latency of a whole trace however few rays it holds).  Afterwards those rays carry bound 0, so
 * the deposits that follow find nothing left to refine, with exact_counts = 1 or 0.  Complex images are skipped.  A trace
 * in SR_PREC_F64 needs none: the call returns at once.  *retraced (may be NULL): rays traced again. */
#define SR_MAX_REFINE 4
int sr_rays_refine(const sr_rays *r, int n_diag, const sr_optic *const *chains, const int *n_ops,
                   sr_image *const *imgs, int64_t *retraced);

/* ---- polarimetry: analyser-weighted intensity images of the traced rays ---------
 * None of these entries has a reference counterpart: the reference forms the exit Jones vector
 * E = amp*exp(i*phase)*(-sin pol, cos pol) (full_solver.py:838-894) and shows it through counts and coherent sums only.
 * An ANALYSER at angle beta (from the y axis, in the sense `pol` is measured) has the transmission axis
 * (a, b) = (-sin beta, cos beta); a ray's weight in that channel is
 *   w = |a E_x + b E_y|^2 = (a Re E_x + b Re E_y)^2 + (a Im E_x + b Im E_y)^2     (= amp^2 cos^2(pol - beta)),
 * and a channel given as (NaN, NaN) has no analyser: w = |E_x|^2 + |E_y|^2 (the attenuation image).  a and b are formed
 * by the caller in float64 and passed down, so host and device work with the same two numbers. */
#define SR_IMG_INTENSITY 2 /* float64 [n_ch][ny][nx], A9 binning; nx, ny = number of bins */
#define SR_MAX_ANALYSERS 4
/* no reference counterpart: an image I[c][iy][ix] = sum of w_c over the rays of pixel (iy, ix), np.histogram2d's binning
 * (the geometry of SR_IMG_COUNTS).  sr_image_zero / _download (float64 buffer) / _bytes / _destroy / _reduce (float64 sum)
 * take it as they take the other kinds. */
int sr_image_create_intensity(sr_image **out, int n_ch, int nx, int ny, double x_lo, double x_hi,
                              double y_lo, double y_hi);
/* no reference counterpart: I += sum of w over the bundle's rays the masks of the chain leave un-rejected; exit rays in
 * HBM -> m_to_mm -> chain (masks and geometry only: the sum is incoherent, the field factors of its legs have modulus 1
 * and no reference beam is added) -> np.histogram2d's bin -> up to SR_MAX_ANALYSERS channels in one pass.  lds_tiles as in
 * sr_deposit_params.  No edge guard: intensities are floating-point sums, a mixed-precision bundle is binned as it is.
 * Errors: bundle not traced, bundle traced without Jf, n_ch different from the image's. */
int sr_rays_deposit_intensity(const sr_rays *r, const sr_optic *chain, int n_ops,
                              const double *analyser_ab /* [n_ch][2] = (a, b); NaN, NaN = no analyser */, int n_ch,
                              int lds_tiles, sr_image *img, sr_deposit_stats *stats);
/* no reference counterpart: the host-array form of the same sums (as sr_hist2d is to the counts image): x, y are
 * detector-plane coordinates (NaN: rejected), E (2, N) complex128, I [n_ch][ny_bins][nx_bins] float64 (overwritten). */
int sr_intensity2d(const double *x, const double *y, const double *E, int64_t n_rays, const double *analyser_ab, int n_ch,
                   int nx_bins, int ny_bins, double x_lo, double x_hi, double y_lo, double y_hi, double *I);
/* no reference counterpart: the rotation map of two channels at +beta and -beta, 0 < beta < pi/2:
 *   D = (I+ - I-)/(I+ + I-), R = hypot(sin 2beta, D cos 2beta), delta = atan2(D cos 2beta, sin 2beta),
 *   alpha = (delta + asin(D/R))/2, NaN where I+ + I- == 0; unambiguous for |alpha| < min(beta, pi/2 - beta);
 * beta = pi/4: alpha = asin(D)/2. */
int sr_image_rotation(const sr_image *img, int ch_plus, int ch_minus, double beta, double *alpha /* [ny][nx] */);

/* ---- ray-sharded multi-GPU: sum of the per-GPU images (RCCL over xGMI) ---------
 * replaces comm.reduce(sh.H, root=0, op=MPI.SUM): examples/jobs/run_scripts/pvti_trace_mpi.py:169-170,
 * interference_MPI.py:189.  The 128-byte id is made on rank 0 and handed to the other ranks by the
 * caller's launcher (synthpy_amd/_rendezvous.py: a TCP rendezvous over MASTER_ADDR:MASTER_PORT, no torch). */
#define SR_COMM_ID_BYTES 128
int sr_comm_unique_id(void *id128);
int sr_comm_create(sr_comm **out, const void *id128, int rank, int n_ranks);
int sr_image_reduce(sr_image *img, sr_comm *comm, int root); /* in place; root < 0: all-reduce */
/* what the communicator itself reports (ncclCommUserRank / ncclCommCount): the mpi4py analogue is comm.Get_rank() /
 * comm.Get_size(), pvti_trace_mpi.py:24-25 */
int sr_comm_ranks(const sr_comm *comm, int *rank, int *n_ranks);
void sr_comm_destroy(sr_comm *comm);

#ifdef __cplusplus
}
#endif
#endif /* SYNTHRAY_H */
