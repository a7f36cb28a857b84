// Included by trace.hip inside its anonymous namespace, after trace_f64.inc (needs CoefPlane, coefs_from_corners, fma3,
// rcp_f64_from_f32, rcp_refine, hi_word, VolDev, TraceArgs, StepTab64, write_outputs, queue_push).
//
// k_trace_tile: k_trace_f64's arithmetic with the per-(lateral cell, node plane) work done ONCE -- per workgroup (the producers'
// kernel, round 3) or per volume (the RECORDS kernel, round 5: template parameter REC, the default wherever the records fit in HBM).
//
// What k_trace_f64 spends per ray and step that is the same for every ray of a cell (76 rays share a cell on BASELINE
// config 3): the new plane's four corner records are loaded, converted to float64 and turned into bilinear coefficients
// (20 conversions + 20 additions), the mid-step plane LO + HI is formed (16 additions), and a cell change re-reads and
// re-converts two planes.  Here a workgroup of SR_TILE_THREADS = 256 rays (four wavefronts) owns a TILE of TB x TC lateral cells
// placed on the box of its rays' predicted paths and keeps, in LDS, the float64 coefficient records of the node planes it is
// working between:
//
//     plane ring (3 slots: node planes k, k+1, and k+2 being written) + mid ring (2 slots: LO + HI of step k, and of step
//     k+1 being written), one record of 16 float64 = {a[4], b[4], c[4], d[4]} per cell and slot.
//
//  * THE RECORDS KERNEL (REC; 8 x 7 tiles, 39 KB of LDS, 128 registers: FOUR workgroups per CU, four wavefronts per SIMD).  The
//    node planes' records are ready-made in HBM (sr_volume::R: k_build_records forms them once per volume with
//    coefs_from_corners -- 128 bytes per node plane and lateral cell, 17 GB for 512^3) and come into the ring by LDS-DMA: at a
//    step's start each of the four wavefronts asks for two tile columns of node plane k+2 (2 x global_load_lds_dwordx4: one
//    kilobyte each, no register, no conversion; the sources are running pointers in scalar registers, one node plane further per step), at its end it adds them
//    to its own two columns of plane k+1 for the mid record (the same lane-linear kilobytes: 4 ds_read_b128 + 4 v_add_f64 + 2
//    ds_write_b128, every lane busy).  No producer wavefront: the four wavefronts of a workgroup do the same work.  LDS
//    layout: see kRecColD (piece-major column blocks 1104 bytes apart: the DMA writes a wavefront's 64 x 16 bytes contiguously, so
//    the padding of the producers' layout is not to be had; the swizzle goes on the SOURCE address).  Measured on BASELINE
//    config 3 (profiles/r05_*): 41.2 ms in the kernels against the producers' 45.0 (round 4: 45.2), VALU busy 0.74 against 0.65.
//  * THE PRODUCERS' KERNEL (8 x 8 tiles, records 144 bytes apart -- 128 + 16: consecutive cells start 4 banks apart --, 46 KB,
//    164 registers: three workgroups per CU) runs where the records do not fit (a third of the free HBM at most), with
//    SYNTHRAY_TILE_RECORDS=0, with tiles that are not eight rows high, and -- AUX -- with the optional terms:
//  * PRODUCERS: the workgroup's first TB*TC lanes (one wavefront at 8 x 8) own one cell each.  At the start of step k they
//    request the four corner records of node plane k+2 (exactly k_trace_f64's loads), at its end they form the coefficients
//    (coefs_from_corners: the same function, the same values), re-read their cell's record of plane k+1 from LDS, and store
//    plane k+2 and the mid record (k+1) + (k+2).  One barrier per step separates a slot's last reader from its next writer.
//  * CONSUMERS: every lane carries one ray, as in k_trace_f64, but holds NO plane in registers: a stage reads the record of
//    its cell from the slot it needs (stage 1: plane k; 2, 3: mid; 4: plane k+1) -- 8 ds_read_b128, requested one stage ahead.
//    A cell change is an index change: the rarely-taken region finds the new cell in the tile's node table (the neighbour the
//    weight points at, accepted when g[i] <= q < g[i+1]: SciPy's find_indices rule) and costs no global load, no conversion.
//  * The arithmetic of a stage, the order of its operations and every constant are k_trace_f64's, so a ray's result is the
//    same bit for bit whichever kernel carried it.  Tests (-m gpu): THIS kernel forced (SYNTHRAY_F64_TILE=1, tile_segments
//    asserted) against the oracle and the reference's fixtures -- test_trace_vs_oracle[...-1-1], test_trace_vs_reference_tight
//    [f64-1-...], test_interferometry_end_to_end_from_s0_f64[1-...], test_non_uniform_grid_vs_oracle -- chosen by the library
//    itself on a dense bundle against the oracle (test_c3_shaped_dense_bundle_takes_the_tile_path_by_itself_vs_oracle), and
//    against k_trace_f64 bit for bit (test_tile_kernel_is_bit_identical_to_the_per_ray_kernel).
//  * A ray that leaves the tile (or the volume: the virtual cells of k_trace_f64 are not kept here), or turns around, is LOST
//    to the tile path for good -- a STRAGGLER: the state it entered the segment with (first segment: formed again from s0) is
//    appended to the bundle's straggler records, its own record is marked gone (v_a = -inf, row 0 = the entry's index), and
//    k_trace_f64 -- stepping a range of node planes from and to records (TraceArgs.k_first / k_last) -- carries that segment's
//    new entries from the segment's first plane to the END of the volume (slab) on the library's SIDE stream, beside the tile
//    kernel's remaining segments; k_strag_finish, after the last segment, forms the outputs (or the slab's exit records) of the
//    gone slots from the entries.  (Until round 5 k_trace_f64 carried a segment's lost rays through that segment's planes only,
//    between two tile launches on the same stream, and they were binned again with the rest: four serial launches of a few
//    hundred microseconds each on BASELINE config 3, and rays on their way out of the beam were lost again in every segment.)
//    The tile is sized so that this is rare: rays diffuse laterally (3.6 cells rms over 511 planes on config 3), so the volume is
//    traced in SEGMENTS of node planes (four on config 3, the first 1.3 / 0.7 times as long as the last: trace.hip,
//    tile_cut_weights); between segments the rays' state goes through the A12 hand-off
//    records and the rays are binned again by their current cell (host side: trace_tiled) -- the kernel reads its rays' records
//    THROUGH the new order (rec_in[order[j]]) and writes them in place j of the other buffer: no gather pass.
//
// Ray order: bands of `band` cell rows along b, inside a band by column c (alternating direction from band to band), inside
// a column by row: 256 consecutive rays cover band x (256 / (band * rays per cell)) cells -- a compact rectangle whatever
// the position, where a Morton run can straddle two distant blocks.
struct TileGeom {
  int tb, tc;       // tile size in cells (rows along b, columns along c)
  int halo;         // cells between the workgroup's first entry cell and the tile's edge
  int band;         // rows per band of the ray order
};

struct TileArgs {
  TraceArgs A;
  TileGeom G;
  int k0, k1;       // this launch steps from node plane k0 to node plane k1 (indices of the volume's -- or the slab's -- own planes)
  int first, last;  // first: state from s0 (else from the hand-off record); last: the volume's (slab's) last segment
  // A12: a slab of node planes (sr_volume_create_slab).  exit_rec: on the last segment the state stays in the hand-off record for
  // the next slab (SR_HANDOFF_EXIT) instead of becoming sf / rf / Jf; slab: there are no further levels (a slab holds only its own
  // planes): a ray the plane form cannot finish comes out NaN, as from k_trace_f64 on a slab
  int exit_rec, slab;
  int rot;          // 1: the producers' wavefront rotates with the workgroup index (see `producer` in the kernel).  The host sets 0
  // A launch may take a RANGE of the bundle's workgroups: block0 = the first one, A.n_blocks = how many.  The host always sets 0
  // and every workgroup: both experiments were measured and ended (docs/HISTORY.md); the arguments stay until the kernel is next timed
  unsigned block0;
  // Not the first segment: the state comes from rec_in[row][order[j]] (the records the segment before wrote -- or a slab's
  // arrivals -- read through the order of the new binning); A.rec is the OTHER buffer, written in place j; perm_out[j] = the
  // ray's index (row 9)
  const double *rec_in;
  const uint32_t *order;
  uint32_t *perm_out;
  // the packed cell (k_keys_band / k_keys_band_rec) of every ray on node plane k0, where the binning before this launch found it: by
  // the ray's index (first) or by its place in rec_in -- read through perm / order as the state is
  const uint32_t *cells;
  // the rays this launch loses (they left their tile, or the volume): appended to the straggler records, (10, strag_cap),
  // *strag_count entries so far -- the state they entered this segment with; k_trace_f64 takes them from there (see the header)
  double *strag_rec;
  int64_t strag_cap;
  unsigned long long *strag_count;
};

// doubles per (cell, slot) record in LDS: 16 coefficients + 2 of padding (144 bytes); with the optional terms' five fields
// (AUX: kappa, n_e, B) 20 more: 38 (304 bytes: consecutive cells 12 banks apart)
// (REC: the records arrive by LDS-DMA, which writes a wavefront's 64 x 16 bytes contiguously: a tile column -- eight cells, one
// kilobyte -- is one block, and inside a block the layout is PIECE-major: 16-byte piece p (0..7: a01 a23 b01 b23 c01 c23 d01 d23)
// of the column's record r (0..7) sits at (p * 8 + r) * 16 bytes, so that the same piece of the eight rows is 128 contiguous
// bytes (no two rows on the same banks) and a record's pieces are 128 bytes apart (immediate offsets of one address).  The
// blocks are 1024 + 80 bytes apart: cells (r, c) and (r', c') share their banks only when r - r' = 5 (c' - c) mod 16 -- five rows
// and one column apart, which the rays of a wavefront are not.  With the records 128 bytes apart in plain order, 39 % of the
// LDS's active cycles were bank conflicts (profiles/r05_pmc_c3_f64_first_layout.csv): a wavefront's rays are in four to six cells
// by the end of a segment.)
constexpr int kRecColD = (1024 + 80) / 8;  // doubles from one column block to the next
__host__ __device__ constexpr int tile_rec(bool aux, bool rec = false) { return aux ? 38 : (rec ? 16 : 18); }

// The tile's node tables, one per lateral axis: entry n = {g[n], 1 / (g[n+1] - g[n])} of the tile's n-th node, 16 bytes, so that a
// cell's g[n], r[n] and g[n+1] are ONE address with immediate offsets.  Entries kTabLo below node 0 and kTabHi from node T on are
// SENTINELS that make the cell search's acceptance test g[n] <= q < g[n+1] fail without a clamp of the index (relocate2):
//   n < 0: {+inf, 1} -- q - g[n] is negative (or NaN);   n = T: {g[T], 1}, and n > T: {-inf, 1} -- q < g[n+1] is false.
// A ray that failed the test is lost to the launch, but finishes its step: each of the step's further searches may move its index
// on by one (three more at the most), so there are four sentinels on either side and every read stays inside the table.
constexpr int kTabLo = 4, kTabHi = 5;
__host__ __device__ constexpr int tile_tab_entries(int t) { return kTabLo + t + kTabHi; }
// REC: the tables lie where those of the largest tile (8 x 8) would, so that their LDS addresses are constants of the kernel
// + the placement's scratch: the bounds of each wavefront's cells, four packed words per wavefront, 16 wavefronts at the most (see
// `box` in the kernel)
__host__ __device__ constexpr int tile_tab_doubles(int tb, int tc) { return 2 * tile_tab_entries(tb) + 2 * tile_tab_entries(tc) + 32; }
static_assert(tile_tab_doubles(8, 8) * sizeof(double) <= 1024, "the records kernel's table head is one KiB");

__host__ __device__ inline size_t tile_lds_bytes(const TileGeom &g, int seg_steps, bool aux = false, bool rec = false) {
  const size_t tables = (size_t)(rec ? tile_tab_doubles(8, 8) : tile_tab_doubles(g.tb, g.tc));
  (void)seg_steps;  // (the step table was in LDS until the constants came by scalar loads)
  // REC: the records start on a 1 KiB boundary of the workgroup's LDS (a tile column of one slot = one DMA's kilobyte)
  const size_t head = rec ? (((tables * sizeof(double)) + 1023) & ~(size_t)1023) / sizeof(double) : ((tables + 1) & ~(size_t)1);
  if (rec) return sizeof(double) * (head + (size_t)5 * g.tc * kRecColD);  // a slot = tc column blocks (see kRecColD)
  return sizeof(double) * (head + (size_t)5 * g.tb * g.tc * tile_rec(aux, rec));
}

// Two uint16 in a word, minimum / maximum of each half (v_pk_min_u16 / v_pk_max_u16), and their reduction over a wavefront in
// registers: four DPP steps inside a row of 16 lanes (the quad's two exchanges, the half row's and the row's mirror), then row 0
// into row 1 and row 2 into row 3 (row_bcast:15), rows 0-1 into rows 2-3 (row_bcast:31).  LANE 63 holds the wavefront's result.
// Every lane of the wavefront must be active.
typedef unsigned short pk_u16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_min_u16(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(pk_u16, a), __builtin_bit_cast(pk_u16, b)));
}
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(pk_u16, a), __builtin_bit_cast(pk_u16, b)));
}
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned dpp_from(unsigned v) {  // lanes of the rows not in ROWS keep their own value
  return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWS, 0xf, false);
}
template <bool MAX>
__device__ __forceinline__ unsigned wave_pk_u16(unsigned v) {
  auto op = [](unsigned a, unsigned b) { return MAX ? pk_max_u16(a, b) : pk_min_u16(a, b); };
  v = op(v, dpp_from<0xB1, 0xf>(v));   // quad_perm:[1,0,3,2]
  v = op(v, dpp_from<0x4E, 0xf>(v));   // quad_perm:[2,3,0,1]
  v = op(v, dpp_from<0x141, 0xf>(v));  // row_half_mirror
  v = op(v, dpp_from<0x140, 0xf>(v));  // row_mirror
  v = op(v, dpp_from<0x142, 0xa>(v));  // row_bcast:15 into rows 1 and 3
  v = op(v, dpp_from<0x143, 0xc>(v));  // row_bcast:31 into rows 2 and 3
  return v;
}

// the key of the band order (see the header); cells outside the volume / dead rays: `oob`
__device__ __forceinline__ uint32_t band_key(int ib, int ic, int ncc, int band) {
  const int bnd = ib / band, row = ib - bnd * band;
  const int col = (bnd & 1) ? ncc - 1 - ic : ic;
  return ((uint32_t)bnd * (uint32_t)ncc + (uint32_t)col) * (uint32_t)band + (uint32_t)row;
}

// shift: low key bits dropped (bin_by_band: band keys past what the LDS counters of the sort hold)
// cells: the cell itself beside its key, packed (ib | ic << 16; kNoCell: outside the volume / dead) -- the tile kernel places its
// tile from it instead of searching again (bin_by_band refuses lateral grids of more than 65535 cells a side)
constexpr uint32_t kNoCell = 0xFFFFFFFFu;
__global__ void k_keys_band(VolDev V, const double *__restrict__ s0, int64_t N, int axis, int band, uint32_t oob_key, int shift,
                            uint32_t *__restrict__ keys, uint32_t *__restrict__ cells) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int b = (axis + 1) % 3, c = (axis + 2) % 3;
  double pa = s0[axis * N + i], pb = s0[b * N + i], pc = s0[c * N + i];
  const double va = s0[(3 + axis) * N + i], vb = s0[(3 + b) * N + i], vc = s0[(3 + c) * N + i];
  const double ga0 = V.g[0][0];
  if (va > 0 && pa < ga0) {  // where the ray meets the entry plane
    const double tau = (ga0 - pa) / va;
    pb = pb + vb * tau;
    pc = pc + vc * tau;
  }
  const double gb0 = V.g[1][0], gbL = V.g[1][V.nb - 1], gc0 = V.g[2][0], gcL = V.g[2][V.nc - 1];
  uint32_t key = oob_key, cell = kNoCell;
  if (pb >= gb0 && pb <= gbL && pc >= gc0 && pc <= gcL) {
    const int ib = find_cell(V.g[1], V.nb, pb, gb0, V.rb0);
    const int ic = find_cell(V.g[2], V.nc, pc, gc0, V.rc0);
    key = band_key(ib, ic, V.nc - 1, band) >> shift;
    cell = (uint32_t)ib | ((uint32_t)ic << 16);
  }
  keys[i] = key;
  cells[i] = cell;
}

// between two segments: the key of a ray's CURRENT cell, from its hand-off record (rows 0, 1 = p_b, p_c; row 2 = v_a; NaN: not a
// plane-form ray, -inf: a straggler, gone from the tile path -- both sort behind every cell)
__global__ void k_keys_band_rec(VolDev V, const double *__restrict__ rec, int64_t N, int band, uint32_t oob_key, int shift,
                                uint32_t *__restrict__ keys, uint32_t *__restrict__ cells) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= N) return;
  const double pb = rec[j], pc = rec[N + j], va = rec[2 * N + j];
  const double gb0 = V.g[1][0], gbL = V.g[1][V.nb - 1], gc0 = V.g[2][0], gcL = V.g[2][V.nc - 1];
  uint32_t key = oob_key, cell = kNoCell;
  if (va > 0 && pb >= gb0 && pb <= gbL && pc >= gc0 && pc <= gcL) {
    const int ib = find_cell(V.g[1], V.nb, pb, gb0, V.rb0);
    const int ic = find_cell(V.g[2], V.nc, pc, gc0, V.rc0);
    key = band_key(ib, ic, V.nc - 1, band) >> shift;
    cell = (uint32_t)ib | ((uint32_t)ic << 16);
  }
  keys[j] = key;
  cells[j] = cell;
}

// after a segment's launch: how many straggler entries there are now (what the segment's k_trace_f64 launch on the side stream
// takes: [snap[q], snap[q + 1])), added to the trace's count of rays past the first kernel
__global__ void k_strag_snap(const unsigned long long *count, unsigned long long *snap, int q, unsigned long long *total) {
  const unsigned long long c = *count;
  snap[q + 1] = c;
  *total += c - snap[q];
}

// After the last segment, once the side stream's launches are done: every gone slot (record row 2 = -inf, row 0 = its entry in
// the straggler records) gets what its straggler ended with -- the state on the last node plane as k_trace_f64 left it in the
// entry (NaN: the plane form could not finish it).  exit_rec: a slab hands that state on (rows 0..8 into the record; row 9, the
// ray's index, is there already).  Otherwise the outputs, by the expressions of k_trace_f64's own tail: vacuum to t_end, sf / rf /
// Jf; a ray that is not finished goes the way the tile kernel's own rejects go (the usual levels from s0; NaN on a slab).
struct StragFinish {
  TraceArgs A;  // rec: the buffer the last segment wrote
  const double *strag;
  int64_t cap;
  int exit_rec, slab;
};
__global__ __launch_bounds__(256) void k_strag_finish(StragFinish F) {
  const TraceArgs &A = F.A;
  const int64_t N = A.N;
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool gone = j < N && A.rec[2 * N + j] == -__builtin_inf();
  double y[9];
#pragma unroll
  for (int row = 0; row < 9; ++row) y[row] = __builtin_nan("");
  if (gone) {
    const int64_t g = (int64_t)A.rec[j];
#pragma unroll
    for (int row = 0; row < 9; ++row) y[row] = F.strag[row * F.cap + g];
  }
  if (F.exit_rec) {
    if (gone) {
#pragma unroll
      for (int row = 0; row < 9; ++row) A.rec[row * N + j] = y[row];
    }
    return;
  }
  const bool finished = gone && y[2] == y[2] && y[6] <= A.t_end;
  if (finished) {
    const double rem = A.t_end - y[6];
    write_outputs(A, j, fma(y[2], rem, A.V.g[0][A.V.na - 1]), fma(y[3], rem, y[0]), fma(y[4], rem, y[1]), y[2], y[3], y[4], y[5], y[7], y[8]);
  }
  if (F.slab) {
    if (gone && !finished) write_lost(A, j);
  } else {
    queue_push(A.out_count, A.out_list, gone && !finished, (uint32_t)j);
  }
}

// REC: the coefficient records ready-made in HBM (sr_volume::R), one of 128 bytes per (node plane, lateral cell), exactly what
// coefs_from_corners forms -- the same function builds them here, once per volume.  Index ((k * (nc-1) + ic) * (nb-1) + ib) * 16:
// the eight cells ib = ob .. ob + 7 of one tile column are ONE KiB, what one global_load_lds_dwordx4 of a wavefront moves.
template <bool PHASE>
__global__ __launch_bounds__(256) void k_build_records(VolDev V, double *__restrict__ R) {
  const int64_t cells = (int64_t)(V.nb - 1) * (V.nc - 1), total = cells * V.na;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(t / cells);
    const int64_t rem = t - (int64_t)k * cells;
    const int ic = (int)(rem / (V.nb - 1)), ib = (int)(rem - (int64_t)ic * (V.nb - 1));
    const int64_t q = col8(V, ib, ic) + koff(V, k), sc = kSC, sb = (int64_t)V.nc * 8;
    float4 v[4] = {V.P[q], V.P[q + sc], V.P[q + sb], V.P[q + sb + sc]};
    float l[4] = {0.f, 0.f, 0.f, 0.f};
    if (PHASE) {
      l[0] = V.L[q];
      l[1] = V.L[q + sc];
      l[2] = V.L[q + sb];
      l[3] = V.L[q + sb + sc];
    }
    CoefPlane p;
    coefs_from_corners<PHASE>(v, l, p);
    double2 *o = reinterpret_cast<double2 *>(R + t * 16);
    o[0] = make_double2(p.a[0], p.a[1]);
    o[1] = make_double2(p.a[2], p.a[3]);
    o[2] = make_double2(p.b[0], p.b[1]);
    o[3] = make_double2(p.b[2], p.b[3]);
    o[4] = make_double2(p.c[0], p.c[1]);
    o[5] = make_double2(p.c[2], p.c[3]);
    o[6] = make_double2(p.d[0], p.d[1]);
    o[7] = make_double2(p.d[2], p.d[3]);
  }
}

// Diagnostic builds (tools/build_variant.sh <name> -DSR_TILE_EXP_...; wrong results, timing only; DESIGN.md round 3 has the numbers):
// SR_TILE_EXP_NOBARRIER (no barrier in the step loop), SR_TILE_EXP_NOPRODUCE (no plane is loaded or built in the loop),
// SR_TILE_EXP_NORELOC (a ray never changes its cell), SR_TILE_EXP_NOSTEPS (the step loop runs no step: what a launch costs before
// its first step and after its last; profiles/r08_tile_startup.txt).  SR_TILE_EXP_DMA_SADDR (right results): the records kernel's LDS-DMA by an
// inline statement in the scalar-base form (lds_dma16, trace.hip; profiles/r06_step_loop.txt).
#ifndef SR_TILE_THREADS
// 256 rays per workgroup with an 8 x 8 tile (46 KB of LDS): THREE workgroups share a CU -- 12 wavefronts, 3 per SIMD at 168
// VGPRs as before, but a workgroup's barrier (four wavefronts, one per SIMD) and its start and end are the other two's issue
// time.  Measured on BASELINE config 3: 768 rays with a 12 x 16 tile (one workgroup per CU) 49.4 ms in two 256-plane segments,
// 256 rays 46.0 ms in three 171-plane segments (6.6 % of the rays leave the smaller tiles: +1.3 ms of k_trace_f64) -- 52.5
// against 50.6 ms per step; 384 and 1024 rays per workgroup: 80 and (28 registers spilled) slower.
#define SR_TILE_THREADS 256
#endif
#ifndef SR_TILE_WAVES
// wavefronts per SIMD the register budget is set for: 3 (158 VGPRs).  4 (128 VGPRs) spills 57 registers: the two records in
// flight (64), the state and the RK4 sums (54), the producers' raw plane (20) do not fit (tools/kernel_resources.py -DSR_TILE_WAVES=4)
#define SR_TILE_WAVES 3
#endif
// AUX: the optional terms of dsdt (d(amp) = kappa*amp, d(pol) = V*n_e*(B.v); full_solver.py:243-268, 356-374, 540-542) ride the
// same stages with k_trace_f64<., true, .>'s arithmetic (aux_coefs / aux_eval / aux_rates: the same functions, the same bits):
// a cell's record carries the bilinear coefficients of {kappa, n_e, B_x, B_y, B_z} behind the gradient fields' (20 more float64),
// built once per (cell, node plane) by a SECOND wavefront of producers (lanes 64 .. 64 + TB*TC - 1: the first wavefront builds
// the gradient records as before), the mid record LO + HI likewise; a stage reads its cell's 160 bytes after the gradient blend.
// 74 KB of LDS with a 6 x 8 tile... the library takes 6 x 7 (64 KB): TWO workgroups per CU, two wavefronts per SIMD at <= 256
// registers.  What a tile loses goes through k_trace_f64<., true, .>'s plane-range form, amp and pol in rows 7, 8 of the record.
// REC (never with AUX; 8 x 8 tiles, 256 threads): the node planes' records come ready-made from HBM (sr_volume::R) by LDS-DMA -- each
// of the four wavefronts brings two tile columns of node plane k + 2 (2 x global_load_lds_dwordx4: 1 KiB each, no register, no
// conversion) at the step's start and, at its end, adds them to its own two columns of plane k + 1 for the mid record (the
// same lane-linear kilobytes: 4 ds_read_b128 + 4 v_add_f64 + 2 ds_write_b128, every lane busy, no bank conflict).  No producer
// wavefront: the four wavefronts of a workgroup do the same work, and the per-step conversions and differences (56 of wavefront
// 0's 66 extra instructions) are gone.  The records are the ones coefs_from_corners forms (k_build_records), the mid record is
// (plane k + 1) + (plane k + 2) component by component as before: the same bits.
#ifndef SR_TILE_REC_WAVES
// REC holds no raw plane and forms no coefficients: 131 registers at a budget of 168, and at a budget of 128 -- FOUR wavefronts per
// SIMD -- 4 of them spilled (20 bytes of scratch per lane, outside the step loop).  With an 8 x 7 tile (36 KB of LDS) four
// workgroups share a CU.  Measured on BASELINE config 3 (profiles/r05_tile_variants.txt): three wavefronts per SIMD 46.3 ms in the
// kernels (the producers' kernel: 45.7), four 41.7.
#define SR_TILE_REC_WAVES 4
#endif
template <bool PHASE, bool AUX = false, bool REC = false>
__global__ __launch_bounds__(SR_TILE_THREADS, AUX ? 2 : (REC ? SR_TILE_REC_WAVES : SR_TILE_WAVES)) void k_trace_tile(TileArgs T) {
  static_assert(!(AUX && REC), "the ready-made records hold the gradient fields only");
  static_assert(SR_TILE_THREADS % 64 == 0 && SR_TILE_THREADS / 64 <= 16, "the placement's scratch holds one slot per wavefront, 16 at the most");
  constexpr int kTileRec = tile_rec(AUX, REC);
  extern __shared__ double lds[];
  const TraceArgs &A = T.A;
  const VolDev &V = A.V;
  const int TB = T.G.tb, TC = T.G.tc, NC = TB * TC;
  // LDS: [node table b: {g, r} x (TB + 9)][node table c: {g, r} x (TC + 9)][placement: 16 x 4 words][records: 5 slots x NC x kTileRec]
  // (tile_tab_entries: sentinels on both sides; REC: laid out for 8 x 8, so that both tables' addresses are constants)
  const int tab_nb = tile_tab_entries(REC ? 8 : TB), tab_nc = tile_tab_entries(REC ? 8 : TC);
  int *org = reinterpret_cast<int *>(lds + 2 * (tab_nb + tab_nc));
  const size_t tables = REC ? 1024 / sizeof(double) : ((size_t)tile_tab_doubles(TB, TC) + 1) & ~(size_t)1;
  // LDS byte addresses of the two tables' entries of node 0 (low word of the flat address)
  // (taken from the LDS pointer itself: the flat pointer's low word comes with a null check that the compiler folds late)
  const unsigned tab_b = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double *)lds + kTabLo * 16u;
  const unsigned tab_c = tab_b + (unsigned)tab_nb * 16u;
  double *recs = lds + tables;                       // 16-byte aligned (REC: 1 KiB)
  const int slot_d = REC ? TC * kRecColD : NC * kTileRec;  // doubles per slot
  // where the record of tile cell (tb, tc) starts inside a slot, in doubles -- REC: in BYTES (its piece 0; the others follow 128
  // bytes apart): the records kernel keeps every LDS address of the step loop as a byte address (see slot_h below)
  // (REC: the column pitch is a constant and the indices are small: a 24-bit multiply-add, where the full 32-bit product is a
  // quarter-rate instruction)
  auto cell_off = [&](int b_, int c_) { return REC ? __mul24(c_, kRecColD * 8) + b_ * 16 : (c_ * TB + b_) * kTileRec; };
  // slots 0..2: node planes (k % 3); 3, 4: mid-step planes (3 + k % 2)

  const unsigned chunk = gridDim.x / 8;
  const unsigned bid = (blockIdx.x % 8) * chunk + blockIdx.x / 8;  // one contiguous run of the ordered rays per XCD
  const bool wg_live = bid < A.n_blocks;                            // uniform over the workgroup: padding workgroups only idle along
  const int64_t j = (int64_t)(T.block0 + bid) * blockDim.x + threadIdx.x;
  const bool have = wg_live && j < A.N;
  const int64_t N = A.N;
  const int a = A.axis, b = (a + 1) % 3, c = (a + 2) % 3;
  int64_t i = 0;

  double y0 = 0, y1 = 0, y2 = 1, y3 = 0, y4 = 0, y5 = 0, y6 = 0, y7 = 0, y8 = 0;  // y7 = amp, y8 = pol (AUX)
  bool alive = false;
  // the state on the entry plane from s0 (as k_trace_f64): false when the ray is not a plane-form ray
  auto from_s0 = [&](const TraceArgs &Q, int64_t ray, double &q0, double &q1, double &q2, double &q3, double &q4, double &q5, double &q6) -> bool {
    const double pa = Q.s0[a * N + ray];
    q0 = Q.s0[b * N + ray];
    q1 = Q.s0[c * N + ray];
    q2 = Q.s0[(3 + a) * N + ray];
    q3 = Q.s0[(3 + b) * N + ray];
    q4 = Q.s0[(3 + c) * N + ray];
    q5 = Q.s0[7 * N + ray];
    q6 = 0;
    const double ga0 = Q.V.g[0][0];
    bool ok = (q2 > 0) && (pa <= ga0);
    if (ok && pa < ga0) {  // vacuum drift onto the entry plane
      const double tau = (ga0 - pa) / q2;
      if (tau >= Q.t_end) {
        ok = false;
      } else {
        q0 = q0 + q3 * tau;
        q1 = q1 + q4 * tau;
        q6 = tau;
      }
    }
    return ok;
  };
  uint32_t pk = kNoCell;  // the ray's packed cell on node plane k0, as the binning found it
  if (T.first) {
    i = have ? (int64_t)A.perm[j] : 0;
    if (have) pk = T.cells[i];
    if (have) alive = from_s0(A, i, y0, y1, y2, y3, y4, y5, y6);
    if (AUX && have) {
      y7 = A.s0[6 * N + i];
      y8 = A.s0[8 * N + i];
    }
    if (!alive) y2 = 1;
  } else if (have) {
    const int64_t o = (int64_t)T.order[j];  // where the ray's record sits in the buffer the segment before wrote
    const double *R = T.rec_in;
    pk = T.cells[o];
    if (AUX) {
      y7 = R[7 * N + o];
      y8 = R[8 * N + o];
    } else {  // amp and pol ride along unchanged
      A.rec[7 * N + j] = R[7 * N + o];
      A.rec[8 * N + j] = R[8 * N + o];
    }
    y0 = R[o];
    y1 = R[N + o];
    y2 = R[2 * N + o];
    y3 = R[3 * N + o];
    y4 = R[4 * N + o];
    y5 = R[5 * N + o];
    y6 = R[6 * N + o];
    const double idx = R[9 * N + o];
    A.rec[9 * N + j] = idx;
    T.perm_out[j] = (uint32_t)idx;
    alive = y2 == y2;
  }
  // gone: a straggler of an earlier segment (v_a = -inf, row 0 = its entry in the straggler records): the marks ride along
  const bool gone = have && !T.first && y2 == -__builtin_inf();
  alive = alive && (y0 == y0) && (y1 == y1) && (y3 == y3) && (y4 == y4) && (y5 == y5) && (y2 < 1e30) && (y2 > 1e-30);
  const bool entered = alive;  // a plane-form ray on node plane k0: if this launch loses it, k_trace_f64 takes it from that state

  // ---- the tile: placed around the cells the workgroup's rays are in now AND the cells a straight line takes them to by the
  // segment's end (the rays that leave a tile are the fast ones, and neighbouring rays are deflected alike: the box of the
  // predicted paths follows them); the box is centred in the tile.  Where the predicted box does not fit, the entry cells alone.
  // The entry cell is the one the binning before this launch found for the ray (T.cells: the same find_cell of the same
  // position; a cell that were off is put right by stage 1's weight test or loses the ray to k_trace_f64: the bits stay), and the
  // cell's own node and reciprocal width come straight from the volume's arrays -- the values the tile's node table will hold.
  // The predicted exit cell is a heuristic: the entry cell moved on by floor(weight + lateral travel x the cell's reciprocal
  // width), the travel with 1 / v_a from the float32 reciprocal -- no search, no division.
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ln = (int)(threadIdx.x & 63);
  int cb = 0, cc = 0, xb = 0, xc = 0;
  double lo_b = 0, r_b = 1, lo_c = 0, r_c = 1;
  if (alive) {
    const double gb0 = V.g[1][0], gbL = V.g[1][V.nb - 1], gc0 = V.g[2][0], gcL = V.g[2][V.nc - 1];
    // strictly inside: the volume's last nodes are k_trace_f64's business (the key kernels' test admits them)
    if (y0 >= gb0 && y0 < gbL && y1 >= gc0 && y1 < gcL && pk != kNoCell) {
      cb = min((int)(pk & 0xffffu), V.nb - 2);
      cc = min((int)(pk >> 16), V.nc - 2);
      lo_b = V.g[1][cb];
      r_b = V.rg[1][cb];
      lo_c = V.g[2][cc];
      r_c = V.rg[2][cc];
      const double dz = (V.g[0][T.k1] - V.g[0][T.k0]) * rcp_f64_from_f32(y2);
      const double ub = fma(y3 * dz, r_b, (y0 - lo_b) * r_b), uc = fma(y4 * dz, r_c, (y1 - lo_c) * r_c);
      xb = min(max(cb + (int)floor(fmin(fmax(ub, -65536.0), 65536.0)), 0), V.nb - 2);
      xc = min(max(cc + (int)floor(fmin(fmax(uc, -65536.0), 65536.0)), 0), V.nc - 2);
    } else {
      alive = false;  // starts outside the volume: lost to this kernel
    }
  }
  // box: {min b, min c} of the entry cells, of entry + predicted, {max b, max c} of the entry cells, of entry + predicted -- four words
  // of two uint16, reduced over the wavefront in registers (wave_pk_u16) and over the workgroup's wavefronts through one LDS slot each
  uint4 *box = reinterpret_cast<uint4 *>(org);
  {
    unsigned e = 0xFFFFFFFFu, x = 0xFFFFFFFFu, E = 0u, X = 0u;
    if (alive) {
      e = E = (unsigned)cb | ((unsigned)cc << 16);
      x = (unsigned)min(cb, xb) | ((unsigned)min(cc, xc) << 16);
      X = (unsigned)max(cb, xb) | ((unsigned)max(cc, xc) << 16);
    }
    e = wave_pk_u16<false>(e);
    x = wave_pk_u16<false>(x);
    E = wave_pk_u16<true>(E);
    X = wave_pk_u16<true>(X);
    if (ln == 63) box[wv] = make_uint4(e, x, E, X);
  }
  __syncthreads();
  uint4 bx = box[0];
#pragma unroll
  for (int w = 1; w < SR_TILE_THREADS / 64; ++w) {
    const uint4 o = box[w];
    bx = make_uint4(pk_min_u16(bx.x, o.x), pk_min_u16(bx.y, o.y), pk_max_u16(bx.z, o.z), pk_max_u16(bx.w, o.w));
  }
  auto place = [](int lo_e, int hi_e, int lo_x, int hi_x, int t, int cells) {
    if (hi_e < lo_e) return 0;  // no live ray
    int lo = lo_x, hi = hi_x;
    if (hi - lo + 1 > t) {
      lo = lo_e;
      hi = hi_e;
    }
    if (hi - lo + 1 > t) hi = lo + t - 1;  // the entry cells span more than a tile: the rays beyond it are lost below
    return min(max(lo - (t - (hi - lo + 1)) / 2, 0), cells - t);
  };
  const int ob = place((int)(bx.x & 0xffffu), (int)(bx.z & 0xffffu), (int)(bx.y & 0xffffu), (int)(bx.w & 0xffffu), TB, V.nb - 1);
  const int oc = place((int)(bx.x >> 16), (int)(bx.z >> 16), (int)(bx.y >> 16), (int)(bx.w >> 16), TC, V.nc - 1);
  typedef double d2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) d2 *lds_d2_t;
  // the node tables: nodes 0 .. t of the tile between their sentinels (tile_tab_entries)
  auto fill_table = [&](unsigned tab, int t_cells, const double *g, const double *rg, int o) {
    for (int t = threadIdx.x; t < tile_tab_entries(t_cells); t += blockDim.x) {
      const int n = t - kTabLo;
      d2 e = {n < 0 ? __builtin_inf() : -__builtin_inf(), 1.0};
      if (n >= 0 && n <= t_cells) e.x = g[o + n];
      if (n >= 0 && n < t_cells) e.y = rg[o + n];
      ((lds_d2_t)(uintptr_t)tab)[n] = e;
    }
  };
  // (the tables are filled further down, while the first node planes are on their way; the lane's own entries {lo, r} it has already)
  int tb = cb - ob, tc = cc - oc;
  if (alive && !(tb >= 0 && tb < TB && tc >= 0 && tc < TC)) alive = false;  // the workgroup's rays span more than a tile
  if (!alive) tb = tc = 0;
  int cell = cell_off(tb, tc);  // record offset inside a slot, in doubles: column-major (see the banks note below)

  // ---- producers: NC consecutive lanes, one cell each.  WHICH lanes rotates with the workgroup index: a CU holds three
  // workgroups, and the hardware places wavefront w of every workgroup on SIMD w -- with the producers always in wavefront 0,
  // SIMD 0 carried all three producer wavefronts (336 instead of 226 instructions per step each) and, through the barriers,
  // set the pace of the whole CU.  Workgroups i, i + 256, i + 512 are the ones dispatched to the same CU (8 XCDs x 32 CUs in
  // turn), so (i / 256) % 4 puts their producers on three different SIMDs.
  const int p_first = T.rot ? (int)((blockIdx.x >> 8) & 3u) * 64 : 0;
  const int p_lane = (int)((threadIdx.x + blockDim.x - (unsigned)p_first % blockDim.x) % blockDim.x);
  const bool producer = !REC && wg_live && p_lane < NC;
  const int pcell = producer ? p_lane * kTileRec : 0;
  const int64_t sc = kSC, sb = (int64_t)V.nc * 8;
  // producer lane t owns the cell with record index t = tc * TB + tb.  Records are 144 bytes apart and column-major: the
  // neighbours of a cell (one row or one column away: 1, TB or TB +- 1 records) start 36, 48, 12 or 20 banks further on,
  // never on the same four banks, and rays that share a 16-lane group of a ds_read_b128 sit in neighbouring cells.
  const int64_t pcol = producer ? col8(V, ob + p_lane % TB, oc + p_lane / TB) : 0;
  struct RawPlane {
    float4 v[4];
    float l[4];
  };
  auto issue_raw = [&](int k, RawPlane &r) {
    const int64_t ko = koff(V, k);
    const float4 *q = V.P + pcol + ko;
    r.v[0] = q[0];
    r.v[1] = q[sc];
    r.v[2] = q[sb];
    r.v[3] = q[sb + sc];
    r.l[0] = r.l[1] = r.l[2] = r.l[3] = 0.f;
    if (PHASE) {
      const float *l = V.L + pcol + ko;
      r.l[0] = l[0];
      r.l[1] = l[sc];
      r.l[2] = l[sb];
      r.l[3] = l[sb + sc];
    }
  };
  // AUX: the second wavefront's lanes own one cell each as well, for the optional terms' fields
  const int a_lane = (int)threadIdx.x - 64;
  const bool aproducer = AUX && wg_live && a_lane >= 0 && a_lane < NC;
  const int apcell = aproducer ? a_lane * kTileRec + 16 : 16;  // the aux coefficients sit behind the record's 16 gradient ones
  const int64_t apcol = aproducer ? col8(V, ob + a_lane % TB, oc + a_lane / TB) : 0;
  auto store_aux = [&](int slot, int off, const AuxPlane &p) {
    double2 *o = reinterpret_cast<double2 *>(recs + slot * slot_d + off);
    const double f[20] = {p.a[0], p.a[1], p.a[2], p.a[3], p.a[4], p.b[0], p.b[1], p.b[2], p.b[3], p.b[4],
                          p.c[0], p.c[1], p.c[2], p.c[3], p.c[4], p.d[0], p.d[1], p.d[2], p.d[3], p.d[4]};  // 10 x 16 bytes
#pragma unroll
    for (int q = 0; q < 10; ++q) o[q] = make_double2(f[2 * q], f[2 * q + 1]);
  };
  auto load_aux_rec = [&](int slot, int off, AuxPlane &p) {
    const double2 *o = reinterpret_cast<const double2 *>(recs + slot * slot_d + off);
    double f[20];
#pragma unroll
    for (int q = 0; q < 10; ++q) {
      const double2 t = o[q];
      f[2 * q] = t.x;
      f[2 * q + 1] = t.y;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      p.a[q] = f[q];
      p.b[q] = f[5 + q];
      p.c[q] = f[10 + q];
      p.d[q] = f[15 + q];
    }
  };
  // node plane k's aux record into slot `dst`, and (prev >= 0) the mid record (plane before) + (this one) into slot `mid`
  auto produce_aux = [&](const double (&u)[4][5], int dst, int prev, int mid) {
    AuxPlane p, q;
    aux_coefs(u, p);
    store_aux(dst, apcell, p);
    if (prev >= 0) {
      load_aux_rec(prev, apcell, q);
#pragma unroll
      for (int f = 0; f < 5; ++f) {  // LO + HI in k_trace_f64's order: (plane k-1) + (plane k)
        q.a[f] += p.a[f];
        q.b[f] += p.b[f];
        q.c[f] += p.c[f];
        q.d[f] += p.d[f];
      }
      store_aux(mid, apcell, q);
    }
  };
  auto store_rec = [&](int slot, int off, const CoefPlane &p) {
    double2 *o = reinterpret_cast<double2 *>(recs + slot * slot_d + off);
    o[0] = make_double2(p.a[0], p.a[1]);
    o[1] = make_double2(p.a[2], p.a[3]);
    o[2] = make_double2(p.b[0], p.b[1]);
    o[3] = make_double2(p.b[2], p.b[3]);
    o[4] = make_double2(p.c[0], p.c[1]);
    o[5] = make_double2(p.c[2], p.c[3]);
    o[6] = make_double2(p.d[0], p.d[1]);
    o[7] = make_double2(p.d[2], p.d[3]);
  };
  auto load_rec = [&](int slot, int off, CoefPlane &p) {
    const double2 *q = reinterpret_cast<const double2 *>(recs + slot * slot_d + off);
    const double2 a01 = q[0], a23 = q[1], b01 = q[2], b23 = q[3], c01 = q[4], c23 = q[5], d01 = q[6], d23 = q[7];
    p.a[0] = a01.x; p.a[1] = a01.y; p.a[2] = a23.x; p.a[3] = a23.y;
    p.b[0] = b01.x; p.b[1] = b01.y; p.b[2] = b23.x; p.b[3] = b23.y;
    p.c[0] = c01.x; p.c[1] = c01.y; p.c[2] = c23.x; p.c[3] = c23.y;
    p.d[0] = d01.x; p.d[1] = d01.y; p.d[2] = d23.x; p.d[3] = d23.y;
  };
  // a node plane from its corner records into slot `dst`, and (prev >= 0) the mid plane (the plane before, in slot `prev`) +
  // (this one) into slot `mid`
  auto produce = [&](const RawPlane &r, int dst, int prev, int mid) {
    CoefPlane p, q;
    coefs_from_corners<PHASE>(r.v, r.l, p);
    store_rec(dst, pcell, p);
    if (prev >= 0) {
      load_rec(prev, pcell, q);  // this lane's own record of the plane before (written by this lane: no barrier needed)
#pragma unroll
      for (int f = 0; f < 4; ++f) {  // LO + HI in k_trace_f64's order: (plane k-1) + (plane k)
        q.a[f] += p.a[f];
        q.b[f] += p.b[f];
        q.c[f] += p.c[f];
        q.d[f] += p.d[f];
      }
      store_rec(mid, pcell, q);
    }
  };
  // REC: wavefront w brings tile columns 2w and 2w + 1 of a node plane into a slot: lane l's 16 bytes are piece l % 8 of the
  // record of cell (ob + l / 8, oc + column), and land at the slot's column + l * 16 -- the DMA's own lane-linear order
  // (wv, ln: the wavefront and the lane in it, from the placement above)
  // Addresses: everything but the lane's place inside its kilobyte is wave-uniform -- the tile's first record, the node plane, the
  // column -- and is kept in scalar registers (ob, oc come out of LDS: readfirstlane tells the compiler); the lane adds ONE 32-bit
  // offset, the same for the whole launch (how the step loop keeps it that way: see lds_dma16 and the loop's DMA).  (Formed per lane in 64-bit integer arithmetic the two addresses were 15 vector
  // instructions per step: profiles/r05_pmc_c3_f64_first_layout.csv, INT32 + INT64 35 per wavefront-step against the producers' 27.)
  const int ob_u = __builtin_amdgcn_readfirstlane(ob), oc_u = __builtin_amdgcn_readfirstlane(oc);
  unsigned lane_off = (unsigned)(ln & 7) * 128u + (unsigned)(ln >> 3) * 16u;  // piece ln / 8 of the record of row ln % 8
  const int64_t col_bytes = (int64_t)(V.nb - 1) * 128, plane_bytes = (int64_t)(V.nc - 1) * col_bytes;
  const char *tile_r = REC ? reinterpret_cast<const char *>(V.R) + ((int64_t)oc_u * (V.nb - 1) + ob_u) * 128 : nullptr;
  // A slot's HANDLE is what the step loop rotates and hands to request / dma_cols / mid_from.  REC: the LDS byte address of the
  // slot's first record, wave-uniform, so that the loop holds no slot * slot_d multiply and an address is one add of a handle
  // and a lane constant; otherwise the slot's index, as the producers' stores and the optional terms' reads take it.
  const unsigned recs_lds = (unsigned)(uintptr_t)recs;  // LDS byte address of the records (low word of the flat address)
  auto slot_h = [&](int slot) { return REC ? (int)(recs_lds + (unsigned)(slot * slot_d) * 8u) : slot; };
  // the wavefront's first column: where its block starts inside a slot (bytes), and the node plane's records of it in HBM.  The
  // records are plane-linear in the volume's -- or the slab's -- OWN planes (k_build_records: no koff() octets here)
  const int wcol_b = 2 * wv * (kRecColD * 8);
  const char *wcol_r = REC ? tile_r + (int64_t)(2 * wv) * col_bytes : nullptr;
  // one kilobyte from src + lane_off into LDS at dst + lane * 16 (lds_dma16, trace.hip: the address forms are weighed there)
  auto glds16 = [&](const char *src, int dst) { lds_dma16(src, lane_off, (unsigned)dst); };
  // the wavefront's two columns of one node plane (src0, src1: their records in HBM) into the slot with handle `slot`
  auto dma_cols = [&](const char *src0, const char *src1, int slot) {
    if (2 * wv < TC) glds16(src0, slot + wcol_b);  // (a tile of fewer than eight columns: the last wavefront has one, or none)
    if (2 * wv + 1 < TC) glds16(src1, slot + wcol_b + kRecColD * 8);
  };
  // the mid record of the wavefront's own two columns: (plane in slot `lo`) + (plane in slot `hi`) -> slot `mid`, 16 bytes per
  // lane; the slots by their handles, the lane's place in the wavefront's block a constant of the launch
  const int mid_lane = wcol_b + ln * 16;
  auto mid_from = [&](int lo, int hi, int mid, bool col0, bool col1) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (!(q ? col1 : col0)) break;
      const d2 a = ((lds_d2_t)(uintptr_t)(unsigned)(lo + mid_lane))[q * (kRecColD / 2)];
      const d2 b = ((lds_d2_t)(uintptr_t)(unsigned)(hi + mid_lane))[q * (kRecColD / 2)];
      ((lds_d2_t)(uintptr_t)(unsigned)(mid + mid_lane))[q * (kRecColD / 2)] = a + b;
    }
  };
  // Start-up order: the first two node planes are asked for as soon as the tile's place is known; the node tables are filled
  // while they are on their way; ONE wait, the mid record, and the barrier that ends the start-up (tables, records, mid record).
  if (REC && wg_live) {
    const char *p0 = wcol_r + (int64_t)T.k0 * plane_bytes;
    dma_cols(p0, p0 + col_bytes, slot_h(T.k0 % 3));
    dma_cols(p0 + plane_bytes, p0 + plane_bytes + col_bytes, slot_h((T.k0 + 1) % 3));
  }
  fill_table(tab_b, TB, V.g[1], V.rg[1], ob);
  fill_table(tab_c, TC, V.g[2], V.rg[2], oc);
  if (REC && wg_live) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    mid_from(slot_h(T.k0 % 3), slot_h((T.k0 + 1) % 3), slot_h(3 + T.k0 % 2), 2 * wv < TC, 2 * wv + 1 < TC);
  }
  if (producer) {
    RawPlane r0, r1;
    issue_raw(T.k0, r0);
    issue_raw(T.k0 + 1, r1);
    produce(r0, T.k0 % 3, -1, 0);
    produce(r1, (T.k0 + 1) % 3, T.k0 % 3, 3 + T.k0 % 2);
  }
  if (aproducer) {
    double u0[4][5], u1[4][5];
    aux_corners(V, apcol + koff(V, T.k0), u0);
    aux_corners(V, apcol + koff(V, T.k0 + 1), u1);
    produce_aux(u0, T.k0 % 3, -1, 0);
    produce_aux(u1, (T.k0 + 1) % 3, T.k0 % 3, 3 + T.k0 % 2);
  }
  __syncthreads();

#ifdef SR_TILE_EXP_NORELOC
  constexpr unsigned kInside = 0xFFFFFFFFu;
#else
  constexpr unsigned kInside = 0x3FEFFFFFu;  // hi32(w) <u this  <=>  0 <= w < 1 - 2^-21  (k_trace_f64)
#endif
  // The cell search inside the tile at position (qb, qc), given the weights (wb, wc) that failed the test in the cached cell: the
  // neighbour each weight points at (the only way out of a cell within one stage: a stage moves a ray by a hundredth of a
  // cell), accepted when the node table says g[n] <= q < g[n+1] (k_trace_f64's locate2); the weights come back formed in the new
  // cell.  The region this is runs for the whole wavefront when ONE of its rays changes its cell, so it is written to be short:
  //  * the step is integer arithmetic on the weight's high word h: (h >> 31) + (h >= kInside as signed) = -1 for a set sign, +1
  //    from kInside on, else 0 -- a shift, a compare and an add with carry per axis.  (-0.0 and a NaN with the sign set step down
  //    where `w < 0.0` did not: the acceptance test below decides, as it always did.)
  //  * no clamp: the index may become -1 or T, where the table holds sentinels that fail the test (tile_tab_entries).
  //  * one address per axis: g[n], r[n] and g[n+1] are 0, 8 and 16 bytes from tab + n * 16; both axes' six reads are one LDS
  //    round trip, and there is no branch in here to keep them ahead of.  They are written as asm, one float64 each, with their
  //    wait (which also ends the wait for any record still in flight: the counted waits that follow only become conservative).
  //    Read through the compiler as {g, r} vectors of 16 bytes, the vectors reach the state: the SLP vectoriser pairs (y0, y1) into
  //    one as well, and the common path pays two 64-bit copies per step; read as two float64 of one 16-byte load, g and r have to
  //    be moved out of the load's register tuple -- six to nine v_mov_b32 per region.
  //  * both axes move on UNCONDITIONALLY: an axis whose weight passed the test gets its own cell again (index + 0: the same
  //    table entries, the same bits), and a ray the table does not accept is lost to this launch whatever its cell variables
  //    hold from here on -- its straggler entry is formed from the state it entered the segment with, not from this one.  (Until
  //    its step ends it reads records at whatever cell_off makes of its index, at most four cells off the tile: LDS reads, of
  //    another slot's bytes or, outside the workgroup's allocation, of zeros.)
  //  * g[n] <= q is the sign of the new weight (q - g[n]) * r[n]: the subtraction's sign is exact, r > 0, and a product that
  //    underflows keeps its sign.  q < g[n+1] is asked of the table itself: the rounded reciprocal could say otherwise.
  // false: not there (the tile's edge, NaN, or a weight within 2^-21 of 1 whose ray is still in its cell: one stage in two
  // million) -- the ray is lost to this launch and k_trace_f64 carries it through the segment; a general walk along the table
  // here cost 1.3 % of the kernel for nothing.
  auto relocate2 = [&](double qb, double qc, double &wb, double &wc) -> bool {
    const int hb = (int)hi_word(wb), hc = (int)hi_word(wc);
    tb += (hb >> 31) + (hb >= (int)kInside ? 1 : 0);
    tc += (hc >> 31) + (hc >= (int)kInside ? 1 : 0);
    const unsigned ab = tab_b + ((unsigned)tb << 4), ac = tab_c + ((unsigned)tc << 4);
    double ub, uc;
    asm volatile("ds_read_b64 %0, %6\n\tds_read_b64 %1, %6 offset:8\n\tds_read_b64 %2, %6 offset:16\n\t"
                 "ds_read_b64 %3, %7\n\tds_read_b64 %4, %7 offset:8\n\tds_read_b64 %5, %7 offset:16\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(lo_b), "=&v"(r_b), "=&v"(ub), "=&v"(lo_c), "=&v"(r_c), "=&v"(uc)
                 : "v"(ab), "v"(ac));
    wb = (qb - lo_b) * r_b;
    wc = (qc - lo_c) * r_c;
    // (the unsigned maximum has its top bit set when either weight's sign is; an OR of the two the compiler widens to 64 bits)
    return ((int)max(hi_word(wb), hi_word(wc)) >= 0) & (qb < ub) & (qc < uc);
  };

  // ---- records in registers.  A record is read by eight ds_read_b128 written as asm: the compiler does not know them to be
  // loads, so it places no wait of its own; the waits are the counted s_waitcnt lgkmcnt(n) below (LDS reads return in
  // order: n = the number of reads issued AFTER the ones wanted).  A record is requested ONE STAGE AHEAD, for the exact
  // cell of the stage that will use it: stage s needs its position q_s = y + w * kp_(s-1) only, and kp_s = v_s / v_a,s is known
  // at the START of stage s, before its blend -- so stage s first places the ray for stage s+1, issues that record's reads,
  // and only then blends with its own record, requested a stage earlier.  Stages 2 and 3 share the mid record and stage 1
  // of the next step takes over stage 4's (the same node plane) when the cell is the same, which it almost always is.
  struct Rec {
    d2 q[8];  // a01 a23 b01 b23 c01 c23 d01 d23
    int off;  // where the record sits in LDS, in doubles from `recs` (AUX: the optional terms' coefficients are 16 further on)
  };
  // slot: the slot's handle (slot_h), cell_d: the cell's place inside a slot as cell_off gives it.  REC: both are bytes, the
  // address is their sum -- one vector add of a scalar
  auto request = [&](int slot, int cell_d, Rec &R) {
    R.off = REC ? 0 : slot * slot_d + cell_d;
    const unsigned addr = REC ? (unsigned)slot + (unsigned)cell_d : recs_lds + (unsigned)(slot * slot_d + cell_d) * 8u;
    if (REC)  // the record's pieces are 128 bytes apart (piece-major blocks)
      asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:128\n\tds_read_b128 %2, %8 offset:256\n\tds_read_b128 %3, %8 offset:384\n\t"
                   "ds_read_b128 %4, %8 offset:512\n\tds_read_b128 %5, %8 offset:640\n\tds_read_b128 %6, %8 offset:768\n\tds_read_b128 %7, %8 offset:896"
                   : "=&v"(R.q[0]), "=&v"(R.q[1]), "=&v"(R.q[2]), "=&v"(R.q[3]), "=&v"(R.q[4]), "=&v"(R.q[5]), "=&v"(R.q[6]), "=&v"(R.q[7])
                   : "v"(addr));
    else
      asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:16\n\tds_read_b128 %2, %8 offset:32\n\tds_read_b128 %3, %8 offset:48\n\t"
                   "ds_read_b128 %4, %8 offset:64\n\tds_read_b128 %5, %8 offset:80\n\tds_read_b128 %6, %8 offset:96\n\tds_read_b128 %7, %8 offset:112"
                   : "=&v"(R.q[0]), "=&v"(R.q[1]), "=&v"(R.q[2]), "=&v"(R.q[3]), "=&v"(R.q[4]), "=&v"(R.q[5]), "=&v"(R.q[6]), "=&v"(R.q[7])
                   : "v"(addr));
  };
#define SR_REC_WAIT(R, n)                                                                                                       \
  asm volatile("s_waitcnt lgkmcnt(" #n ")"                                                                                      \
               : "+v"(R.q[0]), "+v"(R.q[1]), "+v"(R.q[2]), "+v"(R.q[3]), "+v"(R.q[4]), "+v"(R.q[5]), "+v"(R.q[6]), "+v"(R.q[7]))

  // slots rotate with the step: s_lo = k % 3, s_hi = (k + 1) % 3, s_nx = (k + 2) % 3, m_cur = 3 + k % 2, m_nx = 3 + (k + 1) % 2
  // -- held as HANDLES (slot_h; REC: five byte addresses in scalar registers, rotated as they are)
  int s_lo = slot_h(T.k0 % 3), s_hi = slot_h((T.k0 + 1) % 3), s_nx = slot_h((T.k0 + 2) % 3);
  int m_cur = slot_h(3 + T.k0 % 2), m_nx = slot_h(3 + (T.k0 + 1) % 2);
  // REC: where the wavefront's two columns of node plane k + 2 sit in HBM: running pointers, one plane further with every step
  // the last step at which the wavefront asks for its first / second column of node plane k + 2 (none: before every step).  One
  // integer compare with the step stands for "a live workgroup, a column inside the tile, a plane inside the segment"
  constexpr int kNever = -0x7fffffff - 1;
  const int k_col0 = (wg_live && 2 * wv < TC) ? T.k1 - 2 : kNever, k_col1 = (wg_live && 2 * wv + 1 < TC) ? T.k1 - 2 : kNever;
  const char *nx_r0 = REC ? wcol_r + (int64_t)(T.k0 + 2) * plane_bytes : nullptr, *nx_r1 = REC ? nx_r0 + col_bytes : nullptr;
  Rec RA, RB;           // RA: node-plane records (stage 1, stage 4), RB: the mid record
  request(s_lo, cell, RA);
  // The NEXT step's constants {h, h/2, h/6, omega*h/6} by scalar loads, a step ahead: through a constant-address-space pointer,
  // which the compiler reads with s_load whatever else the loop holds (through the generic pointer it turns them into vector
  // loads as soon as the loop has an asm volatile).  A scalar load in flight cannot make a counted wait for a record too short
  // (the counter only reaches n once at most n operations of any kind are outstanding, and the LDS reads return in order): at
  // worst the wait is a little longer.  (Until round 3's last version the table sat in LDS, read by every lane and made
  // uniform with eight v_readfirstlane per step: 0.8 % slower, 5.5 KB of LDS and three spilled registers more.)
  typedef const double __attribute__((address_space(4))) *cdbl_t;
  const cdbl_t ctab = (cdbl_t)(uintptr_t)A.tab64;  // StepTab64 = {h, hh, h6, wa0, waH, wa1, h6w, pad}: 8 doubles per step
  // a running pointer, 64 bytes further with every step; the last step reads the first one's again (there is no step k1)
  const cdbl_t tab0 = ctab + 8 * (int64_t)T.k0;
  cdbl_t tab = tab0;
  double nh = tab[0], nhh = tab[1], nh6 = tab[2], nh6w = tab[6];
#ifdef SR_TILE_EXP_NOSTEPS
  const int k_stop = T.k0;  // no step at all: a launch is its start-up and its tail
#else
  const int k_stop = T.k1;
#endif
  for (int k = T.k0; k < k_stop; ++k) {
    const double Sh = nh, Shh = nhh, Sh6 = nh6, Sh6w = nh6w;
    {
      tab = k + 1 < T.k1 ? tab + 8 : tab0;
      nh = tab[0];
      nhh = tab[1];
      nh6 = tab[2];
      nh6w = tab[6];
    }
    RawPlane NX;
    // AUX: ONE buffer of 20 float64 for the plane on its way, whichever kind of producer the lane is -- the gradient producers'
    // 20 float32 ride in its first ten (bit patterns, no conversion), the optional terms' producers fill all of it: the two
    // kinds never share a lane, and two separate buffers would be 60 registers in every lane of the kernel
    double NXU[20];
    const bool more = k + 2 <= T.k1;  // node plane k + 2 is needed by the next step
    // REC: ... and this wavefront brings a first / a second column of it (k_col0, k_col1: see there)
    const bool more0 = k <= k_col0, more1 = k <= k_col1;
#ifndef SR_TILE_EXP_NOPRODUCE
    if (REC) {
      // the two sources stay wave-uniform pointers in scalar registers: the empty statement hides from the loop's strength
      // reduction that they are induction variables, which would fold lane_off into them (two per-lane 64-bit pointers, moved on
      // by a v_lshl_add_u64 each per step); as they are, the DMA takes the scalar base + 32-bit lane offset form (lds_dma16)
      // (and hide lane_off where it is used: hoisted out of the loop as a 64-bit value it no longer looks like a 32-bit offset)
      if (more0) {
        asm volatile("" : "+s"(nx_r0), "+v"(lane_off));
        glds16(nx_r0, s_nx + wcol_b);
      }
      if (more1) {
        asm volatile("" : "+s"(nx_r1), "+v"(lane_off));
        glds16(nx_r1, s_nx + wcol_b + kRecColD * 8);
      }
    } else if (!AUX) {
      if (producer && more) issue_raw(k + 2, NX);
    } else {
      if (producer && more) {
        RawPlane t;
        issue_raw(k + 2, t);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          NXU[2 * e] = __hiloint2double(__float_as_int(t.v[e].y), __float_as_int(t.v[e].x));
          NXU[2 * e + 1] = __hiloint2double(__float_as_int(t.v[e].w), __float_as_int(t.v[e].z));
        }
        NXU[8] = __hiloint2double(__float_as_int(t.l[1]), __float_as_int(t.l[0]));
        NXU[9] = __hiloint2double(__float_as_int(t.l[3]), __float_as_int(t.l[2]));
      }
      if (aproducer && more) {
        double u[4][5];
        aux_corners(V, apcol + koff(V, k + 2), u);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int f = 0; f < 5; ++f) NXU[5 * e + f] = u[e][f];
      }
    }
#endif
    if (alive) {
      double kp0, kp1, kv0, kv1, kv2, kph, iv;
      double ap0, ap1, av0, av1, av2, aph, at;
      double k7 = 0, k8 = 0, a7 = 0, a8 = 0;  // AUX: slopes and sums of amp, pol
      bool ok = true;
      // ---- stage 1 at (y0, y1): its record RA was requested by the step before (or before the loop) for the cell the ray was
      // in then, and nothing but this region moves it on since
      double wb = (y0 - lo_b) * r_b, wc = (y1 - lo_c) * r_c;
      if (max(hi_word(wb), hi_word(wc)) >= kInside) {  // the rarely-taken region: an index change
        const int was = cell;
        if (!relocate2(y0, y1, wb, wc)) ok = false;   // left the tile: lost to this kernel
        cell = cell_off(tb, tc);
        if (cell != was) request(s_lo, cell, RA);  // the ray ended the step before in another cell than its last stage was in: read again
      }
      // whether the stage just run moved the ray into another cell while placing the next one: set in the rarely-taken region only
      // (a lane mask in scalar registers; a copy of `cell` to compare with afterwards was a vector move and a compare in every step)
      bool moved = false;
      // One stage: (t2, t3, t4) = the stage's velocities, (wb, wc) its weights, R its record (already requested; `pending`
      // reads were issued after it).  Before blending, the NEXT stage's position, cell and weights are formed and (HASNEXT) its
      // record requested into NXT from `nslot`; without it the next stage uses R again unless its cell differs.
      auto stage = [&](auto SI, auto HASNEXT, double t2, double t3, double t4, double t7, Rec &R, Rec &NXT, int nslot, double &nwb, double &nwc) {
        constexpr int s = decltype(SI)::value;
        constexpr bool has_next = decltype(HASNEXT)::value;
        iv = s == 0 ? rcp_f64_from_f32(t2) : rcp_refine(t2, iv);
        const double p0 = t3 * iv, p1 = t4 * iv;  // kp of this stage: where the next stage is
        if (s < 3) {
          const double w = s == 2 ? Sh : Shh;
          const double qb = fma(w, p0, y0), qc = fma(w, p1, y1);
          nwb = (qb - lo_b) * r_b;
          nwc = (qc - lo_c) * r_c;
          if (max(hi_word(nwb), hi_word(nwc)) >= kInside) {
            // this stage's weights (wb, wc) belong to the OLD cell: they are already in registers; the cell variables move on
            const int was = cell;
            if (!relocate2(qb, qc, nwb, nwc)) ok = false;
            cell = cell_off(tb, tc);
            moved = cell != was;
          }
          if (has_next) request(nslot, cell, NXT);
        }
        if (has_next)
          SR_REC_WAIT(R, 8);  // the eight reads just issued may stay in flight
        else
          SR_REC_WAIT(R, 0);
        double F[4];
        F[0] = fma(wc, fma3(wb, R.q[6].x, R.q[4].x), fma3(wb, R.q[2].x, R.q[0].x));
        F[1] = fma(wc, fma3(wb, R.q[6].y, R.q[4].y), fma3(wb, R.q[2].y, R.q[0].y));
        F[2] = fma(wc, fma3(wb, R.q[7].x, R.q[5].x), fma3(wb, R.q[3].x, R.q[1].x));
        F[3] = PHASE ? fma(wc, fma3(wb, R.q[7].y, R.q[5].y), fma3(wb, R.q[3].y, R.q[1].y)) : 0.0;
        const double ivf = (s == 1 || s == 2) ? iv * 0.5 : iv;  // the mid record holds LO + HI
        double r7 = 0, r8 = 0;
        if (AUX) {  // kappa, n_e, B at the stage's position from the same record (ordinary LDS reads: the compiler's own waits)
          AuxPlane P;
          load_aux_rec(0, R.off + 16, P);
          double X[5], damp, dpol;
          aux_eval(P, wb, wc, (s == 1 || s == 2) ? 0.5 : 1.0, X);
          aux_rates(V, a, X, t7, t2, t3, t4, damp, dpol);
          r7 = damp * iv;  // inside the volume (k_trace_f64: the fill-value scale fs = 1)
          r8 = dpol * iv;
        }
        if (s == 0) {
          ap0 = p0;
          ap1 = p1;
          av0 = F[0] * ivf;
          av1 = F[1] * ivf;
          av2 = F[2] * ivf;
          at = iv;
          if (PHASE) aph = F[3] * ivf;
          if (AUX) {
            a7 = r7;
            a8 = r8;
          }
        } else {
          kp0 = p0;
          kp1 = p1;
          kv0 = F[0] * ivf;
          kv1 = F[1] * ivf;
          kv2 = F[2] * ivf;
          if (PHASE) kph = F[3] * ivf;
          if (AUX) {
            k7 = r7;
            k8 = r8;
          }
          if (s < 3) {
            ap0 = fma(2.0, kp0, ap0); ap1 = fma(2.0, kp1, ap1);
            av0 = fma(2.0, kv0, av0); av1 = fma(2.0, kv1, av1); av2 = fma(2.0, kv2, av2);
            at = fma(2.0, iv, at);
            if (PHASE) aph = fma(2.0, kph, aph);
            if (AUX) {
              a7 = fma(2.0, k7, a7);
              a8 = fma(2.0, k8, a8);
            }
          }
        }
      };
      double w1b, w1c, w2b, w2c, w3b, w3c;
      // stage 1 (record RA, node plane k); places stage 2 and requests the mid record for it
      stage(std::integral_constant<int, 0>{}, std::true_type{}, y2, y3, y4, y7, RA, RB, m_cur, w1b, w1c);
      // stage 2 (mid record RB); places stage 3, which uses RB again when its cell is the same
      {
        const double t2 = fma(Shh, av2, y2), t3 = fma(Shh, av0, y3), t4 = fma(Shh, av1, y4);
        ok = ok && (t2 > 0);
        wb = w1b;
        wc = w1c;
        moved = false;
        stage(std::integral_constant<int, 1>{}, std::false_type{}, t2, t3, t4, AUX ? fma(Shh, a7, y7) : 0.0, RB, RB, 0, w2b, w2c);
        if (moved) request(m_cur, cell, RB);
      }
      // stage 3 (mid record RB); places stage 4 and requests node plane k+1 for it into RA
      {
        const double t2 = fma(Shh, kv2, y2), t3 = fma(Shh, kv0, y3), t4 = fma(Shh, kv1, y4);
        ok = ok && (t2 > 0);
        wb = w2b;
        wc = w2c;
        stage(std::integral_constant<int, 2>{}, std::true_type{}, t2, t3, t4, AUX ? fma(Shh, k7, y7) : 0.0, RB, RA, s_hi, w3b, w3c);
      }
      // stage 4 (record RA, node plane k+1); nothing to place: the next step starts from the updated state
      {
        const double t2 = fma(Sh, kv2, y2), t3 = fma(Sh, kv0, y3), t4 = fma(Sh, kv1, y4);
        ok = ok && (t2 > 0);
        wb = w3b;
        wc = w3c;
        double dummy0, dummy1;
        stage(std::integral_constant<int, 3>{}, std::false_type{}, t2, t3, t4, AUX ? fma(Sh, k7, y7) : 0.0, RA, RA, 0, dummy0, dummy1);
      }
      y0 = fma(Sh6, ap0 + kp0, y0);
      y1 = fma(Sh6, ap1 + kp1, y1);
      y2 = fma(Sh6, av2 + kv2, y2);
      y3 = fma(Sh6, av0 + kv0, y3);
      y4 = fma(Sh6, av1 + kv1, y4);
      if (PHASE) y5 = fma(Sh6w, aph + kph, y5);
      y6 = fma(Sh6, at + iv, y6);
      if (AUX) {
        y7 = fma(Sh6, a7 + k7, y7);
        y8 = fma(Sh6, a8 + k8, y8);
      }
      if (!ok || !(y2 > 0)) alive = false;  // left the tile, or turned around: k_trace_f64 takes the ray from s0
    }
#ifndef SR_TILE_EXP_NOPRODUCE
    if (REC) {
      if (more0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's two kilobytes of node plane k + 2, asked for a step ago
        mid_from(s_hi, s_nx, m_nx, true, more1);
      }
    } else if (!AUX) {
      if (producer && more) produce(NX, s_nx, s_hi, m_nx);
    } else {
      if (producer && more) {
        RawPlane t;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t.v[e].x = __int_as_float(__double2loint(NXU[2 * e]));
          t.v[e].y = __int_as_float(__double2hiint(NXU[2 * e]));
          t.v[e].z = __int_as_float(__double2loint(NXU[2 * e + 1]));
          t.v[e].w = __int_as_float(__double2hiint(NXU[2 * e + 1]));
        }
        t.l[0] = __int_as_float(__double2loint(NXU[8]));
        t.l[1] = __int_as_float(__double2hiint(NXU[8]));
        t.l[2] = __int_as_float(__double2loint(NXU[9]));
        t.l[3] = __int_as_float(__double2hiint(NXU[9]));
        produce(t, s_nx, s_hi, m_nx);
      }
      if (aproducer && more) {
        double u[4][5];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int f = 0; f < 5; ++f) u[e][f] = NXU[5 * e + f];
        produce_aux(u, s_nx, s_hi, m_nx);
      }
    }
#endif
#ifndef SR_TILE_EXP_NOBARRIER
    __syncthreads();
#endif
    if (REC) {
      nx_r0 += plane_bytes;
      nx_r1 += plane_bytes;
    }
    const int t = s_lo;
    s_lo = s_hi;
    s_hi = s_nx;
    s_nx = t;
    m_cur ^= m_nx;  // swap 3 <-> 4
    m_nx ^= m_cur;
    m_cur ^= m_nx;
  }
#undef SR_REC_WAIT

  // ---- tail
  const TileArgs *tail_args = (const TileArgs *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(tail_args));
  const TraceArgs &B = tail_args->A;
  unsigned long long tot = 0;
  // A ray this launch lost (it was a plane-form ray on node plane k0 and is not carried any more: it left the tile, the volume,
  // or turned around) becomes a straggler: its state on plane k0 -- the record it came in with; in the first segment formed
  // again from s0 -- is appended to the straggler records (one atomic per wavefront, as queue_push), and its own record says
  // where (row 0) and that it is gone (v_a = -inf).
  const bool lost = have && entered && !alive;
  {
    const unsigned long long mask = __ballot(lost);
    if (mask != 0ull) {
      const int lane = threadIdx.x & 63;
      const int leader = __ffsll((long long)mask) - 1;
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(tail_args->strag_count, (unsigned long long)__popcll(mask));
      base = __shfl(base, leader, 64);
      if (lost) {
        const int64_t g = (int64_t)(base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull)));
        double *S = tail_args->strag_rec;
        const int64_t cap = tail_args->strag_cap;
        if (tail_args->first) {
          double q0, q1, q2, q3, q4, q5, q6;
          from_s0(B, i, q0, q1, q2, q3, q4, q5, q6);
          S[g] = q0;
          S[cap + g] = q1;
          S[2 * cap + g] = q2;
          S[3 * cap + g] = q3;
          S[4 * cap + g] = q4;
          S[5 * cap + g] = q5;
          S[6 * cap + g] = q6;
          S[7 * cap + g] = B.s0[6 * N + i];
          S[8 * cap + g] = B.s0[8 * N + i];
          S[9 * cap + g] = (double)i;
        } else {
          const int64_t o = (int64_t)tail_args->order[j];
          const double *R = tail_args->rec_in;
#pragma unroll
          for (int row = 0; row < 10; ++row) S[row * cap + g] = R[row * N + o];
        }
        B.rec[j] = (double)g;
        B.rec[2 * N + j] = -__builtin_inf();
      }
    }
  }
  const bool to_rec = !tail_args->last || tail_args->exit_rec;   // the state on node plane k1 goes into the hand-off record
  if (have && tail_args->first) {  // rows 7, 8 (without the optional terms), 9 are written once and ride along from then on
    B.rec[7 * N + j] = B.s0[6 * N + i];
    B.rec[8 * N + j] = B.s0[8 * N + i];
    B.rec[9 * N + j] = (double)i;
  }
  if (to_rec) {
    if (have && !lost) {
      const double nan = __builtin_nan("");
      const bool keep = alive || gone;  // gone: y is the record as it came in, marks included
      if (AUX) {  // amp and pol move on with the ray
        B.rec[7 * N + j] = keep ? y7 : nan;
        B.rec[8 * N + j] = keep ? y8 : nan;
      }
      B.rec[j] = keep ? y0 : nan;
      B.rec[N + j] = keep ? y1 : nan;
      B.rec[2 * N + j] = keep ? y2 : nan;
      B.rec[3 * N + j] = keep ? y3 : nan;
      B.rec[4 * N + j] = keep ? y4 : nan;
      B.rec[5 * N + j] = keep ? y5 : nan;
      B.rec[6 * N + j] = keep ? y6 : nan;
    }
    // leaving a slab: the ray's steps through it are counted here (as k_trace_f64 does with SR_HANDOFF_EXIT)
    if (tail_args->last && alive) tot = (unsigned long long)(B.V.na - 1);
  } else {
    // k_strag_finish reads the marks from this buffer: EVERY slot says whether it is gone (the buffer holds whatever an earlier
    // trace left there; the lost lanes wrote theirs above)
    if (have && !lost) {
      B.rec[2 * N + j] = gone ? y2 : 0.0;
      if (gone) B.rec[j] = y0;
    }
    const bool finished = alive && y6 <= B.t_end;
    if (finished) {  // on the exit plane; vacuum to t_end (every RHS term is 0 outside the volume)
      double amp = y7, pol = y8;
      if (!AUX) {
        if (tail_args->first) {
          amp = B.s0[6 * N + i];
          pol = B.s0[8 * N + i];
        } else {  // copied there by this lane at the kernel's start
          amp = B.rec[7 * N + j];
          pol = B.rec[8 * N + j];
        }
      }
      const double rem = B.t_end - y6;
      write_outputs(B, j, fma(y2, rem, B.V.g[0][B.V.na - 1]), fma(y3, rem, y0), fma(y4, rem, y1), y2, y3, y4, y5, amp, pol);
      tot = (unsigned long long)(B.V.na - 1);
    }
    if (tail_args->slab) {
      if (have && !finished && !lost && !gone) write_lost(B, j);
    } else {
      queue_push(B.out_count, B.out_list, have && !finished && !lost && !gone, (uint32_t)j);  // never a plane-form ray here: the usual levels, from s0
    }
  }
  for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
  if ((threadIdx.x & 63) == 0 && tot) atomicAdd(sr::stripe(B.counters, B.step_stripe), tot);
}
