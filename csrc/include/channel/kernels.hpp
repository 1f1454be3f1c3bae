// Host-side launchers for the HIP kernels (implemented in csrc/kernels/*.hip).
#pragma once

#include <string>

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "channel/grid.hpp"
#include "channel/yline_device.hpp"

namespace channel {

// R values the y-line kernels are instantiated for (64*R >= NY).
int yline_supported_R(int NY);
// K-SPEC line geometry for NY: R rows per lane on H waves per line.  Default H = 1 (one wave per
// line, 64 R >= NY); CHANNEL_KSPEC_HALVES=1 opts in to lines over two waves (H = 2, 64 R H >= NY),
// measured slower at the headline grid and checked against the oracle by
// tests/test_solver_gpu.py::test_kspec_halves_matches_oracle
void kspec_geometry(int NY, bool fp64, int& R, int& H);

// Device copies of the per-row coefficient tables (lane-major, see yline_device.hpp).  H = 2: row
// j = h 64R + lane R + r of half h at index (h R + r) 64 + lane (a half's table is the one-wave
// table of its rows), the D1 factorisation per half, and the halves' D1 spikes.
struct YTablesDev {
  double* buf = nullptr;     // single allocation
  size_t bytes = 0;
  dev::YTab tab{};
  int R = 1, H = 1;
  void upload(const YGrid& g, int R, hipStream_t stream, int H = 1);
  void release();
  ~YTablesDev() { release(); }
};

// Debug/test entry point: apply one y-line operator to `lines` complex lines stored [y][line].
enum YLineOp : int {
  YOP_D1 = 0,        // out = D1 in (compact first derivative)
  YOP_HELM = 1,      // out = (K - k^2 M)^{-1} M in, out(+-1) = 0 (velocity recovery)
  YOP_IMPL = 2,      // out = ((1+c k^2) M - c K)^{-1} M in, out(+-1)=0 (implicit viscous step)
  YOP_MAPPLY = 3,    // out = M in (interior rows, 0 on walls)
  YOP_KAPPLY = 4,    // out = K in (interior rows, 0 on walls)
};
void yline_test(const YTablesDev& t, int op, const void* in, void* out, int lines, const double* k2, double c,
                bool fp64, hipStream_t stream);

// Dense D1 = A1^-1 B1 (NY <= 192) applied to [y][line] complex fp64 lines on the matrix cores
// (yline_mfma.hip): the measured MFMA alternative to the PCR D1 solve.
struct DenseD1Dev {
  double* d = nullptr;  // [NP][NP] row-major, zero-padded
  int N = 0, NP = 0;
  void upload(const YGrid& g, hipStream_t stream);
  void release();
  ~DenseD1Dev() { release(); }
};
void d1_dense_mfma(const DenseD1Dev& m, const void* in, void* out, int lines, hipStream_t stream);

// ---- spectral field layout ----------------------------------------------------------------------
// Element (y, line) of a spectral field, line = local kx * nkzs + local kz (nkzs: the kz line
// stride), lines = nkx_loc * nkzs.  kzb = 0: [y][line], every y plane contiguous (the exchange
// blocks of P > 1 are row ranges).  kzb = 8 (one rank, nkzs a multiple of 8, rows padded to a
// multiple of 8): tiles of 8 planes x 8 kz lines, [y / 8][line / 8][y % 8][line % 8], i.e. a 512-B
// (fp32) piece per (8-plane chunk, kz block).  The spectral fields are read in two shapes: K-SPEC
// tiles (4 lines x all y: 49 such pieces instead of 385 rows of 32 B, 1.9 MB apart) and the
// x transforms (2 planes x 8 kz x all kx: 128-B lines, the kx rows of one chunk 22 KB apart);
// tools/tilebench.hip: K-SPEC's pattern 2.5 -> 4.2 TB/s blocked.  Blocking all NY rows of a kz
// block instead ([kz/8][kx][y][8]) gave K-SPEC whole-tile contiguity but spread an x tile over
// 16.8 MB and the chunk's tiles over the whole field: the x-backward's average read latency rose
// from 950 to 1670 cycles (TCP_TCC_READ_REQ_LATENCY, gpurun_out/r4g*), 62 -> 71 us per chunk.
// Row and line parts of the offset are separable: offset = spec_row_off(y) + spec_line_off(line),
// and spec_row_off(y + 64) = spec_row_off(y) + 64 lines in both layouts.
constexpr int kSpecKzBlock = 8, kSpecYBlock = 8;
__host__ __device__ inline size_t spec_row_off(int kzb, int lines, int y) {
  return kzb ? static_cast<size_t>(y / kSpecYBlock) * kSpecYBlock * lines + (y % kSpecYBlock) * kSpecKzBlock
             : static_cast<size_t>(y) * lines;
}
__host__ __device__ inline size_t spec_line_off(int kzb, int line) {
  return kzb ? static_cast<size_t>(line / kSpecKzBlock) * (kSpecYBlock * kSpecKzBlock) + line % kSpecKzBlock
             : static_cast<size_t>(line);
}
__host__ __device__ inline size_t spec_index(int kzb, int nkx, int nkzs, int y, int ikx, int kz) {
  return spec_row_off(kzb, nkx * nkzs, y) + spec_line_off(kzb, ikx * nkzs + kz);
}
// rows allocated per spectral field (kzb: whole 8-plane chunks)
__host__ __device__ inline int spec_rows(int kzb, int N) { return kzb ? (N + kSpecYBlock - 1) / kSpecYBlock * kSpecYBlock : N; }

// ---- the fused spectral (y-line) substep kernel ---------------------------------------------
struct SpecArgs {
  // geometry
  int N = 0;              // NY
  int lines = 0;          // local lines = nkx_loc * nkz, line = ikx_local * nkz + kz
  int nkz = 0, kx0 = 0, nkx = 0, Kx = 0;   // nkz = local kz line stride (pencil: a kz range; kzb: padded to 8)
  int kzb = 0;            // spectral layout (spec_index)
  int kz0 = 0;            // first local kz (pencil)
  double ax = 1, az = 2;  // 2 pi / LX, 2 pi / LZ
  double nu = 1.0 / 3250.0;
  // RK3 substep (mode 1)
  int mode = 0;           // 0 = prepare only (fields from state), 1 = advance + prepare
  double rk_a = 0, rk_b = 0, rk_g = 0, rk_z = 0;
  const double* dt = nullptr;   // device scalar
  // mean flow forcing
  double Q = 1.8;
  int forcing = 0;        // 0 implicit (exact flux), 1 parity (constant add)
  // reference-parity switches (config influence / explicit_d2; every NY)
  bool explicit_dd = false;          // explicit viscous D2 = D1 o D1
  bool analytic_influence = false;   // cosh/sinh influence functions
  const double* ygrid = nullptr;     // [N] y_j (analytic influence)
  // fields (T2* cast to void*)
  void* phi = nullptr;
  void* omega = nullptr;  // line (0,0) holds U(y)
  void* Rphi = nullptr;
  void* Romega = nullptr;
  void* out[6] = {};      // out6 = 1: u, v, w, omega_x, -, omega_z (out[4] == omega: the state is the
                          // omega_y source, the x-backward zeroes its mean line); out6 = 0 (the
                          // combine mode of P > 1): D1 v, v, D1 omega in out[0..2], out[3], out[5]
                          // unused (XArgs::combine forms u, w, omega_x, omega_z from D1 v, omega,
                          // phi, D1 omega).  out[0..2] double as the H_x, H_y, H_z inputs.
  int out6 = 1;
  int store_r = 1;        // 0: skip the R_phi/R_omega stores (last substep: the next one has zeta = 0)
  int lds_poison = 0;     // debug: fill the LDS with NaN before use (CHANNEL_LDS_POISON)
  // diagnostics
  // plane statistics when stats_part is non-null: workgroup b adds its tiles' sums (uu, vv, ww, uv)
  // to row b of stats_part [stats_blocks][stats_stride] (zeroed by the caller, accumulated over the
  // launches of a substep); kspec_stats_reduce forms the [4][N] plane sums from it.  stats_stride
  // is the slot count 4 * 64 R H of the tables (a compile-time constant in the kernels) and
  // stats_blocks >= the grid (kspec_grid_capacity): both checked at the launch.
  double* stats_part = nullptr;
  int stats_stride = 0, stats_blocks = 0;
  double* mean_diag = nullptr;  // [3N + 8]: U, Nx, dU/dy(walls), flux, pressure gradient ...
  unsigned* health = nullptr;   // bit 0: non-finite state
  unsigned long long* prof = nullptr;  // [kKspecPhases] shader-clock sums per phase (debug, CHANNEL_KSPEC_PROF)
};
constexpr int kKspecPhases = 10;
void kspec_launch(const YTablesDev& t, const SpecArgs& a, bool fp64, hipStream_t stream);
// the largest grid (workgroups) kspec_launch runs for these tables and arguments (the switches of
// the environment included): the rows SpecArgs::stats_part needs
int kspec_grid_capacity(const YTablesDev& t, const SpecArgs& a, bool fp64);
// stats[4][N] = the sum over rows 0 .. blocks-1, in that order, of part[blocks][stride], each slot
// mapped to the plane it stands for (kspec_kernel's row map for t.R, t.H)
void kspec_stats_reduce(const YTablesDev& t, const double* part, int stride, int blocks, double* stats, hipStream_t stream);
// kernel name(s) of this thread's last K-SPEC launch in rocprofv3's kernel-name form, template
// arguments R, T, W, NS, XM, PAR, GLM, SPLIT, H ("kspec_kernel<7, float, 4, 2, 2, 0, 0, 0, 1>"); the
// split (CHANNEL_KSPEC_SPLIT=1) reads "kspec_kernel<..., 1, 1> + kspec_out_kernel<R, T, W, XM>" (tests)
std::string kspec_last_variant();

// ---- pressure (y-line Poisson solve, outside the step) ---------------------------------------
// Per line with k2 > 0: (K - k2 M) Pi = M S on the interior rows, S = i al Hx + i be Hz + D1 Hy, and
// (D1 Pi)(+-1) = Hy(+-1) + nu phi(+-1) at the walls, solved as Pi = Pi_p + c1 g1 + c2 g2 with the
// Dirichlet Helmholtz factorisation (right-hand sides M S, e_0, e_N) and the 2 x 2 system of the
// dense D1's wall rows (pressure.hip).  Pi = p + |u|^2 / 2; the mean line, padded kz lines (local kz
// >= nkz_real) and rows >= N of the blocked layout are written as zero.  pi may be hx (in place).
struct PressureArgs {
  int N = 0;              // NY
  int lines = 0;          // local lines = nkx_loc * nkz, line = ikx_local * nkz + kz
  int nkz = 0, nkz_real = 0, kx0 = 0, nkx = 0, Kx = 0;  // nkz = kz line stride (kzb: padded to 8)
  int kzb = 0;            // spectral layout (spec_index)
  int kz0 = 0;
  double ax = 1, az = 2;  // 2 pi / LX, 2 pi / LZ
  double nu = 1.0 / 3250.0;
  const void* hx = nullptr;   // H = u x omega (what the step's transform stage writes)
  const void* hy = nullptr;
  const void* hz = nullptr;
  const void* phi = nullptr;  // the state (its two wall rows are read)
  void* pi = nullptr;
};
void pressure_solve(const YTablesDev& t, const PressureArgs& a, bool fp64, hipStream_t stream);

// ---- passive scalar (y-line advance of one RK3 substep) ----------------------------------------
// Per line, all in fp64 (scalar.hip): N = -(i al Fx + D1 Fy + i be Fz) (mean line: Re N + source), R_n = M N,
//   r = M th + dt [rk_a kappa (K th - k2 M th) + rk_g R_n + rk_z R_prev], wall rows of r zero (mean line:
//   lower, upper), th_new = ((1 + c k2) M - c K, identity wall rows)^-1 r with c = rk_b dt kappa.
// th is advanced in place and R_n stored over R_prev (store_r); the mean line's imaginary part, the padded
// kz lines (local kz >= nkz_real) and the rows >= N of the blocked layout are written as zero.
struct ScalarArgs {
  int N = 0;              // NY
  int lines = 0;          // local lines = nkx_loc * nkz, line = ikx_local * nkz + kz
  int nkz = 0, nkz_real = 0, kx0 = 0, nkx = 0, Kx = 0;  // nkz = kz line stride (kzb: padded to 8)
  int kzb = 0;            // spectral layout (spec_index)
  int kz0 = 0;
  double ax = 1, az = 2;  // 2 pi / LX, 2 pi / LZ
  double kappa = 1.0;     // 1 / (Re Pr)
  double rk_a = 0, rk_b = 0, rk_g = 0, rk_z = 0;
  const double* dt = nullptr;  // device scalar
  double lower = 0, upper = 0, source = 0;  // Theta(-1), Theta(+1), uniform source (mean line)
  const void* fx = nullptr;   // (u theta)^, (v theta)^, (w theta)^ of the substep's state
  const void* fy = nullptr;
  const void* fz = nullptr;
  void* th = nullptr;
  void* Rth = nullptr;
  int store_r = 1;        // 0: skip the R store (last substep: the next one has zeta = 0)
  int lds_poison = 0;     // debug: fill the LDS with NaN before use
  unsigned* health = nullptr;  // bit 0: non-finite state
};
void scalar_advance(const YTablesDev& t, const ScalarArgs& a, bool fp64, hipStream_t stream);

// ---- FFT stages ---------------------------------------------------------------------------
// Per-pass FFT twiddle tables for length n (FftPlan T1/T2 layout, fft_device.hpp), fp32 or fp64.
struct Twiddles {
  void* buf = nullptr;
  void* reg = nullptr;  // n = 1024: [M][64] W_N^(n1 k2), [4][16] W_64^(a c) of the register z stage
  int n = 0;
  bool fp64 = false;
  void build(int n, bool fp64);
  void release();
  ~Twiddles() { release(); }
};
// Source of a spectral field for the backward x-transform: for P ranks the blocks received from
// each source rank s hold [y_local][nkx_s][nkz] starting at element offset off[s].
// Blocks self_seg .. self_seg + nself - 1 (this rank's own kx range, if self_seg >= 0; several when
// the rank's spectral fields are stored as kx sub-blocks, Solver::nkb_) live at self_base + f *
// self_field_stride + off[s] instead (the spectral field itself: no self exchange, no copy).
// exchange segments of the x transforms: P ranks x kx sub-blocks (slab8 with 2 sub-blocks: 16)
constexpr int kMaxSeg = 16;
struct XSrc {
  const void* base = nullptr;
  // combine mode (XArgs::combine): input field j (0 D1 v, 1 v, 2 D1 omega, 3 omega, 4 phi) at fld[j]
  // (the exchange blocks or the spectral field: base is unused) and its self blocks at self_fld[j]
  const void* fld[5] = {};
  const void* self_fld[5] = {};
  int nsrc = 1;
  int kx_start[kMaxSeg + 1] = {0};   // global retained-kx start of source s (kx_start[nsrc] = nkx)
  long long off[kMaxSeg] = {0};      // element offset of source block s
  int self_seg = -1;
  int nself = 1;
  const void* self_base = nullptr;
  long long self_field_stride = 0;
  // per-row table of the exchange segments (row-table modes, optional): for each retained kx row i,
  // rowtab[2 i] = element offset of row i at segment row Y = 0 of the FIRST chunk (y0 = 0),
  // rowtab[2 i + 1] = its segment's Y stride | 0x80000000 for a self block.  Chunk rows then add
  // XArgs::seg_y0 to Y.  Built once per run on the host (Solver::build_rowtab) instead of per launch.
  const unsigned* rowtab = nullptr;
};
struct XDst {             // destination blocks for the forward x-transform (per destination rank)
  void* base = nullptr;
  int ndst = 1;
  int kx_start[kMaxSeg + 1] = {0};
  long long off[kMaxSeg] = {0};
  int self_seg = -1;
  int nself = 1;
  void* self_base = nullptr;
  long long self_field_stride = 0;
  const unsigned* rowtab = nullptr;  // as XSrc::rowtab
};

// ---- x-expanded layout ---------------------------------------------------------------------------
// The intermediates between the x and z transforms are [y][x][kz] complex rows of row pitch
// `xpitch` elements.  xpitch = 0 (or nkz): rows packed at nkz elements (the P > 1 segment paths and
// every caller that does not set it).  One rank: the pitch is rounded up to kXexpAlign elements
// (xexp_pitch: whole 128-B lines in fp32), so the 64-B tile pieces of the x kernels never straddle a
// 64-B boundary and a z row starts on a line; the columns kz >= nkz of a row are padding that is
// neither read as data nor written (profiles/xexp/README.md).
constexpr int kXexpAlign = 16;
constexpr bool kXexpPaddedDefault = true;  // the one-rank solver's layout when CHANNEL_XEXP_LAYOUT is unset
__host__ __device__ constexpr int xexp_pitch(int nkz) { return (nkz + kXexpAlign - 1) / kXexpAlign * kXexpAlign; }

struct XArgs {
  int NX = 0, nkx = 0, Kx = 0, nkz = 0, ny = 0;   // ny = local y planes, nkz = local kz count
  int xpitch = 0;                    // x-expanded row pitch (one segment only); 0 = nkz
  int nfields = 1;
  long long field_stride_spec = 0;   // element stride between fields in the spectral buffers
  long long field_stride_phys = 0;   // element stride between fields in the physical buffers
  // x-expanded buffer blocked by x range (pencil B exchange): x in [x_start[d], x_start[d+1]) lives
  // at poff[d] + (y * nx_d + x - x_start[d]) * nkz.  One segment = plain [y][x][kz].
  int npseg = 1;
  int x_start[9] = {0};
  long long poff[8] = {0};
  int diag = 0;                      // bit 0: skip the transforms (timing diagnosis, CHANNEL_FFT_DIAG)
  // backward only: field zero_mean_field's (kx = 0, kz = 0) element is read as 0 (omega_y: the
  // spectral source is the omega state, whose mean line holds U(y)); kz_glob0 = global kz of local
  // kz 0 (pencil rows)
  int zero_mean_field = -1;
  int kz_glob0 = 0;
  int lds_poison = 0;                // debug: fill the LDS with NaN before use
  // blocked spectral layout (one rank, one source block; spec_index with kzb = 8): rows spec_y0 ..
  // spec_y0 + ny - 1 of fields of line stride nkzs (lines = nkx * nkzs)
  int kzb = 0, nkzs = 0, spec_y0 = 0;
  // P > 1: the exchange segments and self blocks hold the blocked layout too (spec_index with
  // kzb = 8 within each segment: [y/8][line/8][y%8][line%8], line = kx in segment * nkzs + kz;
  // chunk rows start on 8-plane tiles).  fft_impl.hpp seg_yk / seg_stride
  int segblk = 0;
  int seg_y0 = 0;                    // with XSrc / XDst::rowtab: the chunk's first segment row Y
  int seg_yoff = 0;                  // rows of the exchange chunk before this launch's first row (the
                                     // second part of a chunk split over two compute streams)
  int nt = 0;                        // streaming (non-temporal) spectral accesses (solver default 1;
                                     // CHANNEL_XNT=0 off: 35.0 vs 34.75 ms/step, profiles/r04/ab_xnt.txt)
  // backward only: combine mode -- the six output fields u, v, w, omega_x, omega_y, omega_z are
  // formed per element from the five inputs XSrc::fld (D1 v, v, D1 omega, omega, phi; fft_impl.hpp
  // cmb_pair); ax, az = 2 pi / LX, 2 pi / LZ (the kx of retained row i, the kz of kz_glob0 + kz)
  int combine = 0;
  double ax = 1.0, az = 2.0;
};
// backward: spectral (truncated kx) -> [y][x][kz] complex (row pitch XArgs::xpitch), zero padding kx
void xfft_backward(const XArgs& a, const XSrc& src, void* phys, const Twiddles& tw, bool fp64, hipStream_t s);
// forward: [y][x][kz] -> spectral truncated kx (unnormalised)
void xfft_forward(const XArgs& a, const void* phys, const XDst& dst, const Twiddles& tw, bool fp64, hipStream_t s);
// template arguments of this thread's last x-transform launch, in rocprofv3's kernel-name form (tests)
std::string xfft_last_variant();
// the same for this thread's last x-backward launch (a solver step ends with forward transforms)
std::string xfft_last_backward_variant();

struct ZArgs {
  int NX = 0, Nzp = 0, nkz = 0, ny = 0, y0 = 0;   // NX = local x count (rows = ny * NX)
  int xpitch = 0;                    // row pitch (one segment of all Nzp/3 + 1 kz only): 0 = nkz, or xexp_pitch(nkz)
  // rows blocked by kz range (pencil B exchange): kz in [kz_start[s], kz_start[s+1]) of row r lives
  // at off[s] + r * nkz_s + kz - kz_start[s].  One segment = plain [row][kz].
  int nseg = 1;
  int kz_start[9] = {0};
  long long off[8] = {0};
  int diag = 0;                      // bit 0: skip the transforms (timing diagnosis)
  long long field_stride = 0;        // element stride between the 6 input fields
  double scale = 1.0;                // forward normalisation 1/(NX*Nzp)
  const double* inv_dy = nullptr;    // [NY] 1/local spacing for the CFL estimate
  double cx = 0, cz = 0;             // kx_max, kz_max for the CFL estimate
  float* maxima = nullptr;           // [4]: |u|max, |v|max, |w|max, cfl sum max (atomicMax)
  int lds_poison = 0;                // debug: fill the LDS with NaN before use
};
// template arguments of this thread's last zphys_kernel launch, in rocprofv3's kernel-name form (the
// last argument: pair 1 of the next row staged in the per-wave LDS slot; tests)
std::string zphys_last_variant();
// physical-space stage: 6 fields (u,v,w,wx,wy,wz) [y][x][kz] -> z C2R -> H = u x omega -> z R2C
// -> truncated H_x,H_y,H_z written in place over fields 0..2.
void zphys(const ZArgs& a, void* fields, const Twiddles& tw, bool fp64, hipStream_t s);

// export stage (on request, outside the step): the z complex-to-real transform of an x-expanded
// chunk [f][row][kz] (row = y_local * NX + x, nkz = Nzp/3 + 1, row pitch xpitch, one segment: what xfft_backward
// writes and zphys reads) into real rows, and/or the one-point moments of u, v, w per plane
constexpr int kMomRows = 11;  // u', u'^2, v'^2, w'^2, u'v', u'^3, v'^3, w'^3, u'^4, v'^4, w'^4
struct ZRealArgs {
  int NX = 0, Nzp = 0, nkz = 0, ny = 0;   // rows = ny * NX
  int xpitch = 0;                    // row pitch of the inputs and of spec_out (0 = nkz)
  int y0 = 0;                        // global plane of the chunk's first plane (moments, U)
  int nfields = 0;                   // transformed fields, in pairs (an odd count: the last with zero)
  long long field_stride = 0;        // element stride between the input fields
  // real output (T = float | double by storage precision), optional: field f with bit f of
  // out_mask set goes to out[slot][plane][x][z], slot = its rank among the set bits
  void* out = nullptr;
  unsigned out_mask = 0;
  long long out_field_stride = 0;    // real elements between slots
  // moments (optional; needs nfields >= 3 = u, v, w): plane means over NX * Nzp points of the
  // kMomRows products of u' = u - U(y), v, w, accumulated (+=) into moments[kMomRows][NY]
  double* moments = nullptr;
  const double* U = nullptr;         // device [NY]
  int NY = 0;
  // mixed triple products (optional; with moments, nfields == 3 and no real output): plane means of
  // u'u'v, w w v, u'v v accumulated (+=) into triple[kTripleRows][NY].  The second pair is then
  // transformed as (w, v) instead of (w, 0), so w and v meet in the same registers.
  double* triple = nullptr;
  // pressure mode (optional; nfields == 4, field 3 = Pi' = p + |u|^2 / 2 without its plane mean, U set,
  // no triple): the second pair is (w, Pi') and r = Pi' - U u' - (u'^2 + v^2 + w^2) / 2, the static
  // pressure up to its plane mean, is formed per point from the u', v kept from the first pair; bit 3 of
  // out_mask exports r in the place of field 3, and pmom (optional) accumulates (+=) the plane means of
  // r, r^2, r u', r v, r w into pmom[kPresRows][NY] (products in double)
  int pres = 0;
  double* pmom = nullptr;
  // return trip of r (optional; with pres, an instantiation of its own): r goes back into the row's
  // LDS slots as (r, 0), is forward transformed and its retained kz (k < nkz), scaled by 1 / (NX Nzp),
  // are stored as complex [row][kz] at spec_out, x-expanded like the inputs (what xfft_forward reads).
  // spec_out may be the place of field 3: a row's Pi is loaded before its r is stored.
  void* spec_out = nullptr;
  // histograms (optional, with hist set; an instantiation of its own with one plane per block: grid =
  // ny * ceil(NX / rows per block); no real output, moments or pressure mode beside it): nhf = nfields =
  // 3 (u, v, w) or 6 (+ omega_x, omega_y, omega_z) fields, nb bins per 1-D histogram, nj | nb bins per
  // axis of the joint histogram of (u, v).  A sample x of field f at plane y, widened to double, has
  // i = floor((x - hcentre[f][y]) * hscale[f][y] + nb / 2) (product and sum rounded separately) and goes
  // to bin 0 (i < 0 or not a number), nb + 1 (i >= nb) or i + 1; its joint bin per axis is 0, nj + 1 or
  // i / (nb / nj) + 1.  Counts are accumulated (+=) into hist[nhf][NY][nb + 2] and joint[NY][nj + 2][nj + 2]
  // (first index: u), and quad[8][NY] receives (+=) the sums of u'v over the quadrants Q1 (u' >= 0,
  // v >= 0), Q2 (-, +), Q3 (-, -), Q4 (+, -) of u' = u - U(y), then the four sample counts, unscaled.
  int nhf = 0, nb = 0, nj = 0;
  const double* hcentre = nullptr;   // device [nhf][NY]
  const double* hscale = nullptr;    // device [nhf][NY], nb / (2 halfwidth)
  unsigned long long* hist = nullptr;
  unsigned long long* joint = nullptr;
  double* quad = nullptr;
  int hmerge = 1;                    // equal consecutive bins of a thread's 16-byte piece in one LDS atomic
};
constexpr int kTripleRows = 3;  // u'u'v, wwv, u'vv
constexpr int kPresRows = 5;    // r, r^2, r u', r v, r w
constexpr int kQuadRows = 8;    // sums of u'v over Q1..Q4, then their sample counts
constexpr int kHistMaxBins = 256, kHistMaxJoint = 64;  // the block's LDS tables (zreal refuses more)
void zreal(const ZRealArgs& a, const void* fields, const Twiddles& tw, bool fp64, hipStream_t s);

// z stage of the passive scalar: per row of an x-expanded chunk [4 fields][row][kz] (u, v, w, theta; the
// layout zphys reads) the C2R transforms of the pairs (u, v) and (w, theta), the products u theta,
// v theta, w theta in the storage precision, one forward transform of u theta + i v theta split by
// conjugate symmetry and one of (w theta, 0); the retained kz (k < nkz), scaled by 1 / (NX Nzp), are
// stored over fields 0..2 of the row.  A row loads its four inputs before it stores.
struct ZScalarArgs {
  int NX = 0, Nzp = 0, nkz = 0, ny = 0;   // rows = ny * NX
  int xpitch = 0;                    // row pitch (0 = nkz)
  long long field_stride = 0;        // element stride between the four fields
  int lds_poison = 0;                // debug: fill the LDS with NaN before use
};
void zscalar(const ZScalarArgs& a, void* fields, const Twiddles& tw, bool fp64, hipStream_t s);

// standalone FFT entry points for tests: batched C2C along the contiguous axis
void fft_c2c_test(void* data, int n, int batch, int dir, const Twiddles& tw, bool fp64, hipStream_t s);

// ---- small kernels ---------------------------------------------------------------------------
struct DtArgs {
  float* maxima = nullptr;   // [4] from zphys; reset to 0 after use
  double* dt = nullptr;      // output dt (device)
  double* time = nullptr;    // accumulated time (device)
  double* dt_log = nullptr;  // [8]: umax vmax wmax cflsum dt_c dt_v dt ...
  unsigned* health = nullptr;  // bit 1 set on non-finite CFL maxima or dt collapse
  double cfl = 0.5, dt_max = 0.05, dt_fixed = 0.0;
  int parity = 0;
  double NX = 0, NZ = 0, LX = 0, LZ = 0, Re = 0, dy_uniform = 0;
};
void dt_update(const DtArgs& a, hipStream_t s);

// kz=0 plane Hermitian symmetrisation of a [y][nkx][nkz] field held entirely by one rank
void symmetrize_kz0(void* q, int N, int nkx, int nkzs, int Kx, int kzb, bool fp64, hipStream_t s);
// distributed version: pack the local kz=0 column [y][kx_loc], exchange, symmetrise from the
// gathered columns (blocks [c][y][nkx_c] of the ranks of this process row)
struct Kz0SymArgs {
  int N = 0, nkx_loc = 0, nkz_loc = 0, kx0 = 0, nkx = 0;
  int kzb = 0;  // spectral layout of q (spec_index; nkz_loc is then the padded line stride nkzs)
  int nblk = 1;
  int kx_start[kMaxSeg + 1] = {0};
};
void kz0_pack(const void* q, void* col, int N, int nkx_loc, int nkz_loc, int kzb, bool fp64, hipStream_t s);
void kz0_symmetrize_dist(void* q, const void* col_all, const Kz0SymArgs& a, bool fp64, hipStream_t s);

// ---- diagnostics ---------------------------------------------------------------------------
struct SpectraArgs {
  // spectral [NY][lines] fields, lines = nkx_loc*nkz_loc: the K-SPEC outputs D1 v, v and the omega
  // state; u = i (al D1v - be om)/k2 and w = i (be D1v + al om)/k2 are formed per element
  const void *dv = nullptr, *v = nullptr, *om = nullptr;
  double ax = 1.0, az = 2.0;
  // combine = 0 (K-SPEC's six-output mode): u and w are stored fields themselves
  int combine = 1;
  const void *u = nullptr, *w = nullptr;
  int lines = 0, nkx_loc = 0, kx0 = 0, nkz_loc = 0, kz0 = 0;
  int nkzs = 0, kzb = 0;              // line stride in kz, layout (spec_index)
  int nkx = 0, Kx = 0, nkz = 0;       // global retained counts
  const int* planes = nullptr;        // device [nplanes] y indices
  int nplanes = 0;
  double* ekx = nullptr;              // [3][nplanes][Kx+1]  (|kx| bins, summed over kz)
  double* ekz = nullptr;              // [3][nplanes][nkz]   (summed over kx)
  double* map = nullptr;              // [3][nkx][nkz] |q|^2 at planes[0] (may be null)
};
// accumulates (+=) into ekx/ekz; map is overwritten for the local block
void spectra_accumulate(const SpectraArgs& a, bool fp64, hipStream_t s);
// What the three all-plane reductions below read: one local block of spectral fields, walked once.
struct SpecWalkArgs {
  // six-output mode: u, v, w, omega_x, omega_y (the omega state), omega_z; combine mode: D1 v, v,
  // D1 omega, omega, phi (f[5] unused), from which u, w, omega_x, omega_z are formed per element.
  // A reduction needs only the fields its rows use.
  const void* f[6] = {};
  const void* p = nullptr;            // p-hat' in the layout of the fields (pressure strain; optional for the spectra)
  int combine = 0;
  double ax = 1.0, az = 2.0;
  int N = 0;                          // NY (rows beyond it, the blocked layout's padding, are skipped)
  int nkx_loc = 0, kx0 = 0, nkz_loc = 0, kz0 = 0;
  int nkzs = 0, kzb = 0;              // line stride in kz (lines past nkz_loc are skipped), layout (spec_index)
  int nkx = 0, Kx = 0;                // global retained kx count
};
// Velocity-gradient plane sums of the current state (vorticity r.m.s., dissipation): every plane of
// one local block of spectral fields is read once and kGradRows Parseval sums per plane are
// accumulated (+=) into sums[kGradRows][N].  Weights as SpectraArgs (kz = 0 once, kz > 0 twice, the
// mean line skipped); the wall-normal derivatives are the solver's own, D u = i al v - omega_z,
// D w = omega_x + i be v, D v = -i (al u + be w), so no y-solve is needed.  Rows: |omega_x|^2,
// |omega_y|^2, |omega_z|^2, g_uu = k2 |u|^2 + |D u|^2, g_vv, g_ww, g_uv = k2 Re(u v*) + Re(Du Dv*).
constexpr int kGradRows = 7;
struct GradSumArgs : SpecWalkArgs {   // all six fields (p unused)
  double* sums = nullptr;             // [kGradRows][N]
};
void gradsum_accumulate(const GradSumArgs& a, bool fp64, hipStream_t s);
// Pressure-strain plane sums: the Parseval products of the spectral fluctuating static pressure p with
// the strain factors of the current state, read once like the gradient sums (same walk, weights and
// masks: kz = 0 once, kz > 0 twice, the mean line and the padded lines skipped; products and sums in
// double) and accumulated (+=) into sums[kPStrainRows][N].  The wall-normal derivatives are the
// solver's own: D u = i al v - omega_z, D v = -i (al u + be w).  Rows:
//   ps_uu = 2 Re<p (i al u)*>, ps_vv = 2 Re<p (D v)*>, ps_ww = 2 Re<p (i be w)*>,
//   ps_uv = Re<p (D u + i al v)*>, pu = Re<p u*>, pv = Re<p v*>, pp_band = <|p|^2>.
constexpr int kPStrainRows = 7;
struct PStrainArgs : SpecWalkArgs {   // p and, in six-output mode, only u, v, w, omega_z (f[3], f[4] unused)
  double* sums = nullptr;             // [kPStrainRows][N]
};
void pstrain_accumulate(const PStrainArgs& a, bool fp64, hipStream_t s);
// Scalar plane sums: the Parseval products of the passive scalar theta (in the place of p) with itself and
// the velocities of the current state, read once like the gradient sums (same walk, weights and masks)
// and accumulated (+=) into sums[kScalarSumRows][N]: |theta|^2, Re(u theta*), Re(v theta*), Re(w theta*).
constexpr int kScalarSumRows = 4;
struct ScalarSumArgs : SpecWalkArgs {  // p = theta-hat and u, v, w
  double* sums = nullptr;             // [kScalarSumRows][N]
};
void scalarsum_accumulate(const ScalarSumArgs& a, bool fp64, hipStream_t s);
// One-dimensional spectra and co-spectra at every plane: one local block of spectral fields is read
// once, like the gradient sums (same inputs, weights and masks: kz = 0 once, kz > 0 twice, the mean
// line and the padded lines skipped; products and sums in double), and per plane the products are
// accumulated (+=) by |kx| (+kx and -kx folded, summed over kz) and by global kz (summed over kx).
// Summing either output over its wavenumber gives the plane mean of the product.  Rows: |u|^2, |v|^2,
// |w|^2, Re(u v*), |omega_x|^2, |omega_y|^2, |omega_z|^2, |p|^2 (left untouched when p is null).
constexpr int kYSpecRows = 8;
struct YSpectraArgs : SpecWalkArgs {  // all six fields; p or null
  int nkz = 0;                        // global retained kz count
  double* ekx = nullptr;              // [kYSpecRows][N][Kx + 1]
  double* ekz = nullptr;              // [kYSpecRows][N][nkz]
};
void yspectra_accumulate(const YSpectraArgs& a, bool fp64, hipStream_t s);
// Spectral Reynolds-stress budgets at every plane: the terms of the uu, vv, ww, uv budgets per (y, |kx|)
// and per (y, kz), accumulated (+=) like the spectra above (same walk, weights, masks and outputs, with
// kSBudRows rows).  With a.b = Re(a b*), H' = H - H_lin the transform of u' x omega' (H = (u x omega)^,
// H_lin = (-U' v, U' u - U omega_z, U omega_y)), G = Pi - U u the transform of p' + |u'|^2 / 2, p the
// fluctuating static pressure and D the solver's own wall-normal derivatives (GradSumArgs), the rows are
//    0..3   n_uu = u.H'x, n_vv = v.H'y, n_ww = w.H'z, n_uv = u.H'y + v.H'x
//    4..7   g_uu, g_vv, g_ww, g_uv: the summands of the gradient sums' rows 3..6
//    8..11  gs_uu = 2 G.(i al u), gs_vv = 2 G.Dv, gs_ww = 2 G.(i be w), gs_uv = G.(Du + i al v)
//   12..13  gu = G.u, gv = G.v
//   14..19  ps_uu, ps_vv, ps_ww, ps_uv, pu, pv: the summands of the pressure strain's rows 0..5
// in two stages, because H and Pi share a buffer: stage 0 (rows 0..7) reads the six fields and h = H_x,
// H_y, H_z; stage 1 (rows 8..19) reads u, v, w, omega_z, h[0] = Pi and p.
constexpr int kSBudRows = 20;
constexpr int kSBudStage0Rows = 8;    // rows of stage 0; stage 1 has the rest
struct SBudgetArgs : SpecWalkArgs {
  const void* h[3] = {};              // stage 0: H_x, H_y, H_z; stage 1: Pi (h[1], h[2] unused), in the layout of the fields
  const double* U = nullptr;          // [N] mean profile
  const double* dU = nullptr;         // [N] its wall-normal derivative (stage 0)
  int stage = 0;
  int nkz = 0;                        // global retained kz count
  double* ekx = nullptr;              // [kSBudRows][N][Kx + 1]
  double* ekz = nullptr;              // [kSBudRows][N][nkz]
};
void sbudget_accumulate(const SBudgetArgs& a, bool fp64, hipStream_t s);
// Cross-spectra of every plane against a few reference planes: with e = a(kx, kz, y) conj(b(kx, kz, y_r))
// of every stored element (walk, weights and masks of the spectra above: kz = 0 once, kz > 0 twice, the
// mean line and the padded lines skipped; products and sums in double), per reference plane r and plane y
//   ckx[|kx|] += wgt (kx > 0 ? e : kx < 0 ? conj(e) : Re e)      (summed over kz)
//   ckz[kz]   += wgt e                                             (summed over kx)
// so that <a'(x + r_x, y, z) b'(x, y_r, z)> = Re sum_k ckx[k] exp(i k ax r_x), and likewise in z with ckz.
// The kYSpecRows real rows are (Re, Im) of the four complex rows of the row set:
//   kYCrossVelocity  u u*, v v*, w w*, u v*
//   kYCrossShear     u omega_z*, v omega_z*, w omega_x*, omega_z omega_z*      (a at y, b at y_r)
// A reference plane is read from the same kx sub-block as the planes it is paired with.
constexpr int kYCrossMaxRefs = 16;
enum { kYCrossVelocity = 0, kYCrossShear = 1 };
struct YCrossArgs : SpecWalkArgs {    // u, v, w; the shear set also omega_x and omega_z
  int nkz = 0;                        // global retained kz count
  int rows = kYCrossVelocity;
  int nref = 0;
  int yref[kYCrossMaxRefs] = {};      // distinct planes in [0, N)
  double* ckx = nullptr;              // [nref][kYSpecRows][N][Kx + 1]
  double* ckz = nullptr;              // [nref][kYSpecRows][N][nkz]
};
void ycross_accumulate(const YCrossArgs& a, bool fp64, hipStream_t s);
// Regridding of spectral lines onto the solver's grid (regrid.hpp has the tables; kernels/regrid.hip): the
// lines of `nkx` consecutive kx of one kx sub-block are read from a line-major fp64 staging buffer
// [slot][scols][NY_s] (complex; each line contiguous in y), interpolated along y and written
// line-fastest into the block's spectral field.  A workgroup takes one kx, 8 kz lines and one chunk of
// kRegridChunk target planes: it stages the chunk's source window of its lines in LDS, then every lane
// forms one output, value = (sum_m w[y][m] f[j0[y] + m]) / n2 (the unit rows copy f[j0[y] + unit[y]]),
// rounded once to the storage type.  Local kz lines [ncol, nkzs) are written as zeros; a kx whose slot is
// negative is left untouched (the caller zeroes the field first).  Destination addressing is spec_index
// with the geometry of the sub-block.  U (optional): plane y of line (u_ikx, kz 0) becomes (U[y], 0).
constexpr int kRegridLdsBytes = 64 * 1024;  // the kernel's dynamic LDS budget: 8 lines of (max window | 1) rows
struct RegridArgs {
  const double* src = nullptr;        // staging buffer
  const int* slot = nullptr;          // [nkx] slot of kx ikx0 + i of the sub-block, or -1
  int nkx = 0, ikx0 = 0;              // kx of this launch, the first one's index in the sub-block
  int scols = 0, ncol = 0;            // lines per slot; local kz lines with a source (<= scols)
  int NY_s = 0, NY_d = 0, W = 0;
  const int* j0 = nullptr;            // [NY_d]
  const int* unit = nullptr;          // [NY_d]
  const double* w = nullptr;          // [NY_d][W]
  const int* win = nullptr;           // [chunks][2]: win0, winlen
  int max_window = 0;                 // the largest winlen (sizes the LDS)
  double n2 = 1.0;                    // the source's units (divisor)
  void* dst = nullptr;                // the sub-block's field
  int nkx_blk = 0, nkzs = 0, kzb = 0;  // spec_index geometry of the sub-block
  const double* U = nullptr;          // [NY_d] mean profile for line (u_ikx, 0), or null
  int u_ikx = -1;
  int lds_poison = 0;                 // debug: fill the LDS with NaN before use
};
void regrid_launch(const RegridArgs& a, bool fp64, hipStream_t s);
// element (local kx 0, kz 0) of every plane y < N of one spectral field (lines = nkx_loc * nkzs) := 0
void zero_mean_line(void* q, int N, int kzb, int lines, bool fp64, hipStream_t s);
// fault injection (tests): element `elem` of a complex field becomes NaN
void inject_nan(void* field, size_t elem, bool fp64, hipStream_t s);

}  // namespace channel
