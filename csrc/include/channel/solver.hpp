// The channel-flow DNS solver: one instance per rank (one process per GPU).
//
// Formulation (reference README.md:4-6): Kim-Moin-Moser phi = lap(v) / omega_y,
// Fourier x,z with 2/3 dealiasing, compact FD in y, SMR low-storage RK3 with implicit viscous
// terms, constant flow rate, mean profile U(y) evolved on the rank that owns kx=0.
//
// Per RK3 substep (all device-resident, captured into one hipGraph per RK3 step):
//   K-SPEC (y-lines) -> [all-to-all per field, comm stream] -> x C2C inverse (per field)
//   -> z physical stage (C2R, u x omega, R2C, CFL maxima) -> x C2C forward (per field)
//   -> [all-to-all per field] -> next K-SPEC.
// The reference's equivalent is RKstep (RK3.c:111-193) with host-staged transposes.
#pragma once

#include <hip/hip_runtime.h>

#include <complex>
#include <exception>
#include <functional>
#include <memory>
#include <thread>
#include <chrono>
#include <string>
#include <vector>

#include "channel/comm.hpp"
#include "channel/config.hpp"
#include "channel/grid.hpp"
#include "channel/kernels.hpp"
#include "channel/plan.hpp"

namespace channel {

// SMR low-storage RK3 coefficients (RK3_kernels.cu:24-25, 113; RK3.c:14; meanUevol.c:35-38)
struct RK3Coef {
  static constexpr double gamma[3] = {8.0 / 15.0, 5.0 / 12.0, 3.0 / 4.0};
  static constexpr double zeta[3] = {0.0, -17.0 / 60.0, -5.0 / 12.0};
  static constexpr double alpha[3] = {29.0 / 96.0, -3.0 / 40.0, 1.0 / 6.0};
  static constexpr double beta[3] = {37.0 / 160.0, 5.0 / 24.0, 1.0 / 6.0};
};

struct StepLog {
  long step = 0;
  double time = 0, dt = 0, dt_c = 0, dt_v = 0;
  double umax = 0, vmax = 0, wmax = 0, cflsum = 0;
  double dUdy_lo = 0, dUdy_hi = 0, flux = 0, dpdx = 0;
  double utau_lo = 0, utau_hi = 0, utau = 0;
  unsigned health = 0;
};

class Solver {
 public:
  // nccl_uid: empty for P == 1
  Solver(const Config& cfg, int rank, int nranks, int device, const std::string& nccl_uid = std::string());
  ~Solver();
  Solver(const Solver&) = delete;
  Solver& operator=(const Solver&) = delete;

  const Config& config() const { return cfg_; }
  const Plan& plan() const { return plan_; }
  const YGrid& grid() const { return grid_; }
  hipStream_t stream() const { return s_comp_; }
  bool fp64() const { return fp64_; }

  // ---- state --------------------------------------------------------------------------
  // local spectral state, [y][kx_local][kz] true Fourier coefficients; U: NY (used on the owner)
  void set_state(const std::complex<double>* phi, const std::complex<double>* omega, const double* U);
  void get_state(std::complex<double>* phi, std::complex<double>* omega, double* U) const;
  void init_ic();      // config ic: random | laminar | zero (deterministic, independent of P)
  // ---- passive scalar (cfg.scalar; one rank without a communicator) ----------------------------
  // theta-hat in the canonical [y][kx][kz] layout of the state; its mean line (kx, kz) = (0, 0) holds the
  // real mean profile Theta(y) itself.  set_scalar clears R_theta.
  bool scalar_on() const { return sc_ != nullptr; }
  void set_scalar(const std::complex<double>* th);
  void get_scalar(std::complex<double>* th) const;
  void init_scalar_ic();  // config scalar_ic: laminar | zero
  // the flux pass alone on the current state: (u theta)^, (v theta)^, (w theta)^, canonical [3][y][kx][kz]
  std::vector<std::complex<double>> scalar_flux_hat();
  // [5][NY]: Theta, <theta'theta'>, <u'theta'>, <v theta'>, <w theta'> (Parseval plane sums of the retained
  // modes with the weights and the mean-line skip of stats(); products and sums in double)
  std::vector<double> scalar_sums();
  // device time in ms of one substep's scalar work: [x-backward, zscalar, x-forward, scalar_kernel]
  // (events on the compute stream; tools/scalar_cost.py).  The state is left as it was.
  std::vector<double> scalar_timing();
  void prepare();      // fill the transform inputs from the state (K-SPEC mode 0)

  // ---- time stepping ---------------------------------------------------------------------
  void step(bool stats_for_next = false);  // one RK3 step
  void run(long nsteps, bool verbose = true);  // reference-style driver loop with logging/stats
  void synchronize();
  StepLog log();                     // reads device diagnostics (host sync)
  std::vector<double> stats();       // [4][NY] plane sums of the last stats step (global)
  std::vector<double> mean_profile();  // U(y) (owner rank; zeros elsewhere)
  unsigned health();                  // global OR of health flags
  double time() const;
  long steps_done() const { return nstep_; }
  void set_time(double t, double dt);
  void set_use_graph(bool on) { use_graph_ = on; }
  // true when the RK3 step is replayed from a captured hipGraph (after the first captured step)
  bool graph_active() const;
  // the communicator's kind ("rccl" | "shm") or "none" for the single-rank fast path
  std::string comm_kind() const;
  // per-phase timing: hipEvents around every stage on its own stream (no host sync inside the
  // step; the pairs are resolved once per step).  Runs eagerly and, at P = 1, on one stream so the
  // stages are serialised and the phase times add up to the step time.
  void set_phase_timing(bool on);
  // accumulated per-phase times [kspec, x_backward, z_physical, x_forward, a2a, reduce, io, other]
  std::vector<double> phase_times_ms();
  void reset_phase_times();
  // per-step device times: hipEvents recorded on the compute stream around every step() (graph
  // launches included); step_times_ms() synchronises and returns (and clears) them
  void set_step_timing(bool on) { step_timing_ = on; }
  std::vector<double> step_times_ms();
  // K-SPEC per-phase shader-clock sums over all waves (only with CHANNEL_KSPEC_PROF set)
  std::vector<double> kspec_profile();
  void symmetrize();                  // kz=0 Hermitian symmetry (any P; one column exchange)

  // ---- failure handling -------------------------------------------------------
  void take_snapshot();               // device copy of (phi, omega+U, dt, time, step)
  void rollback();                    // restore it; cfl *= rollback_cfl_factor; re-capture graphs
  long snapshot_step() const { return snap_step_; }
  int rollbacks() const { return rollbacks_; }
  double cfl() const { return cfg_.cfl; }
  void inject_nan(int field = PHI);   // fault injection (tests)

  // ---- diagnostics ---------------------------------------------------------------------------
  // energy spectra of u,v,w of the current state at cfg.spectra_planes (global sums):
  // ekx [3][np][Kx+1], ekz [3][np][nkz], map [3][nkx][nkz] at the first plane
  struct Spectra {
    std::vector<int> planes;
    std::vector<double> ekx, ekz, map;
  };
  Spectra spectra();
  // Physical-space export of the current state (one rank without a communicator; not part of the
  // step, which keeps no physical field in memory): x-backward of the K-SPEC outputs chunk by chunk
  // into the step's scratch, then the z complex-to-real export stage (kernels.hpp zreal).
  // physical_fields: planes `planes` (any order) of the fields `names` (u v w wx wy wz), data
  // [name][plane][NX][Nzp]
  struct PhysFields {
    std::vector<int> planes;
    std::vector<std::string> names;
    std::vector<double> data;
    int NX = 0, Nzp = 0;
  };
  PhysFields physical_fields(const std::vector<int>& planes, const std::vector<std::string>& names);
  // plane means of u', u'^2, v'^2, w'^2, u'v', u'^3, v'^3, w'^3, u'^4, v'^4, w'^4 (u' = u - U(y)):
  // [kMomRows][NY], every plane
  std::vector<double> plane_moments();
  // Velocity-gradient plane sums of the current state, [kGradRows][NY] (kernels.hpp GradSumArgs:
  // |omega_x|^2, |omega_y|^2, |omega_z|^2, g_uu, g_vv, g_ww, g_uv; raw sums, no nu and no factor 2),
  // global (any communicator; all-reduced like spectra())
  std::vector<double> gradient_sums();
  // plane means of u'u'v, wwv, u'vv, [kTripleRows][NY] (one rank without a communicator, through the
  // export stage like plane_moments)
  std::vector<double> transport_moments();
  // Histograms of u, v, w (vorticity: and omega_x, omega_y, omega_z) at the planes `planes` (distinct),
  // the joint histogram of (u, v) and the quadrant split of u'v (kernels.hpp ZRealArgs::hist has the
  // binning rule): one rank without a communicator, through the export stage like plane_moments.
  // centre, halfwidth: [nhf][np] as the planes are listed; empty: centre = U(y) for u, -D1 U for
  // omega_z and 0 otherwise, halfwidth = span * the plane r.m.s. of the current state about that centre
  // (plane_moments() for u, v, w, rows 0..2 of gradient_sums() for the vorticity, rounded to 12 significant
  // bits so that two calls on one state bin alike; 1 where it is 0).
  struct PlaneHistograms {
    std::vector<int> planes;
    std::vector<std::string> names;
    int nb = 0, nj = 0;
    std::vector<unsigned long long> hist;   // [nhf][np][nb + 2]: underflow, nb bins, overflow
    std::vector<unsigned long long> joint;  // [np][nj + 2][nj + 2], (u bin, v bin)
    std::vector<double> quad;               // [kQuadRows][np]: plane means of u'v over Q1..Q4, then the quadrants' sample fractions
    std::vector<double> centre, halfwidth;  // [nhf][np], as used
  };
  PlaneHistograms plane_histograms(const std::vector<int>& planes, int nbins = 128, int njoint = 64, double span = 8.0,
                                   bool vorticity = false, const std::vector<double>& centre = {},
                                   const std::vector<double>& halfwidth = {});
  // Pressure of the current state (one rank without a communicator; kernels.hpp PressureArgs):
  // Pi = p + |u|^2 / 2 per (kx, kz) line in the canonical [y][kx][kz] layout, zero on the mean line.
  // The step's transform stage runs once more into a buffer of its own (d_pres_), so neither the
  // state nor K-SPEC's outputs are written and the next step is unchanged bitwise.
  std::vector<std::complex<double>> pressure_hat();
  // plane means <p'p'>, <p'u'>, <p'v>, <p'w> of the fluctuating static pressure p' (central moments),
  // [4][NY], through the export stage (kernels.hpp ZRealArgs::pres)
  std::vector<double> pressure_moments();
  // device time in ms of one pressure solve without the host copy of pressure_hat: [the transform
  // stage, the y-line Poisson kernel] (events on the compute stream; tools/export_cost.py)
  std::vector<double> pressure_timing();
  // The fluctuating static pressure p' of the current state in spectral space, truncated to the retained
  // modes: canonical [y][kx][kz], zero on the mean line (one rank without a communicator).  The
  // pressure-mode export pass over every plane with the return trip of r = p' + <r> to spectral space
  // (kernels.hpp ZRealArgs::spec_out) into field 1 of d_pres_; nothing the next step reads is written.
  std::vector<std::complex<double>> static_pressure_hat();
  // Parseval plane sums of p-hat' with the strain factors, [kPStrainRows][NY] (kernels.hpp PStrainArgs:
  // the pressure-strain terms of the uu, vv, ww, uv budgets, <p'u'>, <p'v> and the retained-band part
  // of <p'p'>); one rank without a communicator
  std::vector<double> pressure_strain();
  // One-dimensional spectra and co-spectra of the current state at every plane (kernels.hpp
  // YSpectraArgs): ekx [kYSpecRows][NY][Kx+1] by |kx| (summed over kz), ekz [kYSpecRows][NY][nkz] by
  // kz (summed over kx); rows uu, vv, ww, uv, wxwx, wywy, wzwz, pp.  Global (any communicator;
  // all-reduced like gradient_sums()).  pressure: also row pp, from static_pressure_hat()'s device part
  // (one rank without a communicator); otherwise that row is zero.
  struct PlaneSpectra {
    std::vector<std::string> rows;
    std::vector<double> ekx, ekz;
  };
  PlaneSpectra plane_spectra(bool pressure = false, double* ms = nullptr);  // ms: the device time of the launches
  // Cross-spectra of every plane against the reference planes refs (distinct, in [0, NY), at most
  // kYCrossMaxRefs; kernels.hpp YCrossArgs): ckx [4][nref][NY][Kx+1] by |kx| and ckz [4][nref][NY][nkz] by
  // kz, complex, of the row set "velocity" (uu, vv, ww, uv) or "shear" (u_wz, v_wz, w_wx, wz_wz), the first
  // factor at y and the conjugated second at the reference plane.  Global (any communicator; all-reduced
  // like plane_spectra()).  ms: the device time of the launches.
  struct PlaneCrossSpectra {
    std::vector<std::string> rows;
    std::vector<int> ref_planes;
    // (Re, Im) pairs, 2 * 4 * nref * NY * nk doubles each; not value-initialised: at 16 planes and the
    // headline grid the result is 270 MB, and its first touch is spread over the threads that fill it
    std::unique_ptr<double[]> ckx, ckz;
    size_t nkx = 0, nkz = 0;             // bins per (row, reference plane, plane): Kx + 1, nkz
    const std::complex<double>* kx() const { return reinterpret_cast<const std::complex<double>*>(ckx.get()); }
    const std::complex<double>* kz() const { return reinterpret_cast<const std::complex<double>*>(ckz.get()); }
  };
  PlaneCrossSpectra plane_cross_spectra(const std::vector<int>& refs, const std::string& rows = "velocity", double* ms = nullptr);
  // device time in ms of the launches of one plane_cross_spectra() and of one plane_spectra() (tools/export_cost.py)
  std::vector<double> plane_cross_spectra_timing(const std::vector<int>& refs, const std::string& rows = "velocity");
  // Spectral Reynolds-stress budgets of the current state at every plane (kernels.hpp SBudgetArgs): ekx
  // [kSBudRows][NY][Kx+1] by |kx| and ekz [kSBudRows][NY][nkz] by kz, with the conventions of
  // plane_spectra(); U and dU are the mean profile and its compact first derivative as the rows used
  // them.  One rank without a communicator (it runs the pressure solve and the static pressure).
  struct SpectralBudgets {
    std::vector<std::string> rows;
    std::vector<double> ekx, ekz, U, dU;
  };
  SpectralBudgets spectral_budgets(double* ms = nullptr);
  // device time in ms of the launches of its two stages (events on the compute stream; tools/export_cost.py)
  std::vector<double> spectral_budgets_timing();
  // H = (u x omega)^ of the current state as the transform stage leaves it before the pressure solve:
  // canonical [3][y][kx][kz] (one rank without a communicator)
  std::vector<std::complex<double>> rotational_hat();

  // ---- restart files (reference-compatible, Appendix B) --------------------------------
  // t: the restart file of theta (layout, units and attributes of G), "-" = none
  void write_restart(const std::string& g, const std::string& ddv, const std::string& umean, const std::string& t = "-");
  void read_restart(const std::string& g, const std::string& ddv, const std::string& umean, const std::string& t = "-");
  // ---- restart onto another grid (regrid.cpp; regrid.hpp has the semantics) ---------------
  // Files on any grid of the same box: modes map by index (truncated or zero-padded), every line is
  // interpolated along y on the device, U(y) with the same table on the host.  read_restart calls it
  // when cfg.regrid is set.  src_stretch: the files' tanh stretching (0: their "stretch" attribute,
  // else the config's).  time and step are restored; dt only when the grid is unchanged.
  void read_restart_regrid(const std::string& g, const std::string& ddv, const std::string& umean, double src_stretch = 0.0);
  // The same from a global source state in memory, in the canonical one-rank get_state layout
  // [NY_s][nkx_s][nkz_s] (true Fourier coefficients); every rank picks its own lines.  The clock is
  // left as it is.
  void regrid_state(const std::complex<double>* phi_s, const std::complex<double>* om_s, const double* U_s, int NX_s, int NY_s,
                    int NZ_s, double stretch_s);
  // host and device times in ms of the last regrid: [source read / reorder, upload, kernel, total]
  std::vector<double> regrid_timing() const { return regrid_ms_; }
  // capture the state now (host copy) and write the files from a background thread; the next
  // checkpoint / wait_checkpoint() / run() end / destructor joins it (and rethrows its error)
  void checkpoint_async(const std::string& g, const std::string& ddv, const std::string& umean, const std::string& t = "-");
  void wait_checkpoint();

  // ---- raw device access (tests / bindings) ----------------------------------------------
  enum Field { PHI = 0, OMEGA, RPHI, ROMEGA, OUT0, OUT1, OUT2, OUT3, OUT4, OUT5 };
  void* field_ptr(int f) const;
  // backward-exchanged field j: the combine mode's inputs (0 D1 v, 1 v, 2 D1 omega, 3 omega, 4 phi)
  // or the six physical-stage fields (choose_layout)
  static constexpr int kCmbIn = 5;
  int bwd_fields() const { return combine_ ? kCmbIn : 6; }
  bool combine() const { return combine_; }
  void* in_field(int j) const;
  void* phys_ptr() const { return phys_; }
  // row pitch of the x-expanded buffer in elements (0: rows of nkz_loc) and the elements per field
  int xexp_row_pitch() const { return xpitch_; }
  size_t phys_field_elems() const { return physn_; }
  const YTablesDev& ytables() const { return ytab_; }
  // kx sub-blocks of the local spectral layout (1 = plain [y][kx_local][kz]; see nkb_)
  int kblocks() const { return nkb_; }
  // backward-exchange kx sub-block groups issued so far (host count: the pipeline bookkeeping of
  // the pre-send, checked by the capture-failure test)
  long long bwd_blocks_issued() const { return bwd_blocks_issued_; }
  // compute streams of the last P > 1 transform stage recorded inside a stream capture (0: none yet)
  int captured_compute_streams() const { return captured_streams_; }
  int spec_kzb() const { return kzb_; }  // spectral layout (spec_index)
  // abort every communicator (the per-axis split ones first: aborting the parent does not abort
  // communicators split from it), so no stream stays blocked in an exchange with a dead peer
  void abort_comms();
  void substep_debug(int n);            // one substep, eager (tests)
  void transforms_debug(bool dt_update);  // backward + phys + forward only (tests)
  Comm* comm() { return comm_.get(); }
  void barrier();
  // host value reduced (max) over all ranks through the solver's communicator (timing, control)
  double max_over_ranks(double v);

 private:
  void choose_layout();
  void alloc();
  void free_all();
  // dst (one rank without a communicator): where the x-forward writes H_x, H_y, H_z (default out_)
  void transforms(int substep, bool stats, void* dst = nullptr);
  void kspec(int mode, int substep, bool stats);
  void a2a_spec(const void* spec, void* xb, bool to_phys);
  void a2a_rows(void* xexp, void* zrows, bool to_z);
  void step_body(bool stats);
  void ev(int phase, bool end, hipStream_t s = nullptr);
  void flush_phase_events();
  hipEvent_t timing_event();
  // P > 1 slab: y-chunked backward exchange -> x -> z -> x -> forward exchange pipeline
  void transforms_slab(int n, const XArgs& xa, const ZArgs& za, const DtArgs& da);
  // exchange of y chunk k (rows [k*ch, (k+1)*ch) of every rank's y range) for nf fields over the
  // column group (the world for the slab)
  void a2a_slab_chunk(int k, int ch, bool to_phys, int nf);
  // the same for rows [r0, r0 + nr) of every rank's y range and kx sub-blocks [blo, bhi) only
  void a2a_slab_rows(int r0, int nr, bool to_phys, int nf, int blo, int bhi);
  // pencil: the same y-chunked pipeline with the B exchange (row group, x <-> kz) between the x
  // transforms and the z stage
  void transforms_pencil(int n, const XArgs& xa, const ZArgs& za, const DtArgs& da);
  void b2b_pencil_chunk(int k, int ch, bool to_z, int nf);
  Comm* col_comm() const { return comm_col_ ? comm_col_.get() : comm_.get(); }
  bool comm_failed();
  void write_logs(const StepLog& L, bool verbose);
  void write_stats_files(const std::vector<double>& st);
  void write_spectra_files(const Spectra& sp);
  void write_field_files();
  void write_moment_files(const std::vector<double>& m);
  void write_budget_files();
  void write_pressure_files();
  // Pi of the current state into field 0 of d_pres_ (device part of pressure_hat): H into the three
  // fields of d_pres_ (rotational_device), then the y-line Poisson solve over H_x (poisson_device)
  void pressure_device(double* ms = nullptr);
  void rotational_device();
  void poisson_device();
  void write_pstrain_files();
  void write_pdf_files();
  void write_yspectra_files();
  void write_sbudget_files();
  void write_ycross_files();
  void write_scalar_files();
  // passive scalar: the flux pass of the stage state into the flux fields (before transforms(), which
  // overwrites u, v, w with H) and the y-line advance of substep n (after K-SPEC; reads d_dt_).
  // ms (eager, timing): += the device times of the x-backward, zscalar and x-forward launches
  void scalar_flux_device(double* ms = nullptr);
  void scalar_advance_device(int n);
  void read_scalar_file(const std::string& path);  // theta from a restart file on this grid
  void* scalar_ptr(int f) const { return static_cast<char*>(sc_) + static_cast<size_t>(f) * spec_ * esz_; }
  // p-hat' of the current state into field 1 of d_pres_ (device part of static_pressure_hat): the
  // pressure solve, then the return trip of r through physical space (static_return_device)
  void static_pressure_device();
  void static_return_device();
  // one device spectral field as canonical [y][kx][kz]; refuses non-zero padding of the device layout
  std::vector<std::complex<double>> spec_to_canonical(const void* d_field, const char* what);
  // x-backward arguments of the whole local slab (transforms and the export): the common part, the
  // one-rank source (sets the blocked layout in xa) and the arguments of planes [y0, y0 + ny)
  XArgs x_args() const;
  XSrc x_src_local(XArgs& xa) const;
  void x_chunk(const XArgs& xa, const XSrc& src, int y0, int ny, XArgs& xc, XSrc& sc) const;
  // export driver: the sorted distinct planes ys in contiguous runs of at most a step chunk; fields
  // 0 .. nf-1 are transformed, those of out_mask handed to sink(y0, ny, host [slot][ny][NX][Nzp]
  // in the storage precision), the moments accumulated into d_mom (either may be absent)
  void export_planes(const std::vector<int>& ys, int nf, unsigned out_mask, double* d_mom,
                     const std::function<void(int, int, const void*)>& sink, double* d_triple = nullptr,
                     bool pres = false, double* d_pmom = nullptr, const ZRealArgs* hist = nullptr);
  // what the diagnostics share (diagnostics.cpp): the arguments of the all-plane spectral reductions
  // for the whole local slab (the fields of the mask `six`, p-hat' on request); fn(byte offset, kx count,
  // global kx start) per kx sub-block; the all-reduce (any communicator) and host copy of n accumulated
  // doubles; the list of all planes; the pressure-mode x-backward of Pi into slot 3 of the scratch and
  // the common z export arguments of a chunk; the export passes of a field selection, plane by plane
  void walk_args(SpecWalkArgs& a, unsigned six, bool pres) const;
  template <typename F>
  void for_kblocks(F&& fn) const;
  void reduce_fetch(double* d, size_t n, double* h);
  std::vector<int> all_planes() const;
  // field: the one spectral field transformed (default: Pi, field 0 of d_pres_); its mean line is kept
  XArgs pi_backward(const XArgs& xc, const XSrc& sc, const void* field = nullptr);
  ZRealArgs zreal_args(int y0, int ny, int nf) const;
  template <typename Put>
  void export_fields(const std::vector<int>& planes, const std::vector<int>& fidx, Put&& put);
  void write_json(const StepLog& L, double ms_per_step);
  void wait(hipStream_t s);           // stream sync with the communicator watchdog (P > 1)
  void invalidate_graphs();
  struct RestartJob {
    std::string g, ddv, umean, t;
    std::vector<std::complex<double>> phi, om, th;
    std::vector<double> U;
    double time = 0, dt = 0;
    long step = 0;
    long serial = 0;
  };
  RestartJob capture_restart(const std::string& g, const std::string& ddv, const std::string& umean, const std::string& t);
  // turn(t) is called before every rank-ordered write step t (t % P = the writing rank)
  void write_restart_job(const RestartJob& j, const std::function<void(int)>& turn);
  // a regrid source: its grid and units, and fill(field 0 phi | 1 omega, local target kx of a batch,
  // host) staging the batch's source planes, each plane_lines lines [kz][y] of (re, im) doubles of
  // which lines [line0, line0 + local kz with a source) are uploaded
  struct RegridSource {
    int NX = 0, NY = 0, NZ = 0;
    double stretch = 2.0, n2 = 1.0;
    size_t plane_lines = 0;
    int line0 = 0;
    std::function<void(int, const std::vector<int>&, std::vector<double>&)> fill;
    std::vector<double> U;  // [NY] mean profile on the target grid (true units)
  };
  void regrid_apply(const RegridSource& src);
  std::vector<double> regrid_ms_;

  Config cfg_;
  Plan plan_;
  YGrid grid_;
  bool fp64_ = false;
  int device_ = 0;
  size_t esz_ = 8;  // bytes per complex element
  hipStream_t s_comp_ = nullptr, s_comm_ = nullptr;
  std::unique_ptr<Comm> comm_;
  // pencil exchange groups (one communicator per decomposition axis): column group
  // (same process row, Pc ranks: A exchange kx <-> y) and row group (same column, Pr ranks: B)
  std::unique_ptr<Comm> comm_col_, comm_row_;
  YTablesDev ytab_;
  Twiddles tw_x_, tw_z_;

  void* state_ = nullptr;  // phi, omega, Rphi, Romega (4 * spec)
  void* out_ = nullptr;    // 6 * spec
  void* phys_ = nullptr;   // 6 * phys
  void* sc_ = nullptr;     // passive scalar (cfg.scalar): theta, R_theta, F_x, F_y, F_z (5 * spec)
  double* d_ssum_ = nullptr;  // scalar sums: [kScalarSumRows][NY]
  void* xbuf_ = nullptr;   // P>1: 6 * ny_loc*nkx*nkz_loc (A-exchange blocks)
  hipEvent_t ev_dtf_[2] = {nullptr, nullptr};  // P = 1 one-chunk path: dt update forked beside the x-forward
  unsigned* d_rowtab_ = nullptr;  // slab P > 1: per retained kx row, its exchange segment's offset / stride (XSrc::rowtab)
  void build_rowtab();
  void* zbuf_ = nullptr;   // pencil: 6 * ny_loc*nx_loc*nkz (B-exchange blocks, z stage in place)
  size_t spec_ = 0, physn_ = 0, xstride_ = 0, zstride_ = 0;
  int xpitch_ = 0;         // x-expanded row pitch (one rank: xexp_pitch(nkz); 0: rows of nkz_loc)
  // spectral layout (spec_index): kzb_ = 8 (one rank) blocks the lines by 8 kz, with the kz line
  // stride nkzs_ padded to a multiple of 8; canon_ = NY * nkx_loc * nkz_loc, the element count of
  // the canonical host layout [y][kx_loc][kz_loc] (set_state / get_state / restart files)
  int kzb_ = 0, nkzs_ = 0;
  bool combine_ = false;  // K-SPEC's combine-mode outputs + the combining x-backward (choose_layout)
  size_t canon_ = 0;

  // device scalars / diagnostics (one allocation)
  void* dscal_ = nullptr;
  double* d_dt_ = nullptr;
  double* d_time_ = nullptr;
  double* d_dtlog_ = nullptr;
  float* d_max_ = nullptr;
  double* d_stats_ = nullptr;
  // K-SPEC's per-workgroup partial plane sums [stats_blocks_][stats_stride_] (SpecArgs::stats_part):
  // one row per workgroup of the largest K-SPEC grid, reduced into d_stats_ after the statistics
  // substep's last launch
  double* d_stats_part_ = nullptr;
  int stats_blocks_ = 0, stats_stride_ = 0;
  double* d_mean_ = nullptr;
  unsigned* d_health_ = nullptr;
  unsigned long long* d_kprof_ = nullptr;
  bool kprof_on_ = false;
  int ystreams_ = 1;               // streams the y chunks alternate over (P = 1)
  std::vector<hipStream_t> s_extra_;   // streams beyond compute + comm for the chunk pipeline
  // P > 1 slab, CHANNEL_PSTREAMS=2: a second compute stream; the y chunks' transforms alternate
  // between s_comp_ and it (the comm stream carries the exchanges), as the P = 1 chunks do
  hipStream_t s_comp2_ = nullptr;
  hipEvent_t ev_comp2_ = nullptr;
  int pstreams_ = 1;  // compute streams of the P > 1 chunk pipeline (CHANNEL_PSTREAMS)
  std::vector<hipEvent_t> ev_join_;
  int ychunk_ = 0;                 // y planes per x->z->x pipeline chunk (P = 1), 0 = whole slab
  double* d_invdy_ = nullptr;
  double* d_red_ = nullptr;  // one double for max_over_ranks
  double* d_y_ = nullptr;    // y grid (analytic influence functions)

  std::vector<hipEvent_t> ev_a2a_, ev_xf_, ev_b_, ev_bb_;
  hipEvent_t ev_spec_ = nullptr, ev_phys_ = nullptr, ev_fwd_done_ = nullptr, ev_red_ = nullptr, ev_stats_ = nullptr;
  std::vector<hipEvent_t> ev_cb_, ev_cc_, ev_cc2_;  // per y-chunk: backward exchange done, compute done (part 0 / part 1)
  // pencil pipeline, per y chunk: A in, x-backward, B in, z stage, B out, x-forward done
  std::vector<hipEvent_t> ev_pen_[6];
  int ychunk_p_ = 0;                       // y planes per chunk of the P > 1 slab pipeline
  bool self_direct_ = true;                // slab: own kx block read/written in place (no self copy)
  // K-SPEC / exchange overlap (P > 1 slab, and a 1-rank communicator): the local spectral fields
  // are stored as nkb_ kx sub-blocks, each [y][kx in block][kz] (block b at element kb_off_[b] of
  // every field).  K-SPEC runs block by block and the backward exchange of block b goes out on the
  // comm stream while block b+1 is solved.  Every rank splits its
  // kx range the same way (balanced), so block (c, b) of rank c is one exchange segment of the x
  // transforms (Pc * nkb_ <= 8 segments).
  int nkb_ = 1;
  std::vector<int> kb_start_, kb_cnt_;     // local ikx start / count of block b (this rank)
  std::vector<size_t> kb_off_;             // element offset of block b in a spectral field
  std::vector<hipEvent_t> ev_kb_;          // K-SPEC block b done (compute stream)
  // Substep 0 of a step consumes a pre-send: the backward exchange of blocks 0 .. nkb_-2 of the
  // state's outputs goes out at the end of the previous step (behind the last K-SPEC's blocks,
  // inside its graph) or, after anything that recomputed the outputs (prepare()), eagerly before
  // the step.  presend_done_: that exchange has been issued for the next substep 0.
  bool presend_done_ = false;
  bool presend_saved_ = false;  // presend_done_ before a step capture (restored if the graph is dropped)
  long long bwd_blocks_issued_ = 0;
  int captured_streams_ = 0;
  int xnt_ = 0;  // non-temporal spectral accesses in the x transforms (XArgs::nt)
  bool kb_overlap() const { return nkb_ > 1 && comm_ != nullptr; }
  // Forward-path overlap (slab, kx sub-blocks): the last y chunk's forward exchange goes out block
  // by block (ev_fb_[b] on the comm stream) and K-SPEC block b waits only for block b's rows.
  // fwd_pending_: the next kspec() (or join_forward()) must consume those events.
  std::vector<hipEvent_t> ev_fb_;
  hipEvent_t ev_cfl_ = nullptr;
  bool fwd_split_ = true, fwd_pending_ = false;
  void join_forward();
  void presend_backward(bool wait_blocks);
  int kb_gstart(int c, int b) const;       // global retained-kx start of block b of column rank c
  int kb_gcount(int c, int b) const;
  size_t kb_index(int y, int ikx, int kz) const;  // blocked element index of (y, local kx, kz)
  size_t dev_index(int y, int ikx, int kz) const;  // device element index of (y, local kx, local kz)
  // phase timing: event pool and the (phase, start, end) pairs of the current step
  struct TPair {
    int phase;
    hipEvent_t a, b;
  };
  std::vector<hipEvent_t> tev_pool_;
  size_t tev_used_ = 0;
  std::vector<TPair> tpairs_;
  hipEvent_t topen_[8] = {};
  std::vector<double> ph_ms_;
  bool phase_timing_ = false;
  bool step_timing_ = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> step_ev_;
  size_t step_ev_used_ = 0;
  bool comm_warm_ = false;
  std::thread ckpt_thread_;
  std::exception_ptr ckpt_error_;
  long ckpt_serial_ = 0;
  unsigned long long run_nonce_ = 0;  // same on every rank of one run (from the communicator id): checkpoint markers
  // t_end checks without a per-step host sync: (dt, time) of the last two steps in pinned memory
  double* h_tdt_ = nullptr;
  hipEvent_t ev_tdt_[2] = {nullptr, nullptr};
  bool tdt_valid_ = false;
  bool t_end_reached();
  void wait_event(hipEvent_t e);      // event sync with the communicator watchdog (P > 1)

  // rollback snapshot
  void* snap_ = nullptr;
  long snap_step_ = -1;
  int rollbacks_ = 0;
  // spectra accumulators [ekx | ekz | map] and plane list (device)
  void* d_spec_ = nullptr;
  void* d_sym_ = nullptr;    // kz = 0 columns (local + gathered) for the distributed symmetrisation
  size_t spec_n_ = 0;
  void* d_real_ = nullptr;   // export: real planes of one chunk (lazily allocated)
  size_t real_n_ = 0;
  double* d_mom_ = nullptr;  // export: [kMomRows][NY], then [kTripleRows][NY]
  double* d_grad_ = nullptr;  // gradient sums: [kGradRows][NY]
  bool budget_note_ = false;  // the "triple files skipped" note has been printed
  void* d_pres_ = nullptr;    // pressure: three spectral fields (H, then Pi over H_x, p-hat' over H_y), lazily allocated
  double* d_pmom_ = nullptr;  // pressure: [kMomRows][NY] (dropped), then [kPresRows][NY]
  bool pres_note_ = false;    // the "pressure files skipped" note has been printed
  double* d_pstr_ = nullptr;  // pressure strain: [kPStrainRows][NY]
  bool pstr_note_ = false;    // the "pressure-strain files skipped" note has been printed
  void* d_hist_ = nullptr;    // histograms: hist, joint (64-bit counts), quad, then centre and scale [nhf][NY]
  size_t hist_n_ = 0;
  void* h_hist_ = nullptr;    // pinned host copy of the counts and the quadrant sums
  bool pdf_note_ = false;     // the "PDF files skipped" note has been printed
  double* d_yspec_ = nullptr;  // plane spectra: ekx [kYSpecRows][NY][Kx+1], then ekz [kYSpecRows][NY][nkz]
  double* h_yspec_ = nullptr;  // pinned host copy of d_yspec_ (the result is 17 MB at the headline grid)
  bool yspec_note_ = false;   // the "pressure row skipped" note has been printed
  double* d_sbud_ = nullptr;  // spectral budgets: ekx [kSBudRows][NY][Kx+1], ekz [kSBudRows][NY][nkz], then U and dU [NY]
  double* h_sbud_ = nullptr;  // pinned host copy of the sums of d_sbud_
  double* d_ycross_ = nullptr;  // cross-spectra: ckx [nref][kYSpecRows][NY][Kx+1], then ckz [nref][kYSpecRows][NY][nkz]
  double* h_ycross_ = nullptr;  // pinned host copy of d_ycross_
  size_t ycross_n_ = 0;         // doubles both hold (grown to the largest nref asked for)
  bool sbud_note_ = false;    // the "spectral budget files skipped" note has been printed
  double comm_timeout_s_ = 900.0;     // CHANNEL_COMM_TIMEOUT_S (0 = wait forever)

  bool use_graph_ = true;
  bool graph_ok_[2] = {false, false};
  // CHANNEL_MARKERS=1 (bench.py sets it at P > 1): one stderr line per rank after the eager warm-up
  // step, the capture and the first replay of each step graph, each after a (watchdog-polled)
  // synchronisation, so a first multi-GPU run that hangs shows which stage and rank stopped
  bool markers_ = false;
  bool capture_fail_test_ = false;
  bool replayed_[2] = {false, false};
  std::chrono::steady_clock::time_point t_created_ = std::chrono::steady_clock::now();
  void marker(const char* what);
  void end_failed_capture();
  hipGraphExec_t gexec_[2] = {nullptr, nullptr};
  bool prepared_ = false;
  long nstep_ = 0;
  bool stats_pending_ = false;
};

}  // namespace channel
