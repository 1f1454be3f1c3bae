// The diagnostics of the solver outside the step: spectra, the physical-space export and what is built
// on it (moments, pressure, pressure strain), the all-plane spectral reductions, and their files.
//
// Between steps out_ (and the state) hold K-SPEC's outputs of the current state and phys_ is scratch;
// everything here goes on the compute stream behind whatever is queued and writes nothing the next
// step reads, so the step graphs stay valid.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <string>
#include <thread>

#include "channel/common.hpp"
#include "channel/solver.hpp"

namespace channel {

namespace {
// the arguments of one kx sub-block: f[], p, nkx_loc and kx0 of a whole-slab SpecWalkArgs adjusted
template <typename A>
A at_block(A a, size_t off, int cnt, int kx0) {
  for (const void*& q : a.f)
    if (q) q = static_cast<const char*>(q) + off;
  if (a.p) a.p = static_cast<const char*>(a.p) + off;
  a.nkx_loc = cnt;
  a.kx0 = kx0;
  return a;
}

// Appends one line of n values to a file, as write_stats_files: scale * v, or sqrt(max(0, v)).
void append_profile(const std::string& file, const double* v, int n, double scale = 1.0, bool root = false) {
  std::ofstream f(file, std::ios::app);
  f.precision(8);
  for (int j = 0; j < n; ++j) f << " " << std::scientific << (root ? std::sqrt(std::max(0.0, v[j])) : scale * v[j]);
  f << " \n";
}

// a note printed once, by rank 0
void note_once(bool& done, int rank, const char* text) {
  if (!done && rank == 0) std::fputs(text, stderr);
  done = true;
}

std::vector<int> distinct_sorted(std::vector<int> ys) {
  std::sort(ys.begin(), ys.end());
  ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
  return ys;
}
// positions of each plane in a request
std::vector<std::vector<size_t>> plane_positions(const std::vector<int>& planes, int NY) {
  std::vector<std::vector<size_t>> pos(NY);
  for (size_t i = 0; i < planes.size(); ++i) pos[planes[i]].push_back(i);
  return pos;
}
// p' = r - <r>_plane, the mean formed in double
template <typename T>
void subtract_mean(T* q, size_t n) {
  double m = 0.0;
  for (size_t e = 0; e < n; ++e) m += q[e];
  m /= static_cast<double>(n);
  for (size_t e = 0; e < n; ++e) q[e] = static_cast<T>(q[e] - m);
}

// Header of a NumPy v1.0 file: magic, version, little-endian length, the dict padded with spaces to a
// multiple of 64 bytes in all and newline-terminated.  shape: "(a, b, c)".
std::string npy_header(const char* descr, const std::string& shape) {
  std::string dict = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shape + ", }";
  const size_t hlen = (10 + dict.size() + 1 + 63) / 64 * 64 - 10;
  dict.resize(hlen - 1, ' ');
  dict.push_back('\n');
  std::string h("\x93NUMPY\x01\x00", 8);
  h.push_back(static_cast<char>(hlen & 0xff));
  h.push_back(static_cast<char>(hlen >> 8));
  return h + dict;
}

// float64 rows per plane and wavenumber, (rows, ny, nk), as a NumPy file (YSPEC_*, SBUD_*)
void write_rows_npy(const std::string& fn, const std::vector<double>& v, int rows, int ny, int nk) {
  std::ofstream f(fn, std::ios::binary | std::ios::trunc);
  CH_CHECK(f.good(), "cannot open '" << fn << "'");
  const std::string h = npy_header("<f8", "(" + std::to_string(rows) + ", " + std::to_string(ny) + ", " + std::to_string(nk) + ")");
  f.write(h.data(), static_cast<std::streamsize>(h.size()));
  f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(double)));
  f.close();
  CH_CHECK(!f.fail(), "writing '" << fn << "' failed");
}

// The export passes of a field selection (phys_field_index values): one pass of the six physical-stage
// fields, or, with p, a pressure-mode pass (u, v, w and Pi, which takes field slot 3) that also serves
// u, v, w, and a plain pass for any of wx, wy, wz beside it.
struct ExportPass {
  unsigned mask = 0;
  int nf = 0;
  bool pres = false;
  // slot of field f (phys_field_index) among this pass's exported fields, -1 if another pass has it
  int slot(int f) const {
    const int bit = f == kPresField ? (pres ? 3 : -1) : ((pres && f >= 3) ? -1 : f);
    if (bit < 0 || !((mask >> bit) & 1u)) return -1;
    int sl = 0;
    for (int b = 0; b < bit; ++b) sl += (mask >> b) & 1u;
    return sl;
  }
};
std::vector<ExportPass> export_passes(const std::vector<int>& fidx) {
  bool pres = false;
  unsigned lo = 0, hi = 0;
  for (int f : fidx) {
    if (f == kPresField) pres = true;
    else if (f < 3) lo |= 1u << f;
    else hi |= 1u << f;
  }
  auto top = [](unsigned m) {
    int n = 0;
    for (int b = 0; b < 6; ++b)
      if ((m >> b) & 1u) n = b + 1;
    return n;
  };
  std::vector<ExportPass> out;
  if (pres) {
    out.push_back(ExportPass{lo | 8u, 4, true});
    if (hi) out.push_back(ExportPass{hi, top(hi), false});
  } else {
    out.push_back(ExportPass{lo | hi, top(lo | hi), false});
  }
  return out;
}
}  // namespace

// ---- shared pieces ---------------------------------------------------------------------------------
// The walk of the whole local slab: the six (combine mode: five) backward-exchanged fields, or of the six
// only those with their bit in `six` (the combine mode needs all five for any of them); p-hat' on request.
void Solver::walk_args(SpecWalkArgs& a, unsigned six, bool pres) const {
  const Plan& p = plan_;
  for (int f = 0; f < bwd_fields(); ++f)
    if (combine_ || ((six >> f) & 1u)) a.f[f] = in_field(f);
  if (pres) a.p = static_cast<const char*>(d_pres_) + spec_ * esz_;
  a.combine = combine_ ? 1 : 0;
  a.ax = p.ax;
  a.az = p.az;
  a.N = p.NY;
  a.nkx_loc = p.nkx_loc;
  a.kx0 = p.kx0;
  a.nkz_loc = p.nkz_loc;
  a.kz0 = p.kz0;
  a.nkzs = nkzs_;
  a.kzb = kzb_;
  a.nkx = p.nkx;
  a.Kx = p.Kx;
}

// fn(byte offset in a field, kx count, global kx start) per kx sub-block of the local spectral layout
template <typename F>
void Solver::for_kblocks(F&& fn) const {
  for (int b = 0; b < nkb_; ++b) fn(kb_off_[b] * esz_, kb_cnt_[b], plan_.kx0 + kb_start_[b]);
}

// n accumulated doubles at d: summed over the communicator, if there is one, and copied to h
void Solver::reduce_fetch(double* d, size_t n, double* h) {
  if (comm_) {
    HIP_CHECK(hipEventRecord(ev_stats_, s_comp_));
    HIP_CHECK(hipStreamWaitEvent(s_comm_, ev_stats_, 0));
    comm_->allreduce_sum_f64(d, n, s_comm_);
    wait(s_comm_);
  }
  HIP_CHECK(hipMemcpyAsync(h, d, n * sizeof(double), hipMemcpyDeviceToHost, s_comp_));
  wait(s_comp_);
}

std::vector<int> Solver::all_planes() const {
  std::vector<int> ys(plan_.NY);
  for (int j = 0; j < plan_.NY; ++j) ys[j] = j;
  return ys;
}

// The pressure mode of the export: the x-backward of one spectral field (default Pi, field 0 of d_pres_;
// the scalar's flux pass: theta) for the planes of the chunk (xc, sc) into slot 3 of the scratch; returns
// its single-field arguments.  The field's mean line is transformed as it is.
XArgs Solver::pi_backward(const XArgs& xc, const XSrc& sc, const void* field) {
  XArgs xp = xc;
  xp.nfields = 1;
  xp.combine = 0;
  xp.zero_mean_field = -1;
  XSrc sp;
  sp.base = static_cast<const char*>(field ? field : d_pres_) + (static_cast<const char*>(sc.base) - static_cast<const char*>(out_));
  sp.nsrc = 1;
  sp.kx_start[0] = 0;
  sp.kx_start[1] = plan_.nkx;
  xfft_backward(xp, sp, static_cast<char*>(phys_) + 3 * physn_ * esz_, tw_x_, fp64_, s_comp_);
  return xp;
}

ZRealArgs Solver::zreal_args(int y0, int ny, int nf) const {
  ZRealArgs za;
  za.NX = plan_.NX;
  za.Nzp = plan_.Nzp;
  za.nkz = plan_.nkz;
  za.xpitch = xpitch_;
  za.ny = ny;
  za.y0 = y0;
  za.nfields = nf;
  za.field_stride = static_cast<long long>(physn_);
  za.U = d_mean_;
  za.NY = plan_.NY;
  return za;
}

// ---- spectra --------------------------------------------------------------------------------------
Solver::Spectra Solver::spectra() {
  const Plan& p = plan_;
  Spectra out;
  out.planes = cfg_.spectra_plane_list();
  const int np = static_cast<int>(out.planes.size());
  const size_t nx = 3 * np * (p.Kx + 1), nz = 3 * np * p.nkz, nm = 3 * static_cast<size_t>(p.nkx) * p.nkz;
  const size_t need = (nx + nz + nm) * sizeof(double) + np * sizeof(int);
  if (spec_n_ < need) {
    if (d_spec_) HIP_CHECK(hipFree(d_spec_));
    HIP_CHECK(hipMalloc(&d_spec_, need));
    spec_n_ = need;
  }
  double* ekx = static_cast<double*>(d_spec_);
  int* planes = reinterpret_cast<int*>(ekx + nx + nz + nm);
  HIP_CHECK(hipMemsetAsync(d_spec_, 0, (nx + nz + nm) * sizeof(double), s_comp_));
  HIP_CHECK(hipMemcpyAsync(planes, out.planes.data(), np * sizeof(int), hipMemcpyHostToDevice, s_comp_));
  SpectraArgs a;
  a.ax = p.ax;
  a.az = p.az;
  a.combine = combine_ ? 1 : 0;
  a.nkz_loc = p.nkz_loc;
  a.nkzs = nkzs_;
  a.kzb = kzb_;
  a.kz0 = p.kz0;
  a.nkx = p.nkx;
  a.Kx = p.Kx;
  a.nkz = p.nkz;
  a.planes = planes;
  a.nplanes = np;
  a.ekx = ekx;
  a.ekz = ekx + nx;
  a.map = ekx + nx + nz;
  for_kblocks([&](size_t off, int cnt, int kx0) {  // (accumulating; map rows are disjoint)
    auto at = [&](int f) { return static_cast<const char*>(field_ptr(f)) + off; };
    a.dv = a.u = at(OUT0);
    a.v = at(OUT1);
    a.w = at(OUT2);
    a.om = at(OMEGA);
    a.lines = cnt * nkzs_;
    a.nkx_loc = cnt;
    a.kx0 = kx0;
    spectra_accumulate(a, fp64_, s_comp_);
  });
  std::vector<double> h(nx + nz + nm);
  reduce_fetch(ekx, h.size(), h.data());
  out.ekx.assign(h.begin(), h.begin() + nx);
  out.ekz.assign(h.begin() + nx, h.begin() + nx + nz);
  out.map.assign(h.begin() + nx + nz, h.end());
  return out;
}

void Solver::write_spectra_files(const Spectra& sp) {
  if (plan_.rank != 0) return;
  const Plan& p = plan_;
  const int np = static_cast<int>(sp.planes.size());
  const double N2 = static_cast<double>(p.NX) * p.Nzp;
  // reference layout (statistics.cu:272-320): NX rows (FFT-order kx) x NZ columns of |q|^2 in the
  // file units (N2 * coefficient), plane planes[0]; overwritten each time like the reference's "w"
  const char* maps[3] = {"Uspec.dat", "Vspec.dat", "Wspec.dat"};
  for (int q = 0; q < 3; ++q) {
    std::ofstream f(cfg_.path + maps[q]);
    std::vector<int> ig_of_pos(p.NX, -1);
    for (int i = 0; i < p.nkx; ++i) ig_of_pos[p.kx_fft_pos(i)] = i;
    for (int x = 0; x < p.NX; ++x) {
      for (int kz = 0; kz < p.NZ; ++kz) {
        double v = 0.0;
        if (ig_of_pos[x] >= 0 && kz < p.nkz) v = sp.map[(static_cast<size_t>(q) * p.nkx + ig_of_pos[x]) * p.nkz + kz];
        f << " " << std::fixed << v * N2 * N2;
      }
      f << " \n";
    }
  }
  // time series of 1-D spectra (true-coefficient units): one line per (plane, component)
  auto app = [&](const char* name) { return std::ofstream(cfg_.path + name, std::ios::app); };
  auto fx = app("SPECTRA_KX.dat");
  auto fz = app("SPECTRA_KZ.dat");
  const double t = time();
  for (int pl = 0; pl < np; ++pl)
    for (int q = 0; q < 3; ++q) {
      fx << nstep_ << " " << std::scientific << t << " " << sp.planes[pl] << " " << "uvw"[q];
      for (int k = 0; k <= p.Kx; ++k) fx << " " << sp.ekx[(static_cast<size_t>(q) * np + pl) * (p.Kx + 1) + k];
      fx << "\n";
      fz << nstep_ << " " << std::scientific << t << " " << sp.planes[pl] << " " << "uvw"[q];
      for (int k = 0; k < p.nkz; ++k) fz << " " << sp.ekz[(static_cast<size_t>(q) * np + pl) * p.nkz + k];
      fz << "\n";
    }
}

// ---- physical-space export ------------------------------------------------------------------------
// The x-backward addresses any plane range of the fields: rows spec_y0 + y through spec_row_off in
// the blocked layout, planes past ny clamped at the loads and masked at the stores (also in the
// plane tiles of the wide kernels), so a run of planes is transformed as it is requested.
void Solver::export_planes(const std::vector<int>& ys, int nf, unsigned out_mask, double* d_mom,
                           const std::function<void(int, int, const void*)>& sink, double* d_triple, bool pres,
                           double* d_pmom, const ZRealArgs* hist) {
  CH_CHECK(!comm_, "physical-space export is single-rank: it needs a solver without a communicator");
  const Plan& p = plan_;
  if (!prepared_) prepare();
  // pressure mode: u, v, w and Pi (field 0 of d_pres_, x-transformed into slot 3 of the scratch); the
  // solve runs first, its transform stage uses the same scratch
  CH_CHECK(!pres || (nf == 4 && (out_mask & 7u) == (out_mask & ~8u) && !d_triple), "export: the pressure mode takes u, v, w, p");
  if (pres) pressure_device();
  const int cap = ychunk_ > 0 && ychunk_ < p.ny_loc ? ychunk_ : p.ny_loc;
  const size_t tsz = fp64_ ? sizeof(double) : sizeof(float);
  const size_t plane = static_cast<size_t>(p.NX) * p.Nzp;
  int nslots = 0;
  for (int f = 0; f < 6; ++f) nslots += (out_mask >> f) & 1u;
  if (nslots) {
    const size_t need = static_cast<size_t>(nslots) * cap * plane * tsz;
    if (real_n_ < need) {
      HIP_CHECK(hipStreamSynchronize(s_comp_));
      if (d_real_) HIP_CHECK(hipFree(d_real_));
      d_real_ = nullptr;
      real_n_ = 0;
      HIP_CHECK(hipMalloc(&d_real_, need));
      real_n_ = need;
    }
  }
  XArgs xa = x_args();
  const XSrc src = x_src_local(xa);
  std::vector<char> host;
  for (size_t i = 0; i < ys.size();) {
    size_t j = i + 1;
    while (j < ys.size() && ys[j] == ys[j - 1] + 1 && static_cast<int>(j - i) < cap) ++j;
    const int y0 = ys[i], ny = static_cast<int>(j - i);
    i = j;
    XArgs xc;
    XSrc sc;
    x_chunk(xa, src, y0, ny, xc, sc);
    if (!combine_) xc.nfields = pres ? 3 : nf;  // (the combine mode forms all six)
    xfft_backward(xc, sc, phys_, tw_x_, fp64_, s_comp_);
    if (pres) pi_backward(xc, sc);
    ZRealArgs za = zreal_args(y0, ny, nf);
    za.out = nslots ? d_real_ : nullptr;
    za.out_mask = out_mask;
    za.out_field_stride = static_cast<long long>(ny * plane);
    za.moments = d_mom;
    za.triple = d_triple;
    za.pres = pres ? 1 : 0;
    za.pmom = d_pmom;
    if (hist) {  // (the tables and outputs of the histogram pass)
      za.nhf = hist->nhf;
      za.nb = hist->nb;
      za.nj = hist->nj;
      za.hcentre = hist->hcentre;
      za.hscale = hist->hscale;
      za.hist = hist->hist;
      za.joint = hist->joint;
      za.quad = hist->quad;
      za.hmerge = hist->hmerge;
    }
    zreal(za, phys_, tw_z_, fp64_, s_comp_);
    if (nslots) {
      host.resize(static_cast<size_t>(nslots) * ny * plane * tsz);
      HIP_CHECK(hipMemcpyAsync(host.data(), d_real_, host.size(), hipMemcpyDeviceToHost, s_comp_));
      HIP_CHECK(hipStreamSynchronize(s_comp_));
      sink(y0, ny, host.data());
    }
  }
}

// The planes `planes` of the fields fidx (phys_field_index values) through their export passes:
// put(k, y, src) receives plane y of field fidx[k] in the storage precision.
template <typename Put>
void Solver::export_fields(const std::vector<int>& planes, const std::vector<int>& fidx, Put&& put) {
  const size_t psz = static_cast<size_t>(plan_.NX) * plan_.Nzp * (fp64_ ? sizeof(double) : sizeof(float));
  const std::vector<int> ys = distinct_sorted(planes);
  for (const ExportPass& ps : export_passes(fidx))
    export_planes(ys, ps.nf, ps.mask, nullptr, [&](int y0, int ny, const void* h) {
      for (size_t k = 0; k < fidx.size(); ++k) {
        const int sl = ps.slot(fidx[k]);
        for (int y = 0; sl >= 0 && y < ny; ++y) put(k, y0 + y, static_cast<const char*>(h) + (static_cast<size_t>(sl) * ny + y) * psz);
      }
    }, nullptr, ps.pres);
}

Solver::PhysFields Solver::physical_fields(const std::vector<int>& planes, const std::vector<std::string>& names) {
  CH_CHECK(!comm_, "physical_fields: the export is single-rank (a solver without a communicator)");
  const Plan& p = plan_;
  CH_CHECK(!names.empty() && !planes.empty(), "physical_fields: no fields or no planes requested");
  std::vector<int> fidx;
  for (const std::string& nm : names) {
    const int f = phys_field_index(nm);
    CH_CHECK(f >= 0, "physical_fields: unknown field '" << nm << "' (u, v, w, wx, wy, wz, p)");
    fidx.push_back(f);
  }
  for (int y : planes) CH_CHECK(y >= 0 && y < p.NY, "physical_fields: plane " << y << " outside [0, NY)");
  PhysFields out;
  out.planes = planes;
  out.names = names;
  out.NX = p.NX;
  out.Nzp = p.Nzp;
  const size_t plane = static_cast<size_t>(p.NX) * p.Nzp, np = planes.size();
  out.data.resize(names.size() * np * plane);
  const auto pos = plane_positions(planes, p.NY);
  export_fields(planes, fidx, [&](size_t k, int y, const char* src) {
    for (size_t i : pos[y]) {
      double* d = out.data.data() + (k * np + i) * plane;
      if (fp64_) std::copy(reinterpret_cast<const double*>(src), reinterpret_cast<const double*>(src) + plane, d);
      else std::copy(reinterpret_cast<const float*>(src), reinterpret_cast<const float*>(src) + plane, d);
      if (fidx[k] == kPresField) subtract_mean(d, plane);  // (after widening)
    }
  });
  return out;
}

std::vector<double> Solver::plane_moments() {
  CH_CHECK(!comm_, "plane_moments: the export is single-rank (a solver without a communicator)");
  const size_t n = static_cast<size_t>(kMomRows) * plan_.NY, na = static_cast<size_t>(kMomRows + kTripleRows) * plan_.NY;
  if (!d_mom_) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_mom_), na * sizeof(double)));
  if (!prepared_) prepare();
  HIP_CHECK(hipMemsetAsync(d_mom_, 0, n * sizeof(double), s_comp_));
  export_planes(all_planes(), 3, 0u, d_mom_, nullptr);
  std::vector<double> m(n);
  reduce_fetch(d_mom_, n, m.data());
  return m;
}

// the mixed triple products of the turbulent-transport terms: the export stage over every plane
// with the (w, v) second pair (kernels.hpp ZRealArgs::triple); the moments it forms on the way are
// dropped
std::vector<double> Solver::transport_moments() {
  CH_CHECK(!comm_, "transport_moments: the export is single-rank (a solver without a communicator)");
  const size_t n = static_cast<size_t>(kMomRows) * plan_.NY, nt = static_cast<size_t>(kTripleRows) * plan_.NY;
  if (!d_mom_) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_mom_), (n + nt) * sizeof(double)));
  if (!prepared_) prepare();
  HIP_CHECK(hipMemsetAsync(d_mom_, 0, (n + nt) * sizeof(double), s_comp_));
  export_planes(all_planes(), 3, 0u, d_mom_, nullptr, d_mom_ + n);
  std::vector<double> m(nt);
  reduce_fetch(d_mom_ + n, nt, m.data());
  return m;
}

// ---- histograms ------------------------------------------------------------------------------------
namespace {
// the compact first derivative of a profile on the host (grid.hpp: tridiag(lo, 1, up) f' = rhs)
std::vector<double> d1_profile(const YGrid& g, const std::vector<double>& f) {
  const int N = g.N;
  std::vector<double> r(N), c(N), d(N);
  for (int j = 1; j < N - 1; ++j) r[j] = g.d1_rm[j] * f[j - 1] + g.d1_rc[j] * f[j] + g.d1_rp[j] * f[j + 1];
  r[0] = g.d1_w0[0] * f[0] + g.d1_w0[1] * f[1] + g.d1_w0[2] * f[2];
  r[N - 1] = g.d1_wN[0] * f[N - 1] + g.d1_wN[1] * f[N - 2] + g.d1_wN[2] * f[N - 3];
  c[0] = g.d1_up[0];
  d[0] = r[0];
  for (int j = 1; j < N; ++j) {
    const double m = 1.0 - g.d1_lo[j] * c[j - 1];
    c[j] = g.d1_up[j] / m;
    d[j] = (r[j] - g.d1_lo[j] * d[j - 1]) / m;
  }
  for (int j = N - 2; j >= 0; --j) d[j] -= c[j] * d[j + 1];
  return d;
}
const char* const kHistNames[6] = {"u", "v", "w", "wx", "wy", "wz"};
}  // namespace

// CHANNEL_HIST_MERGE=0|1: one LDS atomic per sample, or equal consecutive bins of a thread's 16-byte
// piece merged into one (A/B; profiles/pdfs/README.md has the measurement behind the default)
static int hist_merge_env() {
  const char* e = std::getenv("CHANNEL_HIST_MERGE");
  return e ? (std::atoi(e) != 0 ? 1 : 0) : 1;
}

Solver::PlaneHistograms Solver::plane_histograms(const std::vector<int>& planes, int nbins, int njoint, double span,
                                                 bool vorticity, const std::vector<double>& centre,
                                                 const std::vector<double>& halfwidth) {
  CH_CHECK(!comm_, "plane_histograms: the export is single-rank (a solver without a communicator)");
  const Plan& p = plan_;
  const int N = p.NY, nhf = vorticity ? 6 : 3, np = static_cast<int>(planes.size());
  CH_CHECK(np > 0, "plane_histograms: no planes requested");
  for (int y : planes) CH_CHECK(y >= 0 && y < N, "plane_histograms: plane " << y << " outside [0, NY)");
  CH_CHECK(distinct_sorted(planes).size() == planes.size(), "plane_histograms: a plane is listed twice");
  CH_CHECK(nbins >= 2 && nbins % 2 == 0 && nbins <= kHistMaxBins, "plane_histograms: nbins must be even, in [2, " << kHistMaxBins << "]");
  CH_CHECK(njoint >= 1 && njoint <= kHistMaxJoint && nbins % njoint == 0,
           "plane_histograms: njoint must divide nbins and be at most " << kHistMaxJoint);
  CH_CHECK(span > 0, "plane_histograms: span must be positive");
  const size_t nfp = static_cast<size_t>(nhf) * np;
  CH_CHECK(centre.empty() || centre.size() == nfp, "plane_histograms: centre must have shape (" << nhf << ", " << np << ")");
  CH_CHECK(halfwidth.empty() || halfwidth.size() == nfp, "plane_histograms: halfwidth must have shape (" << nhf << ", " << np << ")");
  for (double h : halfwidth) CH_CHECK(h > 0 && std::isfinite(h), "plane_histograms: halfwidth must be positive");
  for (double c : centre) CH_CHECK(std::isfinite(c), "plane_histograms: centre must be finite");
  if (!prepared_) prepare();

  PlaneHistograms out;
  out.planes = planes;
  out.names.assign(kHistNames, kHistNames + nhf);
  out.nb = nbins;
  out.nj = njoint;
  out.centre = centre;
  out.halfwidth = halfwidth;
  if (centre.empty()) {
    out.centre.assign(nfp, 0.0);
    const std::vector<double> U = mean_profile();
    const std::vector<double> dU = vorticity ? d1_profile(grid_, U) : std::vector<double>();
    for (int i = 0; i < np; ++i) {
      out.centre[i] = U[planes[i]];
      if (vorticity) out.centre[5 * static_cast<size_t>(np) + i] = -dU[planes[i]];
    }
  }
  if (halfwidth.empty()) {
    // the r.m.s. of the state that is binned: <u'^2>, <v^2>, <w^2> are rows 1..3 of the moments
    out.halfwidth.assign(nfp, 1.0);
    const std::vector<double> m = plane_moments();
    const std::vector<double> g = vorticity ? gradient_sums() : std::vector<double>();
    for (int f = 0; f < nhf; ++f)
      for (int i = 0; i < np; ++i) {
        const double ms = f < 3 ? m[static_cast<size_t>(1 + f) * N + planes[i]] : g[static_cast<size_t>(f - 3) * N + planes[i]];
        // the r.m.s. rounded to 12 significant bits: the plane sums are atomic and differ in their last
        // bits from call to call, which must not move the bin edges between two calls on one state
        int ex = 0;
        const double mant = ms > 0 && std::isfinite(ms) ? std::frexp(std::sqrt(ms), &ex) : 0.0;
        const double rms = std::ldexp(std::round(mant * 4096.0) / 4096.0, ex);
        if (rms > 0) out.halfwidth[static_cast<size_t>(f) * np + i] = span * rms;
      }
  }

  // device: hist [nhf][NY][nb + 2] and joint [NY][nj + 2][nj + 2] (64-bit counts), quad [kQuadRows][NY],
  // then centre and scale [nhf][NY] (planes that are not requested: 0 and 1, never read)
  const size_t hb2 = nbins + 2, jb2 = njoint + 2;
  const size_t nh = static_cast<size_t>(nhf) * N * hb2, nj2 = static_cast<size_t>(N) * jb2 * jb2, nq = static_cast<size_t>(kQuadRows) * N;
  const size_t ncs = static_cast<size_t>(nhf) * N;
  const size_t need = (nh + nj2 + nq + 2 * ncs) * 8;
  if (hist_n_ < need) {
    HIP_CHECK(hipStreamSynchronize(s_comp_));
    if (d_hist_) HIP_CHECK(hipFree(d_hist_));
    if (h_hist_) HIP_CHECK(hipHostFree(h_hist_));
    d_hist_ = h_hist_ = nullptr;
    hist_n_ = 0;
    HIP_CHECK(hipMalloc(&d_hist_, need));
    // (through pinned memory: a copy into fresh pageable vectors runs at a fraction of the link's rate)
    HIP_CHECK(hipHostMalloc(&h_hist_, need, hipHostMallocDefault));
    hist_n_ = need;
  }
  unsigned long long* d_h = static_cast<unsigned long long*>(d_hist_);
  double* d_q = reinterpret_cast<double*>(d_h + nh + nj2);
  std::vector<double> cs(2 * ncs, 0.0);
  std::fill(cs.begin() + ncs, cs.end(), 1.0);
  for (int f = 0; f < nhf; ++f)
    for (int i = 0; i < np; ++i) {
      cs[static_cast<size_t>(f) * N + planes[i]] = out.centre[static_cast<size_t>(f) * np + i];
      cs[ncs + static_cast<size_t>(f) * N + planes[i]] = nbins / (2.0 * out.halfwidth[static_cast<size_t>(f) * np + i]);
    }
  HIP_CHECK(hipMemsetAsync(d_hist_, 0, (nh + nj2 + nq) * 8, s_comp_));
  HIP_CHECK(hipMemcpyAsync(d_q + nq, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice, s_comp_));
  ZRealArgs hz;
  hz.nhf = nhf;
  hz.nb = nbins;
  hz.nj = njoint;
  hz.hcentre = d_q + nq;
  hz.hscale = d_q + nq + ncs;
  hz.hist = d_h;
  hz.joint = d_h + nh;
  hz.quad = d_q;
  hz.hmerge = hist_merge_env();
  export_planes(distinct_sorted(planes), nhf, 0u, nullptr, nullptr, nullptr, false, nullptr, &hz);
  const unsigned long long* h = static_cast<const unsigned long long*>(h_hist_);
  HIP_CHECK(hipMemcpyAsync(h_hist_, d_hist_, (nh + nj2 + nq) * 8, hipMemcpyDeviceToHost, s_comp_));
  wait(s_comp_);
  out.hist.resize(nfp * hb2);
  out.joint.resize(static_cast<size_t>(np) * jb2 * jb2);
  out.quad.resize(static_cast<size_t>(kQuadRows) * np);
  const double* hq = reinterpret_cast<const double*>(h + nh + nj2);
  const double inv = 1.0 / (static_cast<double>(p.NX) * p.Nzp);
  for (int i = 0; i < np; ++i) {
    const size_t y = static_cast<size_t>(planes[i]);
    for (int f = 0; f < nhf; ++f)
      std::copy(h + (f * static_cast<size_t>(N) + y) * hb2, h + (f * static_cast<size_t>(N) + y + 1) * hb2,
                out.hist.begin() + (static_cast<size_t>(f) * np + i) * hb2);
    std::copy(h + nh + y * jb2 * jb2, h + nh + (y + 1) * jb2 * jb2, out.joint.begin() + static_cast<size_t>(i) * jb2 * jb2);
    for (int q = 0; q < kQuadRows; ++q) out.quad[static_cast<size_t>(q) * np + i] = hq[static_cast<size_t>(q) * N + y] * inv;
  }
  return out;
}

// <path>PDF_<step>.npy (nhf, np, nb + 2), <path>JPDF_UV_<step>.npy (np, nj + 2, nj + 2), both uint64,
// <path>QUAD_<step>.npy (8, np) float64 and a sidecar <path>PDF_<step>.json with the centres and
// half-widths of this write (each write bins about its own step's r.m.s.)
void Solver::write_pdf_files() {
  if (comm_) return note_once(pdf_note_, plan_.rank,
                              "[channel] pdf_every: PDF_*.npy, JPDF_UV_*.npy, QUAD_*.npy skipped (the export is single-rank)\n");
  const std::vector<int> planes = distinct_sorted(cfg_.pdf_plane_list());
  const PlaneHistograms ph = plane_histograms(planes, cfg_.pdf_bins, cfg_.pdf_joint_bins, cfg_.pdf_span, cfg_.pdf_vorticity != 0);
  const size_t nhf = ph.names.size(), np = planes.size();
  char step[16];
  std::snprintf(step, sizeof(step), "%08ld", nstep_);
  auto put = [&](const char* name, const char* descr, const std::string& shape, const void* v, size_t bytes) {
    const std::string fn = cfg_.path + name + step + ".npy";
    std::ofstream f(fn, std::ios::binary | std::ios::trunc);
    CH_CHECK(f.good(), "cannot open '" << fn << "'");
    const std::string h = npy_header(descr, shape);
    f.write(h.data(), static_cast<std::streamsize>(h.size()));
    f.write(static_cast<const char*>(v), static_cast<std::streamsize>(bytes));
    f.close();
    CH_CHECK(!f.fail(), "writing '" << fn << "' failed");
  };
  auto s = [](size_t v) { return std::to_string(v); };
  put("PDF_", "<u8", "(" + s(nhf) + ", " + s(np) + ", " + s(ph.nb + 2) + ")", ph.hist.data(), ph.hist.size() * 8);
  put("JPDF_UV_", "<u8", "(" + s(np) + ", " + s(ph.nj + 2) + ", " + s(ph.nj + 2) + ")", ph.joint.data(), ph.joint.size() * 8);
  put("QUAD_", "<f8", "(" + s(kQuadRows) + ", " + s(np) + ")", ph.quad.data(), ph.quad.size() * 8);
  std::ofstream js(cfg_.path + "PDF_" + step + ".json");
  js.precision(17);
  js << "{\"step\": " << nstep_ << ", \"time\": " << time() << ", \"planes\": [";
  for (size_t i = 0; i < np; ++i) js << (i ? ", " : "") << planes[i];
  js << "], \"y\": [";
  for (size_t i = 0; i < np; ++i) js << (i ? ", " : "") << grid_.y[planes[i]];
  js << "], \"names\": [";
  for (size_t k = 0; k < nhf; ++k) js << (k ? ", " : "") << "\"" << ph.names[k] << "\"";
  js << "], \"nbins\": " << ph.nb << ", \"njoint\": " << ph.nj << ", \"span\": " << cfg_.pdf_span << ", \"Re\": " << cfg_.Re;
  auto rows = [&](const char* key, const std::vector<double>& v) {
    js << ", \"" << key << "\": [";
    for (size_t k = 0; k < nhf; ++k) {
      js << (k ? ", [" : "[");
      for (size_t i = 0; i < np; ++i) js << (i ? ", " : "") << v[k * np + i];
      js << "]";
    }
    js << "]";
  };
  rows("centre", ph.centre);
  rows("halfwidth", ph.halfwidth);
  js << "}\n";
}

// ---- pressure ------------------------------------------------------------------------------------
// The step's transform stage (x-backward, z stage, x-forward; substep index 1: no CFL maxima, no dt
// update) once more, from K-SPEC's outputs of the current state into d_pres_ instead of over them,
// then the y-line Poisson solve in place over H_x.  state_ and out_ are only read: the next step sees
// what it would have seen.  phys_ is scratch between steps, as the export assumes.
void Solver::pressure_device(double* ms) {
  CH_CHECK(!comm_, "pressure: the pressure solve is single-rank (a solver without a communicator)");
  if (!prepared_) prepare();
  hipEvent_t te[3] = {nullptr, nullptr, nullptr};
  if (ms) {
    for (hipEvent_t& e : te) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(te[0], s_comp_));
  }
  rotational_device();
  if (ms) HIP_CHECK(hipEventRecord(te[1], s_comp_));
  poisson_device();
  if (ms) {
    HIP_CHECK(hipEventRecord(te[2], s_comp_));
    HIP_CHECK(hipStreamSynchronize(s_comp_));
    float t01 = 0, t12 = 0;
    HIP_CHECK(hipEventElapsedTime(&t01, te[0], te[1]));
    HIP_CHECK(hipEventElapsedTime(&t12, te[1], te[2]));
    ms[0] = t01;
    ms[1] = t12;
    for (hipEvent_t e : te) (void)hipEventDestroy(e);
  }
}

// the first half: H = (u x omega)^ of the current state into the three fields of d_pres_
void Solver::rotational_device() {
  CH_CHECK(!comm_, "pressure: the pressure solve is single-rank (a solver without a communicator)");
  if (!prepared_) prepare();
  if (!d_pres_) {
    HIP_CHECK(hipMalloc(&d_pres_, 3 * spec_ * esz_));
    HIP_CHECK(hipMemsetAsync(d_pres_, 0, 3 * spec_ * esz_, s_comp_));
  }
  transforms(1, false, d_pres_);
}

// the second half: the y-line Poisson solve, Pi in place over H_x
void Solver::poisson_device() {
  const Plan& p = plan_;
  PressureArgs a;
  a.N = p.NY;
  a.lines = p.nkx_loc * nkzs_;
  a.nkz = nkzs_;
  a.nkz_real = p.nkz_loc;
  a.kzb = kzb_;
  a.kz0 = p.kz0;
  a.kx0 = p.kx0;
  a.nkx = p.nkx;
  a.Kx = p.Kx;
  a.ax = p.ax;
  a.az = p.az;
  a.nu = 1.0 / cfg_.Re;
  char* h = static_cast<char*>(d_pres_);
  a.hx = h;
  a.hy = h + spec_ * esz_;
  a.hz = h + 2 * spec_ * esz_;
  a.phi = field_ptr(PHI);
  a.pi = h;
  pressure_solve(ytab_, a, fp64_, s_comp_);
}

std::vector<std::complex<double>> Solver::rotational_hat() {
  rotational_device();
  std::vector<std::complex<double>> out;
  out.reserve(3 * canon_);
  for (int c = 0; c < 3; ++c) {
    const std::vector<std::complex<double>> h = spec_to_canonical(static_cast<const char*>(d_pres_) + c * spec_ * esz_, "rotational term");
    out.insert(out.end(), h.begin(), h.end());
  }
  return out;
}

std::vector<double> Solver::pressure_timing() {
  std::vector<double> ms(2, 0.0);
  pressure_device(ms.data());
  return ms;
}

std::vector<std::complex<double>> Solver::pressure_hat() {
  pressure_device();
  return spec_to_canonical(d_pres_, "pressure");
}

// one spectral field on the device (one rank) as canonical [y][kx][kz] complex128 on the host
std::vector<std::complex<double>> Solver::spec_to_canonical(const void* d_field, const char* what) {
  const Plan& p = plan_;
  std::vector<char> h(spec_ * esz_);
  HIP_CHECK(hipMemcpyAsync(h.data(), d_field, h.size(), hipMemcpyDeviceToHost, s_comp_));
  HIP_CHECK(hipStreamSynchronize(s_comp_));
  std::vector<std::complex<double>> t(spec_);
  for (size_t i = 0; i < spec_; ++i) {
    if (fp64_) t[i] = {reinterpret_cast<const double2*>(h.data())[i].x, reinterpret_cast<const double2*>(h.data())[i].y};
    else t[i] = {reinterpret_cast<const float2*>(h.data())[i].x, reinterpret_cast<const float2*>(h.data())[i].y};
  }
  // device layout -> canonical [y][kx][kz]; what is left behind (padded kz lines and rows of the
  // blocked layout) must be exactly zero: the x transform of the export reads whole tiles
  std::vector<std::complex<double>> out(canon_);
  for (int y = 0; y < p.NY; ++y)
    for (int i = 0; i < p.nkx_loc; ++i)
      for (int k = 0; k < p.nkz_loc; ++k) {
        std::complex<double>& e = t[dev_index(y, i, k)];
        out[(static_cast<size_t>(y) * p.nkx_loc + i) * p.nkz_loc + k] = e;
        e = 0.0;
      }
  size_t bad = 0;
  for (size_t i = 0; i < spec_; ++i) bad += (t[i].real() != 0.0 || t[i].imag() != 0.0) ? 1 : 0;
  CH_CHECK(bad == 0, what << ": " << bad << " padding elements of the spectral layout are not zero");
  return out;
}

std::vector<double> Solver::pressure_moments() {
  CH_CHECK(!comm_, "pressure_moments: the export is single-rank (a solver without a communicator)");
  const size_t N = static_cast<size_t>(plan_.NY), nm = kMomRows * N, np = kPresRows * N;
  if (!d_pmom_) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_pmom_), (nm + np) * sizeof(double)));
  if (!prepared_) prepare();
  HIP_CHECK(hipMemsetAsync(d_pmom_, 0, (nm + np) * sizeof(double), s_comp_));
  // (the moments give <u'>, which is zero to rounding but is subtracted all the same, <v> and <w>
  // are exactly the mean line's zeros)
  export_planes(all_planes(), 4, 0u, d_pmom_, nullptr, nullptr, true, d_pmom_ + nm);
  std::vector<double> h(nm + np);
  reduce_fetch(d_pmom_, nm + np, h.data());
  // central moments: <p'p'> = <r^2> - <r>^2, <p'u'> = <r u'> - <r><u'>, <p'v> = <r v>, <p'w> = <r w>
  std::vector<double> m(4 * N);
  const double* r = h.data() + nm;
  for (size_t j = 0; j < N; ++j) {
    const double rm = r[j], um = h[j];
    m[j] = r[N + j] - rm * rm;
    m[N + j] = r[2 * N + j] - rm * um;
    m[2 * N + j] = r[3 * N + j];
    m[3 * N + j] = r[4 * N + j];
  }
  return m;
}

// one line of NY values per call and file, as write_stats_files: the pressure r.m.s. and <p'u'>, <p'v>
void Solver::write_pressure_files() {
  if (comm_) return note_once(pres_note_, plan_.rank,
                              "[channel] pressure_every: PRMS.dat, PU.dat, PV.dat skipped (the pressure solve is single-rank)\n");
  const std::vector<double> m = pressure_moments();
  const int N = plan_.NY;
  append_profile(cfg_.path + "PRMS.dat", m.data(), N, 1.0, true);
  append_profile(cfg_.path + "PU.dat", m.data() + N, N);
  append_profile(cfg_.path + "PV.dat", m.data() + 2 * N, N);
}

// ---- spectral static pressure, pressure-strain -------------------------------------------------------
// The pressure-mode export pass over every plane with the return trip of r (kernels.hpp
// ZRealArgs::spec_out): per chunk the x-backward of u, v, w and of Pi (into slot 3 of the scratch), the
// z kernel, which leaves r-hat(x, kz) in slot 3, and the forward x transform of that one field into
// the chunk's planes of field 1 of d_pres_ (the H_y slot, free after the solve; Pi stays in field 0).
// The mean line, which holds <r>, is zeroed; the padding of the blocked layout is never written and
// stays the zeros of the allocation.  Like the export it writes nothing the next step reads.
void Solver::static_pressure_device() {
  CH_CHECK(!comm_, "static_pressure: the export is single-rank (a solver without a communicator)");
  pressure_device();
  static_return_device();
}

// the second half: from Pi in field 0 of d_pres_ to p-hat' in field 1
void Solver::static_return_device() {
  const Plan& p = plan_;
  const int cap = ychunk_ > 0 && ychunk_ < p.ny_loc ? ychunk_ : p.ny_loc;
  XArgs xa = x_args();
  const XSrc src = x_src_local(xa);
  char* slot3 = static_cast<char*>(phys_) + 3 * physn_ * esz_;
  char* phat = static_cast<char*>(d_pres_) + spec_ * esz_;
  for (int y0 = 0; y0 < p.NY; y0 += cap) {
    const int ny = std::min(cap, p.NY - y0);
    XArgs xc;
    XSrc sc;
    x_chunk(xa, src, y0, ny, xc, sc);
    if (!combine_) xc.nfields = 3;  // (the combine mode forms all six)
    xfft_backward(xc, sc, phys_, tw_x_, fp64_, s_comp_);
    const XArgs xp = pi_backward(xc, sc);
    ZRealArgs za = zreal_args(y0, ny, 4);
    za.pres = 1;
    za.spec_out = slot3;
    zreal(za, phys_, tw_z_, fp64_, s_comp_);
    // (the chunk's planes of the destination, as transforms() addresses them)
    XDst dc;
    dc.base = phat + (static_cast<const char*>(sc.base) - static_cast<const char*>(out_));
    dc.ndst = 1;
    dc.kx_start[0] = 0;
    dc.kx_start[1] = p.nkx;
    xfft_forward(xp, slot3, dc, tw_x_, fp64_, s_comp_);
  }
  zero_mean_line(phat, p.NY, kzb_, p.nkx_loc * nkzs_, fp64_, s_comp_);
}

std::vector<std::complex<double>> Solver::static_pressure_hat() {
  static_pressure_device();
  return spec_to_canonical(static_cast<const char*>(d_pres_) + spec_ * esz_, "static pressure");
}

// ---- the all-plane reductions over the spectral fields -------------------------------------------
// As spectra(): K-SPEC's outputs of the current state are read in place, one launch per kx sub-block on
// the compute stream, one all-reduce over the result.
std::vector<double> Solver::pressure_strain() {
  CH_CHECK(!comm_, "pressure_strain: the export is single-rank (a solver without a communicator)");
  const size_t n = static_cast<size_t>(kPStrainRows) * plan_.NY;
  if (!d_pstr_) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_pstr_), n * sizeof(double)));
  static_pressure_device();
  HIP_CHECK(hipMemsetAsync(d_pstr_, 0, n * sizeof(double), s_comp_));
  PStrainArgs a;
  walk_args(a, 1u | 2u | 4u | 32u, true);  // u, v, w, omega_z
  a.sums = d_pstr_;
  for_kblocks([&](size_t off, int cnt, int kx0) { pstrain_accumulate(at_block(a, off, cnt, kx0), fp64_, s_comp_); });
  std::vector<double> g(n);
  reduce_fetch(d_pstr_, n, g.data());
  return g;
}

// one line of NY values per call and file, as write_stats_files: the pressure-strain terms of the uu,
// vv, ww, uv budgets
void Solver::write_pstrain_files() {
  if (comm_) return note_once(pstr_note_, plan_.rank,
                              "[channel] pstrain_every: PS_UU.dat, PS_VV.dat, PS_WW.dat, PS_UV.dat skipped (the export is single-rank)\n");
  const std::vector<double> m = pressure_strain();
  const int N = plan_.NY;
  const char* names[4] = {"PS_UU.dat", "PS_VV.dat", "PS_WW.dat", "PS_UV.dat"};
  for (int q = 0; q < 4; ++q) append_profile(cfg_.path + names[q], m.data() + static_cast<size_t>(q) * N, N);
}

// ---- passive scalar ------------------------------------------------------------------------------------
std::vector<std::complex<double>> Solver::scalar_flux_hat() {
  CH_CHECK(sc_, "scalar_flux_hat: scalar = false");
  if (!prepared_) prepare();
  scalar_flux_device();
  std::vector<std::complex<double>> out;
  out.reserve(3 * canon_);
  for (int c = 0; c < 3; ++c) {
    const std::vector<std::complex<double>> h = spec_to_canonical(scalar_ptr(2 + c), "scalar flux");
    out.insert(out.end(), h.begin(), h.end());
  }
  return out;
}

// Row 0 is the mean line of theta itself; rows 1..4 one more operation of the shared spectral walk, with
// theta in the place of p-hat' and K-SPEC's outputs read in place (the combine mode's as the spectra do).
std::vector<double> Solver::scalar_sums() {
  CH_CHECK(sc_ && !comm_, "scalar_sums: scalar = true on one rank without a communicator");
  const size_t N = static_cast<size_t>(plan_.NY), n = static_cast<size_t>(kScalarSumRows) * N;
  if (!d_ssum_) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_ssum_), n * sizeof(double)));
  if (!prepared_) prepare();
  HIP_CHECK(hipMemsetAsync(d_ssum_, 0, n * sizeof(double), s_comp_));
  ScalarSumArgs a;
  walk_args(a, 1u | 2u | 4u, false);
  a.p = scalar_ptr(0);
  a.sums = d_ssum_;
  for_kblocks([&](size_t off, int cnt, int kx0) { scalarsum_accumulate(at_block(a, off, cnt, kx0), fp64_, s_comp_); });
  std::vector<double> g(n + N);
  reduce_fetch(d_ssum_, n, g.data() + N);
  // Theta: the NY elements of the mean line alone, element (y, 0, 0) of either layout (strided copies: the
  // planes of the plain layout; row y % 8 of every 8-plane tile of the blocked one)
  std::vector<char> h(N * esz_);
  const size_t lines = static_cast<size_t>(plan_.nkx_loc) * nkzs_;
  const int nb = kzb_ ? kSpecYBlock : 1;
  for (int b = 0; b < nb && b < plan_.NY; ++b) {
    const size_t rows = (N - b + nb - 1) / nb;
    HIP_CHECK(hipMemcpy2DAsync(h.data() + b * esz_, nb * esz_, static_cast<const char*>(scalar_ptr(0)) + dev_index(b, 0, 0) * esz_,
                               nb * lines * esz_, esz_, rows, hipMemcpyDeviceToHost, s_comp_));
  }
  HIP_CHECK(hipStreamSynchronize(s_comp_));
  for (size_t j = 0; j < N; ++j)
    g[j] = fp64_ ? reinterpret_cast<const double2*>(h.data())[j].x : static_cast<double>(reinterpret_cast<const float2*>(h.data())[j].x);
  return g;
}

std::vector<double> Solver::scalar_timing() {
  CH_CHECK(sc_, "scalar_timing: scalar = false");
  if (!prepared_) prepare();
  std::vector<double> ms(4, 0.0);
  scalar_flux_device(ms.data());
  // the advance on a copy's worth of state: theta and R_theta are put back afterwards
  const size_t fb = spec_ * esz_;
  void* keep = nullptr;
  HIP_CHECK(hipMalloc(&keep, 2 * fb));
  HIP_CHECK(hipMemcpyAsync(keep, scalar_ptr(0), 2 * fb, hipMemcpyDeviceToDevice, s_comp_));
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, s_comp_));
  scalar_advance_device(0);
  HIP_CHECK(hipEventRecord(e1, s_comp_));
  HIP_CHECK(hipMemcpyAsync(scalar_ptr(0), keep, 2 * fb, hipMemcpyDeviceToDevice, s_comp_));
  HIP_CHECK(hipStreamSynchronize(s_comp_));
  float t = 0;
  HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
  ms[3] = t;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(keep);
  return ms;
}

// one line of NY values per call and file, as write_stats_files: Theta, the scalar r.m.s., <u'theta'>,
// <v theta'>; TWALL.dat: step, time and the wall derivatives of Theta by the compact D1 (on the host)
void Solver::write_scalar_files() {
  const std::vector<double> m = scalar_sums();
  const int N = plan_.NY;
  append_profile(cfg_.path + "TMEAN.dat", m.data(), N);
  append_profile(cfg_.path + "TRMS.dat", m.data() + N, N, 1.0, true);
  append_profile(cfg_.path + "UT.dat", m.data() + 2 * N, N);
  append_profile(cfg_.path + "VT.dat", m.data() + 3 * N, N);
  // D1 Theta: tridiag(d1_lo, 1, d1_up) f' = B1 Theta
  const YGrid& g = grid_;
  std::vector<double> r(N), cp(N);
  const double* f = m.data();
  r[0] = g.d1_w0[0] * f[0] + g.d1_w0[1] * f[1] + g.d1_w0[2] * f[2];
  r[N - 1] = g.d1_wN[0] * f[N - 1] + g.d1_wN[1] * f[N - 2] + g.d1_wN[2] * f[N - 3];
  for (int j = 1; j < N - 1; ++j) r[j] = g.d1_rm[j] * f[j - 1] + g.d1_rc[j] * f[j] + g.d1_rp[j] * f[j + 1];
  cp[0] = g.d1_up[0];
  for (int j = 1; j < N; ++j) {
    const double mj = 1.0 - g.d1_lo[j] * cp[j - 1];
    cp[j] = g.d1_up[j] / mj;
    r[j] = (r[j] - g.d1_lo[j] * r[j - 1]) / mj;
  }
  for (int j = N - 2; j >= 0; --j) r[j] -= cp[j] * r[j + 1];
  std::ofstream tw(cfg_.path + "TWALL.dat", std::ios::app);
  tw.precision(10);
  tw << nstep_ << " " << std::scientific << time() << " " << r[0] << " " << r[N - 1] << "\n";
}

std::vector<double> Solver::gradient_sums() {
  const size_t n = static_cast<size_t>(kGradRows) * plan_.NY;
  if (!d_grad_) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_grad_), n * sizeof(double)));
  if (!prepared_) prepare();
  HIP_CHECK(hipMemsetAsync(d_grad_, 0, n * sizeof(double), s_comp_));
  GradSumArgs a;
  walk_args(a, 63u, false);
  a.sums = d_grad_;
  for_kblocks([&](size_t off, int cnt, int kx0) { gradsum_accumulate(at_block(a, off, cnt, kx0), fp64_, s_comp_); });
  std::vector<double> g(n);
  reduce_fetch(d_grad_, n, g.data());
  return g;
}

// With the pressure row the device part of static_pressure_hat() runs first (it writes d_pres_ and the
// step's scratch).
Solver::PlaneSpectra Solver::plane_spectra(bool pressure, double* ms) {
  CH_CHECK(!pressure || !comm_, "plane_spectra: the pressure row is single-rank (a solver without a communicator)");
  const Plan& p = plan_;
  const size_t nx = static_cast<size_t>(kYSpecRows) * p.NY * (p.Kx + 1), nz = static_cast<size_t>(kYSpecRows) * p.NY * p.nkz;
  if (!d_yspec_) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_yspec_), (nx + nz) * sizeof(double)));
  if (!h_yspec_) HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_yspec_), (nx + nz) * sizeof(double), hipHostMallocDefault));
  if (!prepared_) prepare();
  if (pressure) static_pressure_device();
  HIP_CHECK(hipMemsetAsync(d_yspec_, 0, (nx + nz) * sizeof(double), s_comp_));
  YSpectraArgs a;
  walk_args(a, 63u, pressure);
  a.nkz = p.nkz;
  a.ekx = d_yspec_;
  a.ekz = d_yspec_ + nx;
  hipEvent_t te[2] = {nullptr, nullptr};
  if (ms) {
    for (hipEvent_t& e : te) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(te[0], s_comp_));
  }
  for_kblocks([&](size_t off, int cnt, int kx0) { yspectra_accumulate(at_block(a, off, cnt, kx0), fp64_, s_comp_); });
  if (ms) {
    float t = 0;
    HIP_CHECK(hipEventRecord(te[1], s_comp_));
    HIP_CHECK(hipEventSynchronize(te[1]));
    HIP_CHECK(hipEventElapsedTime(&t, te[0], te[1]));
    *ms = t;
    for (hipEvent_t e : te) (void)hipEventDestroy(e);
  }
  PlaneSpectra out;
  out.rows = {"uu", "vv", "ww", "uv", "wxwx", "wywy", "wzwz", "pp"};
  // (through pinned memory: a copy into fresh pageable vectors runs at a fraction of the link's rate)
  reduce_fetch(d_yspec_, nx + nz, h_yspec_);
  out.ekx.assign(h_yspec_, h_yspec_ + nx);
  out.ekz.assign(h_yspec_ + nx, h_yspec_ + nx + nz);
  return out;
}

// <path>YSPEC_KX_<step>.npy (8, NY, Kx+1) and <path>YSPEC_KZ_<step>.npy (8, NY, nkz), float64, and a
// sidecar <path>YSPEC_<step>.json; every rank takes part in the sums, rank 0 writes
void Solver::write_yspectra_files() {
  bool pres = cfg_.yspectra_pressure != 0;
  if (pres && comm_) {
    note_once(yspec_note_, plan_.rank,
              "[channel] yspectra_pressure: row pp of YSPEC_*.npy skipped (the pressure solve is single-rank)\n");
    pres = false;
  }
  const PlaneSpectra sp = plane_spectra(pres);
  if (plan_.rank != 0) return;
  const Plan& p = plan_;
  char step[16];
  std::snprintf(step, sizeof(step), "%08ld", nstep_);
  write_rows_npy(cfg_.path + "YSPEC_KX_" + step + ".npy", sp.ekx, kYSpecRows, p.NY, p.Kx + 1);
  write_rows_npy(cfg_.path + "YSPEC_KZ_" + step + ".npy", sp.ekz, kYSpecRows, p.NY, p.nkz);
  std::ofstream js(cfg_.path + "YSPEC_" + step + ".json");
  js.precision(17);
  js << "{\"step\": " << nstep_ << ", \"time\": " << time() << ", \"rows\": [";
  for (size_t k = 0; k < sp.rows.size(); ++k) js << (k ? ", " : "") << "\"" << sp.rows[k] << "\"";
  js << "], \"pressure\": " << (pres ? "true" : "false") << ", \"ax\": " << p.ax << ", \"az\": " << p.az << ", \"y\": [";
  for (int j = 0; j < p.NY; ++j) js << (j ? ", " : "") << grid_.y[j];
  js << "], \"Re\": " << cfg_.Re << "}\n";
}

// ---- cross-spectra against reference planes ------------------------------------------------------
// One launch set per kx sub-block with the reference planes as a grid factor, one all-reduce, one copy
// through pinned memory; the sums are sized by the reference planes of the call (17 MB each at the
// headline grid) and kept for the next one.  Reads the fields and writes its own sums only.
Solver::PlaneCrossSpectra Solver::plane_cross_spectra(const std::vector<int>& refs, const std::string& rows, double* ms) {
  const Plan& p = plan_;
  CH_CHECK(rows == "velocity" || rows == "shear", "plane_cross_spectra: unknown row set '" << rows << "' (velocity, shear)");
  CH_CHECK(!refs.empty(), "plane_cross_spectra: no reference plane");
  CH_CHECK(static_cast<int>(refs.size()) <= kYCrossMaxRefs, "plane_cross_spectra: more than " << kYCrossMaxRefs << " reference planes");
  for (size_t i = 0; i < refs.size(); ++i) {
    CH_CHECK(refs[i] >= 0 && refs[i] < p.NY, "plane_cross_spectra: reference plane " << refs[i] << " outside [0, NY)");
    for (size_t k = 0; k < i; ++k) CH_CHECK(refs[k] != refs[i], "plane_cross_spectra: reference plane " << refs[i] << " given twice");
  }
  const size_t nref = refs.size(), NY = static_cast<size_t>(p.NY), nkx = static_cast<size_t>(p.Kx) + 1, nkz = static_cast<size_t>(p.nkz);
  const size_t nx = nref * kYSpecRows * NY * nkx, nz = nref * kYSpecRows * NY * nkz;
  if (ycross_n_ < nx + nz) {
    wait(s_comp_);
    if (d_ycross_) HIP_CHECK(hipFree(d_ycross_));
    if (h_ycross_) HIP_CHECK(hipHostFree(h_ycross_));
    d_ycross_ = h_ycross_ = nullptr;
    ycross_n_ = 0;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_ycross_), (nx + nz) * sizeof(double)));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_ycross_), (nx + nz) * sizeof(double), hipHostMallocDefault));
    ycross_n_ = nx + nz;
  }
  if (!prepared_) prepare();
  hipEvent_t te[2] = {nullptr, nullptr};
  if (ms)
    for (hipEvent_t& e : te) HIP_CHECK(hipEventCreate(&e));
  HIP_CHECK(hipMemsetAsync(d_ycross_, 0, (nx + nz) * sizeof(double), s_comp_));
  const bool shear = rows == "shear";
  YCrossArgs a;
  walk_args(a, shear ? (1u | 2u | 4u | 8u | 32u) : (1u | 2u | 4u), false);
  a.nkz = p.nkz;
  a.rows = shear ? kYCrossShear : kYCrossVelocity;
  a.nref = static_cast<int>(nref);
  for (size_t i = 0; i < nref; ++i) a.yref[i] = refs[i];
  a.ckx = d_ycross_;
  a.ckz = d_ycross_ + nx;
  if (ms) HIP_CHECK(hipEventRecord(te[0], s_comp_));
  for_kblocks([&](size_t off, int cnt, int kx0) { ycross_accumulate(at_block(a, off, cnt, kx0), fp64_, s_comp_); });
  if (ms) HIP_CHECK(hipEventRecord(te[1], s_comp_));
  reduce_fetch(d_ycross_, nx + nz, h_ycross_);
  if (ms) {
    float t = 0;
    HIP_CHECK(hipEventElapsedTime(&t, te[0], te[1]));
    *ms = t;
    for (hipEvent_t e : te) (void)hipEventDestroy(e);
  }
  PlaneCrossSpectra out;
  out.rows = shear ? std::vector<std::string>{"u_wz", "v_wz", "w_wx", "wz_wz"} : std::vector<std::string>{"uu", "vv", "ww", "uv"};
  out.ref_planes = refs;
  out.nkx = nkx;
  out.nkz = nkz;
  out.ckx.reset(new double[2 * 4 * nref * NY * nkx]);
  out.ckz.reset(new double[2 * 4 * nref * NY * nkz]);
  // device rows [ref][2 q + (Re, Im)][y][k] -> complex [q][ref][y][k]: one (array, row, reference plane)
  // block per task, on a few threads (the pages of the result are touched here for the first time)
  const size_t tasks = 2 * 4 * nref;
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t t = next++; t < tasks; t = next++) {
      const bool z = t >= 4 * nref;
      const size_t q = (z ? t - 4 * nref : t) / nref, r = (z ? t - 4 * nref : t) % nref;
      const size_t plane = NY * (z ? nkz : nkx);
      const double* re = h_ycross_ + (z ? nx : 0) + (r * kYSpecRows + 2 * q) * plane;
      const double* im = re + plane;
      double* o = (z ? out.ckz.get() : out.ckx.get()) + 2 * (q * nref + r) * plane;
      for (size_t e = 0; e < plane; ++e) {
        o[2 * e] = re[e];
        o[2 * e + 1] = im[e];
      }
    }
  };
  std::vector<std::thread> pool;
  for (size_t t = 1; t < std::min<size_t>(8, tasks); ++t) pool.emplace_back(work);
  work();
  for (std::thread& t : pool) t.join();
  return out;
}

std::vector<double> Solver::plane_cross_spectra_timing(const std::vector<int>& refs, const std::string& rows) {
  std::vector<double> ms(2, 0.0);
  plane_cross_spectra(refs, rows, &ms[0]);
  plane_spectra(false, &ms[1]);
  return ms;
}

// <path>YCROSS_KX_<step>.npy (4, nref, NY, Kx+1) and <path>YCROSS_KZ_<step>.npy (4, nref, NY, nkz), complex128,
// and a sidecar <path>YCROSS_<step>.json; every rank takes part in the sums, rank 0 writes
void Solver::write_ycross_files() {
  const PlaneCrossSpectra cs = plane_cross_spectra(cfg_.ycross_plane_list(), cfg_.ycross_rows);
  if (plan_.rank != 0) return;
  const Plan& p = plan_;
  char step[16];
  std::snprintf(step, sizeof(step), "%08ld", nstep_);
  const size_t nref = cs.ref_planes.size();
  auto write = [&](const char* name, const double* v, int nk) {
    const std::string fn = cfg_.path + name + step + ".npy";
    std::ofstream f(fn, std::ios::binary | std::ios::trunc);
    CH_CHECK(f.good(), "cannot open '" << fn << "'");
    const std::string h = npy_header("<c16", "(4, " + std::to_string(nref) + ", " + std::to_string(p.NY) + ", " + std::to_string(nk) + ")");
    f.write(h.data(), static_cast<std::streamsize>(h.size()));
    f.write(reinterpret_cast<const char*>(v), static_cast<std::streamsize>(2 * 4 * nref * p.NY * static_cast<size_t>(nk) * sizeof(double)));
    f.close();
    CH_CHECK(!f.fail(), "writing '" << fn << "' failed");
  };
  write("YCROSS_KX_", cs.ckx.get(), p.Kx + 1);
  write("YCROSS_KZ_", cs.ckz.get(), p.nkz);
  std::ofstream js(cfg_.path + "YCROSS_" + step + ".json");
  js.precision(17);
  js << "{\"step\": " << nstep_ << ", \"time\": " << time() << ", \"rows\": [";
  for (size_t k = 0; k < cs.rows.size(); ++k) js << (k ? ", " : "") << "\"" << cs.rows[k] << "\"";
  js << "], \"row_set\": \"" << cfg_.ycross_rows << "\", \"ref_planes\": [";
  for (size_t k = 0; k < nref; ++k) js << (k ? ", " : "") << cs.ref_planes[k];
  js << "], \"ref_y\": [";
  for (size_t k = 0; k < nref; ++k) js << (k ? ", " : "") << grid_.y[cs.ref_planes[k]];
  js << "], \"ax\": " << p.ax << ", \"az\": " << p.az << ", \"y\": [";
  for (int j = 0; j < p.NY; ++j) js << (j ? ", " : "") << grid_.y[j];
  js << "], \"Re\": " << cfg_.Re << "}\n";
}

// ---- spectral Reynolds-stress budgets ------------------------------------------------------------
// The two halves of the pressure and of the static pressure with a stage of the reduction after each:
// rows 0..7 while d_pres_ holds H, rows 8..19 once it holds Pi (field 0) and p-hat' (field 1).  U' is the
// host's compact D1 of the mean profile.  Like the pressure it writes d_pres_, the step's scratch and
// its own sums only.
Solver::SpectralBudgets Solver::spectral_budgets(double* ms) {
  CH_CHECK(!comm_, "spectral_budgets: the pressure solve is single-rank (a solver without a communicator)");
  const Plan& p = plan_;
  const size_t nx = static_cast<size_t>(kSBudRows) * p.NY * (p.Kx + 1), nz = static_cast<size_t>(kSBudRows) * p.NY * p.nkz;
  const size_t N = static_cast<size_t>(p.NY);
  if (!d_sbud_) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_sbud_), (nx + nz + 2 * N) * sizeof(double)));
  if (!h_sbud_) HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_sbud_), (nx + nz) * sizeof(double), hipHostMallocDefault));
  if (!prepared_) prepare();
  SpectralBudgets out;
  out.rows = {"n_uu", "n_vv", "n_ww", "n_uv", "g_uu", "g_vv", "g_ww", "g_uv", "gs_uu", "gs_vv",
              "gs_ww", "gs_uv", "gu", "gv", "ps_uu", "ps_vv", "ps_ww", "ps_uv", "pu", "pv"};
  out.U = mean_profile();
  out.dU = d1_profile(grid_, out.U);
  std::vector<double> prof(out.U);
  prof.insert(prof.end(), out.dU.begin(), out.dU.end());
  HIP_CHECK(hipMemsetAsync(d_sbud_, 0, (nx + nz) * sizeof(double), s_comp_));
  HIP_CHECK(hipMemcpyAsync(d_sbud_ + nx + nz, prof.data(), 2 * N * sizeof(double), hipMemcpyHostToDevice, s_comp_));
  HIP_CHECK(hipStreamSynchronize(s_comp_));  // (prof is pageable and leaves scope)
  const size_t fsz = spec_ * esz_;
  auto stage = [&](int st) {
    SBudgetArgs a;
    walk_args(a, st == 0 ? 63u : (1u | 2u | 4u | 32u), st == 1);
    for (int c = 0; c < (st == 0 ? 3 : 1); ++c) a.h[c] = static_cast<const char*>(d_pres_) + c * fsz;
    a.U = d_sbud_ + nx + nz;
    a.dU = a.U + N;
    a.stage = st;
    a.nkz = p.nkz;
    a.ekx = d_sbud_;
    a.ekz = d_sbud_ + nx;
    for_kblocks([&](size_t off, int cnt, int kx0) {
      SBudgetArgs b = at_block(a, off, cnt, kx0);
      for (const void*& q : b.h)
        if (q) q = static_cast<const char*>(q) + off;
      sbudget_accumulate(b, fp64_, s_comp_);
    });
  };
  hipEvent_t te[4] = {nullptr, nullptr, nullptr, nullptr};
  if (ms)
    for (hipEvent_t& e : te) HIP_CHECK(hipEventCreate(&e));
  rotational_device();
  if (ms) HIP_CHECK(hipEventRecord(te[0], s_comp_));
  stage(0);
  if (ms) HIP_CHECK(hipEventRecord(te[1], s_comp_));
  poisson_device();
  static_return_device();
  if (ms) HIP_CHECK(hipEventRecord(te[2], s_comp_));
  stage(1);
  if (ms) HIP_CHECK(hipEventRecord(te[3], s_comp_));
  reduce_fetch(d_sbud_, nx + nz, h_sbud_);
  if (ms) {
    float t01 = 0, t23 = 0;
    HIP_CHECK(hipEventElapsedTime(&t01, te[0], te[1]));
    HIP_CHECK(hipEventElapsedTime(&t23, te[2], te[3]));
    ms[0] = t01;
    ms[1] = t23;
    for (hipEvent_t e : te) (void)hipEventDestroy(e);
  }
  out.ekx.assign(h_sbud_, h_sbud_ + nx);
  out.ekz.assign(h_sbud_ + nx, h_sbud_ + nx + nz);
  return out;
}

std::vector<double> Solver::spectral_budgets_timing() {
  std::vector<double> ms(2, 0.0);
  spectral_budgets(ms.data());
  return ms;
}

// <path>SBUD_KX_<step>.npy (20, NY, Kx+1) and <path>SBUD_KZ_<step>.npy (20, NY, nkz), float64, and a
// sidecar <path>SBUD_<step>.json with the mean profile and its derivative as the rows used them
void Solver::write_sbudget_files() {
  if (comm_) return note_once(sbud_note_, plan_.rank,
                              "[channel] sbudget_every: SBUD_KX_*.npy, SBUD_KZ_*.npy, SBUD_*.json skipped (the pressure solve is single-rank)\n");
  const SpectralBudgets sb = spectral_budgets();
  const Plan& p = plan_;
  char step[16];
  std::snprintf(step, sizeof(step), "%08ld", nstep_);
  write_rows_npy(cfg_.path + "SBUD_KX_" + step + ".npy", sb.ekx, kSBudRows, p.NY, p.Kx + 1);
  write_rows_npy(cfg_.path + "SBUD_KZ_" + step + ".npy", sb.ekz, kSBudRows, p.NY, p.nkz);
  std::ofstream js(cfg_.path + "SBUD_" + step + ".json");
  js.precision(17);
  js << "{\"step\": " << nstep_ << ", \"time\": " << time() << ", \"rows\": [";
  for (size_t k = 0; k < sb.rows.size(); ++k) js << (k ? ", " : "") << "\"" << sb.rows[k] << "\"";
  js << "], \"ax\": " << p.ax << ", \"az\": " << p.az;
  auto prof = [&](const char* key, const double* v) {
    js << ", \"" << key << "\": [";
    for (int j = 0; j < p.NY; ++j) js << (j ? ", " : "") << v[j];
    js << "]";
  };
  prof("y", grid_.y.data());
  prof("U", sb.U.data());
  prof("dU", sb.dU.data());
  js << ", \"Re\": " << cfg_.Re << "}\n";
}

// one line of NY values per call and file, as write_stats_files: the vorticity r.m.s., the
// dissipation 2 nu g of the uu, vv, ww, uv budgets and (one rank without a communicator) the triple
// products of the turbulent transport
void Solver::write_budget_files() {
  const std::vector<double> g = gradient_sums();
  std::vector<double> t;
  if (!comm_) t = transport_moments();
  else note_once(budget_note_, plan_.rank, "[channel] budget_every: TRIPLE_*.dat skipped (the physical-space export is single-rank)\n");
  if (plan_.rank != 0) return;
  const int N = plan_.NY;
  const double nu = 1.0 / cfg_.Re;
  const char* wn[3] = {"WXRMS.dat", "WYRMS.dat", "WZRMS.dat"};
  const char* en[4] = {"EPS_UU.dat", "EPS_VV.dat", "EPS_WW.dat", "EPS_UV.dat"};
  const char* tn[3] = {"TRIPLE_UUV.dat", "TRIPLE_WWV.dat", "TRIPLE_UVV.dat"};
  for (int q = 0; q < 3; ++q) append_profile(cfg_.path + wn[q], g.data() + q * N, N, 1.0, true);
  for (int q = 0; q < 4; ++q) append_profile(cfg_.path + en[q], g.data() + (3 + q) * N, N, 2.0 * nu);
  if (!t.empty())
    for (int q = 0; q < 3; ++q) append_profile(cfg_.path + tn[q], t.data() + q * N, N);
}

// One NumPy v1.0 file per field, <path>FIELD_<name>_<step>.npy of shape (nplanes, NX, Nzp) in the
// storage precision, and a sidecar <path>FIELDS_<step>.json
void Solver::write_field_files() {
  const Plan& p = plan_;
  const std::vector<int> planes = cfg_.fields_plane_list();
  const std::vector<std::string> names = cfg_.fields_list();
  std::vector<int> fidx;
  for (const std::string& nm : names) fidx.push_back(phys_field_index(nm));
  char step[16];
  std::snprintf(step, sizeof(step), "%08ld", nstep_);
  const size_t plane = static_cast<size_t>(p.NX) * p.Nzp, psz = plane * (fp64_ ? sizeof(double) : sizeof(float));
  const std::string head = npy_header(fp64_ ? "<f8" : "<f4", "(" + std::to_string(planes.size()) + ", " + std::to_string(p.NX) +
                                                                 ", " + std::to_string(p.Nzp) + ")");
  std::vector<std::ofstream> files;
  for (const std::string& nm : names) {
    files.emplace_back(cfg_.path + "FIELD_" + nm + "_" + step + ".npy", std::ios::binary | std::ios::trunc);
    std::ofstream& f = files.back();
    CH_CHECK(f.good(), "cannot open field file for '" << nm << "' under '" << cfg_.path << "'");
    f.write(head.data(), static_cast<std::streamsize>(head.size()));
  }
  const std::streamoff data0 = static_cast<std::streamoff>(head.size());
  const auto pos = plane_positions(planes, p.NY);
  std::vector<char> pbuf;
  export_fields(planes, fidx, [&](size_t k, int y, const char* src) {
    if (fidx[k] == kPresField) {
      pbuf.assign(src, src + psz);
      if (fp64_) subtract_mean(reinterpret_cast<double*>(pbuf.data()), plane);
      else subtract_mean(reinterpret_cast<float*>(pbuf.data()), plane);
      src = pbuf.data();
    }
    for (size_t i : pos[y]) {
      files[k].seekp(data0 + static_cast<std::streamoff>(i * psz));
      files[k].write(src, static_cast<std::streamsize>(psz));
    }
  });
  for (size_t k = 0; k < names.size(); ++k) {
    files[k].close();
    CH_CHECK(!files[k].fail(), "writing the field file of '" << names[k] << "' failed");
  }
  std::ofstream js(cfg_.path + "FIELDS_" + step + ".json");
  js.precision(17);
  js << "{\"step\": " << nstep_ << ", \"time\": " << time() << ", \"planes\": [";
  for (size_t i = 0; i < planes.size(); ++i) js << (i ? ", " : "") << planes[i];
  js << "], \"y\": [";
  for (size_t i = 0; i < planes.size(); ++i) js << (i ? ", " : "") << grid_.y[planes[i]];
  js << "], \"fields\": [";
  for (size_t k = 0; k < names.size(); ++k) js << (k ? ", " : "") << "\"" << names[k] << "\"";
  js << "], \"NX\": " << p.NX << ", \"Nzp\": " << p.Nzp << ", \"LX\": " << cfg_.LX << ", \"LZ\": " << cfg_.LZ << "}\n";
}

// skewness m3 / m2^1.5 and flatness m4 / m2^2 of u, v, w per plane (0 where m2 = 0: the walls), one
// line of NY values per call, as write_stats_files
void Solver::write_moment_files(const std::vector<double>& m) {
  const int N = plan_.NY;
  auto app = [&](const char* name) { return std::ofstream(cfg_.path + name, std::ios::app); };
  const char* sk[3] = {"USKEW.dat", "VSKEW.dat", "WSKEW.dat"};
  const char* fl[3] = {"UFLAT.dat", "VFLAT.dat", "WFLAT.dat"};
  const int r2[3] = {1, 2, 3}, r3[3] = {5, 6, 7}, r4[3] = {8, 9, 10};
  for (int q = 0; q < 3; ++q) {
    auto fs = app(sk[q]);
    auto ff = app(fl[q]);
    for (int j = 0; j < N; ++j) {
      const double m2 = m[r2[q] * N + j];
      const double d3 = m2 > 0 ? m2 * std::sqrt(m2) : 0.0, d4 = m2 * m2;  // (either may underflow to 0)
      fs << " " << std::fixed << (d3 > 0 ? m[r3[q] * N + j] / d3 : 0.0);
      ff << " " << std::fixed << (d4 > 0 ? m[r4[q] * N + j] / d4 : 0.0);
    }
    fs << " \n";
    ff << " \n";
  }
}

}  // namespace channel
