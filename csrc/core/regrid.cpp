// Restart onto another grid: the host tables (regrid.hpp) and the solver's two entry points, a pair of
// restart files on any grid of the same box (read_restart_regrid) and a global state in memory
// (regrid_state).  Both stage source lines in the files' line-major order, upload them in batches of
// whole kx planes and let regrid_launch (kernels/regrid.hip) interpolate, transpose and round them into
// the device layout; no state-sized host array is built.
#include "channel/regrid.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "channel/common.hpp"
#include "channel/io.hpp"
#include "channel/solver.hpp"

namespace channel {

int RegridTable::max_window() const { return winlen.empty() ? 0 : *std::max_element(winlen.begin(), winlen.end()); }

RegridTable regrid_table(int NY_s, double s_s, int NY_d, double s_d) {
  CH_CHECK(NY_s >= 5 && NY_d >= 5 && s_s > 0 && s_d > 0, "regrid_table: NY >= 5 and stretch > 0 on both grids");
  const std::vector<double> ys = YGrid::build(NY_s, s_s).y, yd = YGrid::build(NY_d, s_d).y;
  RegridTable t;
  t.NY_s = NY_s;
  t.NY_d = NY_d;
  const int W = t.W = std::min(kRegridWidth, NY_s);
  t.j0.assign(NY_d, 0);
  t.unit.assign(NY_d, -1);
  t.w.assign(static_cast<size_t>(NY_d) * W, 0.0);
  for (int j = 0; j < NY_d; ++j) {
    const double y = yd[j];
    // y in [ys[m], ys[m + 1]) (the last interval is closed)
    int m = static_cast<int>(std::upper_bound(ys.begin(), ys.end(), y) - ys.begin()) - 1;
    m = std::min(std::max(m, 0), NY_s - 2);
    const int s0 = t.j0[j] = std::min(std::max(m - (W / 2 - 1), 0), NY_s - W);
    double* w = &t.w[static_cast<size_t>(j) * W];
    for (int a = 0; a < W; ++a)
      if (std::fabs(y - ys[s0 + a]) <= kRegridSnap) t.unit[j] = a;
    if (t.unit[j] >= 0) {
      w[t.unit[j]] = 1.0;
      continue;
    }
    for (int a = 0; a < W; ++a) {
      double num = 1.0, den = 1.0;
      for (int b = 0; b < W; ++b) {
        if (b == a) continue;
        num *= y - ys[s0 + b];
        den *= ys[s0 + a] - ys[s0 + b];
      }
      w[a] = num / den;
    }
  }
  const int chunks = (NY_d + kRegridChunk - 1) / kRegridChunk;
  t.win0.assign(chunks, 0);
  t.winlen.assign(chunks, 0);
  for (int c = 0; c < chunks; ++c) {
    int lo = NY_s, hi = 0;
    for (int j = c * kRegridChunk; j < std::min(NY_d, (c + 1) * kRegridChunk); ++j) {
      lo = std::min(lo, t.j0[j]);
      hi = std::max(hi, t.j0[j] + W);
    }
    t.win0[c] = lo;
    t.winlen[c] = hi - lo;
  }
  return t;
}

RegridModeMap regrid_mode_map(int NX_s, int NZ_s, int NX_d, int NZ_d, int kx0, int nkx_loc) {
  CH_CHECK(NX_s >= 1 && NZ_s >= 2 && NX_d >= 1 && NZ_d >= 2, "regrid_mode_map: bad grid");
  const int Kx_s = NX_s / 3, Kx_d = NX_d / 3, nkx_d = 2 * Kx_d + 1;
  CH_CHECK(kx0 >= 0 && nkx_loc >= 0 && kx0 + nkx_loc <= nkx_d, "regrid_mode_map: kx range outside the " << nkx_d << " retained kx");
  RegridModeMap m;
  m.plane.assign(nkx_loc, -1);
  for (int i = 0; i < nkx_loc; ++i) {
    const int ig = kx0 + i, k = ig <= Kx_d ? ig : ig - nkx_d;
    if (std::abs(k) <= Kx_s) m.plane[i] = k >= 0 ? k : NX_s + k;
  }
  m.nkz_take = std::min((2 * NZ_s - 2) / 3, (2 * NZ_d - 2) / 3) + 1;
  return m;
}

namespace {

// device copy of a host array, freed on scope exit
template <typename T>
struct DevArray {
  T* d = nullptr;
  DevArray() = default;
  explicit DevArray(size_t n) { HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d), std::max<size_t>(n, 1) * sizeof(T))); }
  explicit DevArray(const std::vector<T>& h) : DevArray(h.size()) {
    if (!h.empty()) HIP_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  DevArray(const DevArray&) = delete;
  DevArray& operator=(const DevArray&) = delete;
  ~DevArray() {
    if (d) (void)hipFree(d);
  }
};

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// U on the target grid from a source profile in units of n2, with the lines' arithmetic
std::vector<double> interp_profile(const RegridTable& t, const std::vector<double>& Us, double n2) {
  std::vector<double> U(t.NY_d);
  for (int j = 0; j < t.NY_d; ++j) {
    const double* f = &Us[t.j0[j]];
    double v = 0.0;
    if (t.unit[j] >= 0) {
      v = f[t.unit[j]];
    } else {
      for (int m = 0; m < t.W; ++m) v += t.w[static_cast<size_t>(j) * t.W + m] * f[m];
    }
    U[j] = v / n2;
  }
  return U;
}

}  // namespace

// Staged host bytes per batch of source planes; CHANNEL_REGRID_BUDGET_MB overrides it (tests run
// several batches on small grids with 0: one plane per batch)
static size_t regrid_budget_bytes() {
  if (const char* e = std::getenv("CHANNEL_REGRID_BUDGET_MB")) return static_cast<size_t>(std::max(0.0, std::atof(e)) * (1 << 20));
  return static_cast<size_t>(512) << 20;
}

void Solver::regrid_apply(const RegridSource& S) {
  const Plan& p = plan_;
  const auto t_begin = std::chrono::steady_clock::now();
  const RegridTable T = regrid_table(S.NY, S.stretch, p.NY, cfg_.stretch);
  const RegridModeMap M = regrid_mode_map(S.NX, S.NZ, p.NX, p.NZ, p.kx0, p.nkx_loc);
  const int ncol = std::min(std::max(M.nkz_take - p.kz0, 0), p.nkz_loc);  // local kz lines with a source
  const int maxwin = T.max_window();
  CH_CHECK(static_cast<size_t>(kSpecKzBlock) * (maxwin | 1) * 16 <= static_cast<size_t>(kRegridLdsBytes),
           "regrid: NY " << S.NY << " -> " << p.NY << " reads up to " << maxwin << " source rows per " << kRegridChunk
                         << " target planes, more than the kernel's " << kRegridLdsBytes << " B of LDS hold for 8 lines");
  for (size_t c = 0; c < T.win0.size(); ++c)
    CH_CHECK(T.win0[c] >= 0 && T.winlen[c] >= T.W && T.win0[c] + T.winlen[c] <= S.NY, "regrid: window outside the source grid");
  std::vector<int> win(2 * T.win0.size());
  for (size_t c = 0; c < T.win0.size(); ++c) {
    win[2 * c] = T.win0[c];
    win[2 * c + 1] = T.winlen[c];
  }
  std::vector<int> src_i;  // local target kx with a source plane
  for (int i = 0; i < p.nkx_loc; ++i)
    if (M.plane[i] >= 0) src_i.push_back(i);
  regrid_ms_.assign(4, 0.0);

  HIP_CHECK(hipStreamSynchronize(s_comp_));
  HIP_CHECK(hipMemsetAsync(field_ptr(PHI), 0, spec_ * esz_, s_comp_));
  HIP_CHECK(hipMemsetAsync(field_ptr(OMEGA), 0, spec_ * esz_, s_comp_));
  HIP_CHECK(hipMemsetAsync(field_ptr(RPHI), 0, 2 * spec_ * esz_, s_comp_));
  if (ncol > 0 && !src_i.empty()) {
    const DevArray<int> d_j0(T.j0), d_unit(T.unit), d_win(win);
    const DevArray<double> d_w(T.w), d_U(S.U);
    const size_t line_bytes = static_cast<size_t>(S.NY) * 16;
    const size_t nb_max = std::max<size_t>(1, regrid_budget_bytes() / (S.plane_lines * line_bytes));
    const int nb = static_cast<int>(std::min(nb_max, src_i.size()));
    const DevArray<double> d_stage(static_cast<size_t>(nb) * ncol * S.NY * 2);
    const DevArray<int> d_slot(p.nkx_loc);
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    std::vector<double> host;
    std::vector<int> slot(p.nkx_loc), batch;
    for (int field : {static_cast<int>(OMEGA), static_cast<int>(PHI)}) {
      for (size_t b0 = 0; b0 < src_i.size(); b0 += nb) {
        batch.assign(src_i.begin() + b0, src_i.begin() + std::min(src_i.size(), b0 + nb));
        auto t0 = std::chrono::steady_clock::now();
        S.fill(field == PHI ? 0 : 1, batch, host);
        CH_CHECK(host.size() == batch.size() * S.plane_lines * S.NY * 2, "regrid: staged batch has the wrong size");
        regrid_ms_[0] += 1e3 * seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        // the local kz lines with a source are one contiguous piece of every plane
        HIP_CHECK(hipMemcpy2D(d_stage.d, ncol * line_bytes, host.data() + static_cast<size_t>(S.line0) * S.NY * 2,
                              S.plane_lines * line_bytes, ncol * line_bytes, batch.size(), hipMemcpyHostToDevice));
        std::fill(slot.begin(), slot.end(), -1);
        for (size_t k = 0; k < batch.size(); ++k) slot[batch[k]] = static_cast<int>(k);
        HIP_CHECK(hipMemcpy(d_slot.d, slot.data(), slot.size() * sizeof(int), hipMemcpyHostToDevice));
        regrid_ms_[1] += 1e3 * seconds_since(t0);
        HIP_CHECK(hipEventRecord(e0, s_comp_));
        for (int kb = 0; kb < nkb_; ++kb) {
          // the batch's kx of sub-block kb
          const int lo = std::max(batch.front(), kb_start_[kb]), hi = std::min(batch.back() + 1, kb_start_[kb] + kb_cnt_[kb]);
          if (lo >= hi) continue;
          RegridArgs a;
          a.src = d_stage.d;
          a.slot = d_slot.d + lo;
          a.nkx = hi - lo;
          a.ikx0 = lo - kb_start_[kb];
          a.scols = a.ncol = ncol;
          a.NY_s = S.NY;
          a.NY_d = p.NY;
          a.W = T.W;
          a.j0 = d_j0.d;
          a.unit = d_unit.d;
          a.w = d_w.d;
          a.win = d_win.d;
          a.max_window = maxwin;
          a.n2 = S.n2;
          a.dst = static_cast<char*>(field_ptr(field)) + kb_off_[kb] * esz_;
          a.nkx_blk = kb_cnt_[kb];
          a.nkzs = nkzs_;
          a.kzb = kzb_;
          if (field == OMEGA && p.owns_mean() && kb == 0) {  // line (0, 0) of the omega field holds U(y)
            a.U = d_U.d;
            a.u_ikx = 0;
          }
          a.lds_poison = lds_poison_enabled() ? 1 : 0;
          regrid_launch(a, fp64_, s_comp_);
        }
        HIP_CHECK(hipEventRecord(e1, s_comp_));
        HIP_CHECK(hipStreamSynchronize(s_comp_));  // the staging buffer is reused by the next batch
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        regrid_ms_[2] += ms;
      }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  HIP_CHECK(hipStreamSynchronize(s_comp_));
  prepared_ = false;
  regrid_ms_[3] = 1e3 * seconds_since(t_begin);
}

void Solver::read_restart_regrid(const std::string& g, const std::string& ddv, const std::string& umean, double src_stretch) {
  const Plan& p = plan_;
  int dims[3], dims2[3];
  std::vector<double> none;
  h5_read_planes(g, {}, none, dims);
  h5_read_planes(ddv, {}, none, dims2);
  CH_CHECK(dims[0] == dims2[0] && dims[1] == dims2[1] && dims[2] == dims2[2],
           "restart files " << g << " and " << ddv << " are on different grids");
  CH_CHECK(dims[0] >= 1 && dims[1] >= 5 && dims[2] >= 4 && dims[2] % 2 == 0,
           "restart file " << g << " has dims " << dims[0] << "x" << dims[1] << "x" << dims[2]);
  RegridSource S;
  S.NX = dims[0];
  S.NY = dims[1];
  S.NZ = dims[2] / 2;
  S.n2 = static_cast<double>(S.NX) * (2 * S.NZ - 2);
  auto attrs = h5_read_attrs(g);
  // the box is not regridded
  for (const char* k : {"LX", "LZ"}) {
    if (!attrs.count(k)) continue;
    const double have = attrs[k], want = std::string(k) == "LX" ? cfg_.LX : cfg_.LZ;
    std::ostringstream hs, ws;
    hs.precision(17);
    ws.precision(17);
    hs << have;
    ws << want;
    CH_CHECK(std::fabs(have - want) <= 1e-12 * std::fabs(want), "restart file " << g << " has " << k << " = " << hs.str()
                                                                                << ", the config has " << k << " = " << ws.str()
                                                                                << " (regrid keeps the box)");
  }
  if (src_stretch > 0) {
    S.stretch = src_stretch;
  } else if (attrs.count("stretch")) {
    S.stretch = attrs["stretch"];
  } else {
    S.stretch = cfg_.stretch;
    if (p.rank == 0)
      std::cerr << "[channel] read_restart: " << g << " carries no stretch; taking the config's stretch = " << cfg_.stretch << "\n";
  }
  CH_CHECK(S.stretch > 0, "restart file " << g << ": stretch must be positive");
  const RegridTable T = regrid_table(S.NY, S.stretch, p.NY, cfg_.stretch);
  // U(y): the named UMEAN file, else the full-precision copy inside G, else the parabola (on the target grid)
  std::vector<double> u64, Us;
  const bool in_g = h5_read_vector(g, "umean", u64) && static_cast<int>(u64.size()) == S.NY;
  if (!umean.empty() && umean != "-") {
    {
      std::ifstream f(umean, std::ios::binary | std::ios::ate);
      CH_CHECK(f.good(), "cannot read " << umean);
      const long long bytes = static_cast<long long>(f.tellg());
      CH_CHECK(bytes == 8LL * S.NY, "UMEAN file " << umean << " holds " << bytes / 8 << " records, the restart file " << g
                                                  << " has NY = " << S.NY);
    }
    Us = umean_read(umean, S.NY);
    // the companion of G (the same profile rounded to float32): G's full-precision copy, as read_restart does
    bool companion = in_g;
    for (int j = 0; companion && j < S.NY; ++j) companion = static_cast<float>(u64[j]) == static_cast<float>(Us[j]);
    if (companion) {
      Us = u64;
    } else if (p.rank == 0 && !u64.empty()) {
      std::cerr << "[channel] read_restart: U(y) from " << umean << " (differs from the 'umean' stored in " << g
                << ", which is ignored)\n";
    }
  } else if (in_g) {
    Us = u64;
  }
  if (!Us.empty()) {
    S.U = interp_profile(T, Us, S.n2);
  } else {
    S.U.resize(p.NY);
    for (int j = 0; j < p.NY; ++j) S.U[j] = 0.75 * cfg_.Q * (1.0 - grid_.y[j] * grid_.y[j]);
  }
  const RegridModeMap M = regrid_mode_map(S.NX, S.NZ, p.NX, p.NZ, p.kx0, p.nkx_loc);
  S.plane_lines = S.NZ;
  S.line0 = p.kz0;
  S.fill = [&](int field, const std::vector<int>& ikx, std::vector<double>& host) {
    std::vector<int> planes(ikx.size());
    for (size_t k = 0; k < ikx.size(); ++k) planes[k] = M.plane[ikx[k]];
    int d[3];
    h5_read_planes(field == 0 ? ddv : g, planes, host, d);
  };
  regrid_apply(S);
  const bool same_grid = S.NX == p.NX && S.NY == p.NY && S.NZ == p.NZ && S.stretch == cfg_.stretch;
  const double t = attrs.count("time") ? attrs["time"] : 0.0, dt = attrs.count("dt") ? attrs["dt"] : 0.0;
  set_time(t, same_grid ? dt : 0.0);  // another grid: the device time-step control finds its own first dt
  nstep_ = attrs.count("step") ? static_cast<long>(attrs["step"]) : 0;
}

void Solver::regrid_state(const std::complex<double>* phi_s, const std::complex<double>* om_s, const double* U_s, int NX_s,
                          int NY_s, int NZ_s, double stretch_s) {
  const Plan& p = plan_;
  CH_CHECK(NX_s >= 3 && NY_s >= 5 && NZ_s >= 2 && stretch_s > 0, "regrid_state: bad source grid");
  CH_CHECK(phi_s && om_s, "regrid_state: phi and omega are required");
  const int nkx_s = 2 * (NX_s / 3) + 1, nkz_s = (2 * NZ_s - 2) / 3 + 1;
  RegridSource S;
  S.NX = NX_s;
  S.NY = NY_s;
  S.NZ = NZ_s;
  S.stretch = stretch_s;
  S.n2 = 1.0;
  const RegridTable T = regrid_table(NY_s, stretch_s, p.NY, cfg_.stretch);
  S.U = interp_profile(T, U_s ? std::vector<double>(U_s, U_s + NY_s) : std::vector<double>(NY_s, 0.0), 1.0);
  const RegridModeMap M = regrid_mode_map(NX_s, NZ_s, p.NX, p.NZ, p.kx0, p.nkx_loc);
  const int ncol = std::min(std::max(M.nkz_take - p.kz0, 0), p.nkz_loc);
  S.plane_lines = std::max(ncol, 1);
  S.line0 = 0;
  // canonical [y][kx][kz] -> the files' line-major order, this rank's lines only
  S.fill = [&](int field, const std::vector<int>& ikx, std::vector<double>& host) {
    const std::complex<double>* f = field == 0 ? phi_s : om_s;
    host.assign(ikx.size() * S.plane_lines * NY_s * 2, 0.0);
    for (size_t k = 0; k < ikx.size(); ++k) {
      const int kx = p.kx_of(p.kx0 + ikx[k]), is = kx >= 0 ? kx : nkx_s + kx;
      for (int c = 0; c < ncol; ++c)
        for (int y = 0; y < NY_s; ++y) {
          const std::complex<double> v = f[(static_cast<size_t>(y) * nkx_s + is) * nkz_s + p.kz0 + c];
          const size_t o = ((k * S.plane_lines + c) * NY_s + y) * 2;
          host[o] = v.real();
          host[o + 1] = v.imag();
        }
    }
  };
  regrid_apply(S);
}

}  // namespace channel
