// Torch-free Python bindings of the native core (channel_gpu_amd._core).
//
// Config, grid, plan, Solver, I/O, bootstrap and communicator entry points, built with pybind11
// only (no libtorch): a process that imports just this module runs on the ROCm runtime and RCCL
// of /opt/rocm, exactly like the C++ driver binary.  bench.py and the Python driver use it that
// way; the torch extension (_C, bindings.cpp) re-exports everything here and adds the tensor
// kernel entry points used by the tests.
#include <pybind11/complex.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <complex>
#include <map>
#include <memory>

#include "channel/bootstrap.hpp"
#include "channel/comm.hpp"
#include "channel/common.hpp"
#include "channel/config.hpp"
#include "channel/grid.hpp"
#include "channel/io.hpp"
#include "channel/kernels.hpp"
#include "channel/plan.hpp"
#include "channel/regrid.hpp"
#include "channel/solver.hpp"

namespace py = pybind11;
using namespace channel;

namespace {

py::array_t<double> vec(const std::vector<double>& v) {
  py::array_t<double> a(v.size());
  std::copy(v.begin(), v.end(), a.mutable_data());
  return a;
}

// a per-plane diagnostic of the solver (the call without the GIL) as a (rows, NY) array
py::array_t<double> profile_rows(Solver& s, std::vector<double> (Solver::*call)(), int rows) {
  std::vector<double> v;
  {
    py::gil_scoped_release r;
    v = (s.*call)();
  }
  py::array_t<double> a({static_cast<py::ssize_t>(rows), static_cast<py::ssize_t>(s.plan().NY)});
  std::copy(v.begin(), v.end(), a.mutable_data());
  return a;
}

// a canonical spectral field of the solver (the call without the GIL) as a (NY, nkx_loc, nkz_loc) array
py::array_t<std::complex<double>> canonical_field(Solver& s, std::vector<std::complex<double>> (Solver::*call)()) {
  std::vector<std::complex<double>> v;
  {
    py::gil_scoped_release r;
    v = (s.*call)();
  }
  const Plan& p = s.plan();
  py::array_t<std::complex<double>> a({static_cast<py::ssize_t>(p.NY), static_cast<py::ssize_t>(p.nkx_loc),
                                       static_cast<py::ssize_t>(p.nkz_loc)});
  std::copy(v.begin(), v.end(), a.mutable_data());
  return a;
}

py::bytes new_uid() { return py::bytes(Comm::new_unique_id()); }

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // namespace

PYBIND11_MODULE(_core, m) {
  m.doc() = "channel_gpu_amd native core, torch-free bindings (gfx950 HIP kernels, RCCL, HDF5 I/O)";
  py::register_exception<channel::Error>(m, "ChannelError", PyExc_RuntimeError);
  py::class_<Config>(m, "Config")
      .def(py::init<>())
      .def_static("from_file", &Config::from_file, py::arg("path"), py::arg("overrides") = std::vector<std::string>())
      .def_static("from_string",
                  [](const std::string& text, const std::vector<std::string>& overrides) {
                    ConfigTree t = ConfigTree::parse_string(text);
                    for (const auto& o : overrides) {
                      auto eq = o.find('=');
                      CH_CHECK(eq != std::string::npos, "override must be key=value");
                      std::string k = o.substr(0, eq);
                      if (t.has("application." + k)) k = "application." + k;
                      t.set(k, o.substr(eq + 1));
                    }
                    return Config::from_tree(t);
                  },
                  py::arg("text"), py::arg("overrides") = std::vector<std::string>())
      .def("to_string", &Config::to_string)
      .def("validate", &Config::validate)
      .def_property_readonly("nzp", &Config::nzp)
#define RW(f) .def_readwrite(#f, &Config::f)
      RW(NX) RW(NY) RW(NZ) RW(in_G) RW(in_DDV) RW(in_UMEAN) RW(out_G) RW(out_DDV) RW(out_UMEAN) RW(path) RW(Re) RW(Q)
      RW(LX) RW(LZ) RW(stretch) RW(nsteps) RW(t_end) RW(cfl) RW(dt_fixed) RW(dt_max) RW(cfl_mode) RW(stats_every)
      RW(symmetry_every) RW(checkpoint_every) RW(log_every) RW(precision) RW(decomposition) RW(pr) RW(pc) RW(seed)
      RW(ic) RW(ic_amplitude) RW(forcing) RW(influence) RW(explicit_d2) RW(checkpoint_async) RW(health_check) RW(health_every) RW(on_nan) RW(snapshot_every)
      RW(max_rollbacks) RW(rollback_cfl_factor) RW(spectra_every) RW(spectra_planes) RW(log_json)
      RW(fields_every) RW(fields_planes) RW(fields) RW(moments_every) RW(budget_every) RW(pressure_every)
      RW(pstrain_every) RW(yspectra_every) RW(yspectra_pressure) RW(sbudget_every)
      RW(ycross_every) RW(ycross_planes) RW(ycross_rows)
      RW(pdf_every) RW(pdf_planes) RW(pdf_bins) RW(pdf_joint_bins) RW(pdf_span) RW(pdf_vorticity)
      RW(regrid) RW(regrid_stretch)
      RW(scalar) RW(Pr) RW(scalar_lower) RW(scalar_upper) RW(scalar_source) RW(scalar_ic) RW(in_T) RW(out_T) RW(scalar_every);
#undef RW

  m.def("parse_config_tree", [](const std::string& text) { return ConfigTree::parse_string(text).items(); });

  py::class_<YGrid>(m, "YGrid")
      .def_static("build", &YGrid::build, py::arg("N"), py::arg("stretch") = 2.0)
      .def_readonly("N", &YGrid::N)
      .def_property_readonly("y", [](const YGrid& g) { return vec(g.y); })
      .def_property_readonly("d1_lo", [](const YGrid& g) { return vec(g.d1_lo); })
      .def_property_readonly("d1_up", [](const YGrid& g) { return vec(g.d1_up); })
      .def_property_readonly("d1_rm", [](const YGrid& g) { return vec(g.d1_rm); })
      .def_property_readonly("d1_rc", [](const YGrid& g) { return vec(g.d1_rc); })
      .def_property_readonly("d1_rp", [](const YGrid& g) { return vec(g.d1_rp); })
      .def_property_readonly("d1_w0", [](const YGrid& g) { return std::vector<double>(g.d1_w0, g.d1_w0 + 3); })
      .def_property_readonly("d1_wN", [](const YGrid& g) { return std::vector<double>(g.d1_wN, g.d1_wN + 3); })
      .def_property_readonly("m_lo", [](const YGrid& g) { return vec(g.m_lo); })
      .def_property_readonly("m_up", [](const YGrid& g) { return vec(g.m_up); })
      .def_property_readonly("k_lo", [](const YGrid& g) { return vec(g.k_lo); })
      .def_property_readonly("k_c", [](const YGrid& g) { return vec(g.k_c); })
      .def_property_readonly("k_up", [](const YGrid& g) { return vec(g.k_up); })
      .def_property_readonly("trap", [](const YGrid& g) { return vec(g.trap); })
      .def_property_readonly("d2_w0", [](const YGrid& g) { return std::vector<double>(g.d2_w0, g.d2_w0 + 3); })
      .def_property_readonly("d2_wN", [](const YGrid& g) { return std::vector<double>(g.d2_wN, g.d2_wN + 3); })
      .def_readonly("d2_w0_up", &YGrid::d2_w0_up)
      .def_readonly("d2_wN_lo", &YGrid::d2_wN_lo);

  // regridding tables (regrid.hpp), bound like YGrid.build so the CPU tests reach them
  py::class_<RegridTable>(m, "RegridTable")
      .def_readonly("NY_s", &RegridTable::NY_s)
      .def_readonly("NY_d", &RegridTable::NY_d)
      .def_readonly("W", &RegridTable::W)
      .def_property_readonly("j0", [](const RegridTable& t) { return py::array_t<int>(t.j0.size(), t.j0.data()); })
      .def_property_readonly("unit", [](const RegridTable& t) { return py::array_t<int>(t.unit.size(), t.unit.data()); })
      .def_property_readonly("w",
                             [](const RegridTable& t) {
                               py::array_t<double> a({static_cast<py::ssize_t>(t.NY_d), static_cast<py::ssize_t>(t.W)});
                               std::copy(t.w.begin(), t.w.end(), a.mutable_data());
                               return a;
                             })
      .def_property_readonly("win0", [](const RegridTable& t) { return py::array_t<int>(t.win0.size(), t.win0.data()); })
      .def_property_readonly("winlen", [](const RegridTable& t) { return py::array_t<int>(t.winlen.size(), t.winlen.data()); })
      .def("max_window", &RegridTable::max_window);
  m.def("regrid_table", &regrid_table, py::arg("NY_s"), py::arg("stretch_s"), py::arg("NY_d"), py::arg("stretch_d"));
  m.def("regrid_mode_map",
        [](int NX_s, int NZ_s, int NX_d, int NZ_d, int kx0, int nkx_loc) {
          const RegridModeMap mm = regrid_mode_map(NX_s, NZ_s, NX_d, NZ_d, kx0, nkx_loc);
          return py::make_tuple(py::array_t<int>(mm.plane.size(), mm.plane.data()), mm.nkz_take);
        },
        py::arg("NX_s"), py::arg("NZ_s"), py::arg("NX_d"), py::arg("NZ_d"), py::arg("kx0"), py::arg("nkx_loc"),
        "(source plane of every local target kx or -1, count of kz columns taken)");
  m.attr("regrid_lds_bytes") = kRegridLdsBytes;

  py::class_<Split>(m, "Split")
      .def_static("balanced", &Split::balanced)
      .def_readonly("start", &Split::start)
      .def_readonly("count", &Split::count)
      .def("owner", &Split::owner);

  py::class_<Plan>(m, "Plan")
      .def_static("make", &Plan::make)
#define RO(f) .def_readonly(#f, &Plan::f)
      RO(NX) RO(NY) RO(NZ) RO(Nzp) RO(Kx) RO(nkx) RO(Kz) RO(nkz) RO(P) RO(rank) RO(kx_split) RO(y_split) RO(nkx_loc)
      RO(kx0) RO(ny_loc) RO(y0) RO(R) RO(ax) RO(az) RO(Pr) RO(Pc) RO(prow) RO(pcol) RO(kz_split) RO(x_split)
      RO(nkz_loc) RO(kz0) RO(nx_loc) RO(x0)
#undef RO
      .def("lines_loc", &Plan::lines_loc)
      .def("pencil", &Plan::pencil)
      .def("owns_mean", &Plan::owns_mean)
      .def("kx_of", &Plan::kx_of)
      .def("kx_fft_pos", &Plan::kx_fft_pos);

  m.def("yline_supported_R", &yline_supported_R);
  m.def("kspec_last_variant", [] { return kspec_last_variant(); },
        "kernel name(s) and template arguments of this thread's last K-SPEC launch (rocprofv3 kernel-name form)");


  m.def("new_unique_id", &new_uid);
  m.def("hdf5_available", &hdf5_available);
  m.def("set_debug_sync", &set_debug_sync);
  m.def("set_lds_poison", &set_lds_poison);
  m.def("lds_poison_enabled", &lds_poison_enabled);
  m.def("install_crash_handler", &install_crash_handler, "native backtrace on fatal signals (stderr)");
  m.def("h5_create_field", &h5_create_field, py::arg("path"), py::arg("NX"), py::arg("NY"), py::arg("NZ"),
        py::arg("fp64") = false, py::arg("Kx") = -1);
  m.def("h5_write_planes", &h5_write_planes);
  m.def("h5_read_planes", [](const std::string& p, const std::vector<int>& planes) {
    std::vector<double> d;
    int dims[3];
    h5_read_planes(p, planes, d, dims);
    return std::make_pair(vec(d), std::vector<int>(dims, dims + 3));
  });
  m.def("h5_write_attrs", &h5_write_attrs);
  m.def("h5_write_vector", &h5_write_vector);
  m.def("h5_read_vector", [](const std::string& p, const std::string& name) {
    std::vector<double> v;
    const bool ok = h5_read_vector(p, name, v);
    return py::make_tuple(ok, vec(v));
  });
  m.def("h5_read_attrs", &h5_read_attrs);
  m.def("umean_write", &umean_write);
  m.def("umean_read", &umean_read);

  py::class_<StepLog>(m, "StepLog")
#define LG(f) .def_readonly(#f, &StepLog::f)
      LG(step) LG(time) LG(dt) LG(dt_c) LG(dt_v) LG(umax) LG(vmax) LG(wmax) LG(cflsum) LG(dUdy_lo) LG(dUdy_hi) LG(flux)
      LG(dpdx) LG(utau_lo) LG(utau_hi) LG(utau) LG(health);
#undef LG

  py::class_<Solver>(m, "Solver")
      .def(py::init([](const Config& cfg, int rank, int nranks, int device, py::bytes uid) {
             return std::make_unique<Solver>(cfg, rank, nranks, device, std::string(uid));
           }),
           py::arg("cfg"), py::arg("rank") = 0, py::arg("nranks") = 1, py::arg("device") = 0,
           py::arg("uid") = py::bytes(""))
      .def_property_readonly("plan", &Solver::plan, py::return_value_policy::reference_internal)
      .def_property_readonly("grid", &Solver::grid, py::return_value_policy::reference_internal)
      .def_property_readonly("config", &Solver::config, py::return_value_policy::reference_internal)
      .def("set_state",
           [](Solver& s, py::array_t<std::complex<double>, py::array::c_style | py::array::forcecast> phi,
              py::array_t<std::complex<double>, py::array::c_style | py::array::forcecast> om,
              py::array_t<double, py::array::c_style | py::array::forcecast> U) {
             const size_t n = s.plan().spec_elems();
             CH_CHECK(static_cast<size_t>(phi.size()) == n && static_cast<size_t>(om.size()) == n,
                         "state arrays must have NY*nkx_loc*nkz_loc elements");
             CH_CHECK(U.size() == s.plan().NY, "U must have NY elements");
             py::gil_scoped_release r;
             s.set_state(phi.data(), om.data(), U.data());
           })
      .def("get_state",
           [](Solver& s) {
             const Plan& p = s.plan();
             py::array_t<std::complex<double>> phi({p.NY, p.nkx_loc, p.nkz_loc}), om({p.NY, p.nkx_loc, p.nkz_loc});
             py::array_t<double> U(p.NY);
             s.get_state(phi.mutable_data(), om.mutable_data(), U.mutable_data());
             return py::make_tuple(phi, om, U);
           })
      .def("init_ic", &Solver::init_ic, py::call_guard<py::gil_scoped_release>())
      .def("scalar_on", &Solver::scalar_on)
      .def("set_scalar",
           [](Solver& s, py::array_t<std::complex<double>, py::array::c_style | py::array::forcecast> th) {
             CH_CHECK(static_cast<size_t>(th.size()) == s.plan().spec_elems(), "theta must have NY*nkx_loc*nkz_loc elements");
             py::gil_scoped_release r;
             s.set_scalar(th.data());
           },
           "theta-hat, canonical (NY, nkx, nkz); the mean line (kx, kz) = (0, 0) is the mean profile Theta(y)")
      .def("get_scalar",
           [](Solver& s) {
             const Plan& p = s.plan();
             py::array_t<std::complex<double>> th({p.NY, p.nkx_loc, p.nkz_loc});
             s.get_scalar(th.mutable_data());
             return th;
           })
      .def("init_scalar_ic", &Solver::init_scalar_ic, py::call_guard<py::gil_scoped_release>())
      .def("scalar_flux_hat",
           [](Solver& s) {
             std::vector<std::complex<double>> v;
             {
               py::gil_scoped_release r;
               v = s.scalar_flux_hat();
             }
             const Plan& p = s.plan();
             py::array_t<std::complex<double>> a({static_cast<py::ssize_t>(3), static_cast<py::ssize_t>(p.NY),
                                                  static_cast<py::ssize_t>(p.nkx_loc), static_cast<py::ssize_t>(p.nkz_loc)});
             std::copy(v.begin(), v.end(), a.mutable_data());
             return a;
           },
           "the flux pass alone: (u theta)^, (v theta)^, (w theta)^ of the current state, (3, NY, nkx, nkz)")
      .def("scalar_sums", [](Solver& s) { return profile_rows(s, &Solver::scalar_sums, 5); },
           "(5, NY): Theta, <theta'theta'>, <u'theta'>, <v theta'>, <w theta'>")
      .def("scalar_timing", &Solver::scalar_timing, py::call_guard<py::gil_scoped_release>(),
           "device ms of one substep's scalar work: x-backward, zscalar, x-forward, scalar_kernel")
      .def("prepare", &Solver::prepare, py::call_guard<py::gil_scoped_release>())
      .def("step", &Solver::step, py::arg("stats_for_next") = false, py::call_guard<py::gil_scoped_release>())
      .def("run", &Solver::run, py::arg("nsteps"), py::arg("verbose") = true, py::call_guard<py::gil_scoped_release>())
      .def("synchronize", &Solver::synchronize, py::call_guard<py::gil_scoped_release>())
      .def("log", &Solver::log, py::call_guard<py::gil_scoped_release>())
      .def("stats", [](Solver& s) { return vec(s.stats()); })
      .def("kblocks", &Solver::kblocks)
      .def("bwd_blocks_issued", &Solver::bwd_blocks_issued)
      .def("captured_compute_streams", &Solver::captured_compute_streams)
      .def("spec_kzb", &Solver::spec_kzb)
      .def("combine", &Solver::combine)
      .def("mean_profile", [](Solver& s) { return vec(s.mean_profile()); })
      .def("health", &Solver::health)
      .def("time", &Solver::time)
      .def("steps_done", &Solver::steps_done)
      .def("set_time", &Solver::set_time)
      .def("set_use_graph", &Solver::set_use_graph)
      .def("set_phase_timing", &Solver::set_phase_timing, py::call_guard<py::gil_scoped_release>())
      .def("phase_times_ms", &Solver::phase_times_ms)
      .def("reset_phase_times", &Solver::reset_phase_times)
      .def("set_step_timing", &Solver::set_step_timing)
      .def("step_times_ms", &Solver::step_times_ms, py::call_guard<py::gil_scoped_release>())
      .def("graph_active", &Solver::graph_active)
      .def("comm_kind", &Solver::comm_kind)
      .def("kspec_profile", &Solver::kspec_profile)
      .def("symmetrize", &Solver::symmetrize)
      .def("substep_debug", &Solver::substep_debug, py::call_guard<py::gil_scoped_release>())
      .def("transforms_debug", &Solver::transforms_debug, py::call_guard<py::gil_scoped_release>())
      .def("write_restart", &Solver::write_restart, py::arg("g"), py::arg("ddv"), py::arg("umean") = "-", py::arg("t") = "-",
           py::call_guard<py::gil_scoped_release>())
      .def("read_restart", &Solver::read_restart, py::arg("g"), py::arg("ddv"), py::arg("umean") = "-", py::arg("t") = "-",
           py::call_guard<py::gil_scoped_release>())
      .def("read_restart_regrid", &Solver::read_restart_regrid, py::arg("g"), py::arg("ddv"), py::arg("umean") = "-",
           py::arg("src_stretch") = 0.0, py::call_guard<py::gil_scoped_release>())
      .def("regrid_state",
           [](Solver& s, py::array_t<std::complex<double>, py::array::c_style | py::array::forcecast> phi,
              py::array_t<std::complex<double>, py::array::c_style | py::array::forcecast> om,
              py::array_t<double, py::array::c_style | py::array::forcecast> U, int NX, int NY, int NZ, double stretch) {
             const size_t n = static_cast<size_t>(NY) * (2 * (NX / 3) + 1) * ((2 * NZ - 2) / 3 + 1);
             CH_CHECK(NX >= 3 && NY >= 5 && NZ >= 2 && static_cast<size_t>(phi.size()) == n && static_cast<size_t>(om.size()) == n,
                      "regrid_state: source arrays must have NY*nkx*nkz elements of the source grid");
             CH_CHECK(U.size() == NY, "regrid_state: U must have the source's NY elements");
             py::gil_scoped_release r;
             s.regrid_state(phi.data(), om.data(), U.data(), NX, NY, NZ, stretch);
           },
           py::arg("phi"), py::arg("omega"), py::arg("U"), py::arg("NX"), py::arg("NY"), py::arg("NZ"), py::arg("stretch"))
      .def("regrid_timing", &Solver::regrid_timing)
      .def("checkpoint_async", &Solver::checkpoint_async, py::arg("g"), py::arg("ddv"), py::arg("umean") = "-",
           py::arg("t") = "-", py::call_guard<py::gil_scoped_release>())
      .def("wait_checkpoint", &Solver::wait_checkpoint, py::call_guard<py::gil_scoped_release>())
      .def("barrier", &Solver::barrier, py::call_guard<py::gil_scoped_release>())
      .def("max_over_ranks", &Solver::max_over_ranks, py::call_guard<py::gil_scoped_release>())
      .def("take_snapshot", &Solver::take_snapshot, py::call_guard<py::gil_scoped_release>())
      .def("rollback", &Solver::rollback, py::call_guard<py::gil_scoped_release>())
      .def("rollbacks", &Solver::rollbacks)
      .def("snapshot_step", &Solver::snapshot_step)
      .def("cfl", &Solver::cfl)
      .def("inject_nan", &Solver::inject_nan, py::arg("field") = 0)
      .def("spectra",
           [](Solver& s) {
             Solver::Spectra sp;
             {
               py::gil_scoped_release r;
               sp = s.spectra();
             }
             const Plan& p = s.plan();
             const int np = static_cast<int>(sp.planes.size());
             auto arr = [](const std::vector<double>& v, std::vector<py::ssize_t> shape) {
               py::array_t<double> a(shape);
               std::copy(v.begin(), v.end(), a.mutable_data());
               return a;
             };
             py::dict d;
             d["planes"] = sp.planes;
             d["ekx"] = arr(sp.ekx, {3, np, p.Kx + 1});
             d["ekz"] = arr(sp.ekz, {3, np, p.nkz});
             d["map"] = arr(sp.map, {3, p.nkx, p.nkz});
             return d;
           },
           "energy spectra of u, v, w of the current state at cfg.spectra_planes (global)")
      .def("physical_fields",
           [](Solver& s, const std::vector<int>& planes, const std::vector<std::string>& names) {
             // the arrays view the result in place (a capsule owns it): no second host copy
             auto pf = std::make_unique<Solver::PhysFields>();
             {
               py::gil_scoped_release r;
               *pf = s.physical_fields(planes, names);
             }
             Solver::PhysFields* raw = pf.release();
             py::capsule owner(raw, [](void* q) { delete static_cast<Solver::PhysFields*>(q); });
             const py::ssize_t np = static_cast<py::ssize_t>(raw->planes.size());
             const size_t per = static_cast<size_t>(np) * raw->NX * raw->Nzp;
             py::dict d;
             for (size_t f = 0; f < raw->names.size(); ++f)
               d[py::str(raw->names[f])] = py::array_t<double>({np, static_cast<py::ssize_t>(raw->NX), static_cast<py::ssize_t>(raw->Nzp)},
                                                                raw->data.data() + f * per, owner);
             return d;
           },
           py::arg("planes"), py::arg("names"),
           "physical-space planes of the current state: name -> (nplanes, NX, Nzp) float64 (one rank)")
      .def("plane_moments",
           [](Solver& s) { return profile_rows(s, &Solver::plane_moments, kMomRows); },
           "plane means of u', u'^2, v'^2, w'^2, u'v', u'^3, v'^3, w'^3, u'^4, v'^4, w'^4: (11, NY) (one rank)")
      .def("plane_histograms",
           [](Solver& s, const std::vector<int>& planes, int nbins, int njoint, double span, bool vorticity,
              const std::vector<double>& centre, const std::vector<double>& halfwidth) {
             Solver::PlaneHistograms ph;
             {
               py::gil_scoped_release r;
               ph = s.plane_histograms(planes, nbins, njoint, span, vorticity, centre, halfwidth);
             }
             const py::ssize_t np = static_cast<py::ssize_t>(ph.planes.size()), nhf = static_cast<py::ssize_t>(ph.names.size());
             auto counts = [](const std::vector<unsigned long long>& v, std::vector<py::ssize_t> shape) {
               py::array_t<std::uint64_t> a(shape);
               std::copy(v.begin(), v.end(), a.mutable_data());
               return a;
             };
             auto reals = [](const std::vector<double>& v, std::vector<py::ssize_t> shape) {
               py::array_t<double> a(shape);
               std::copy(v.begin(), v.end(), a.mutable_data());
               return a;
             };
             py::dict d;
             d["planes"] = ph.planes;
             d["names"] = ph.names;
             d["nbins"] = ph.nb;
             d["njoint"] = ph.nj;
             d["hist"] = counts(ph.hist, {nhf, np, ph.nb + 2});
             d["joint"] = counts(ph.joint, {np, ph.nj + 2, ph.nj + 2});
             d["quad"] = reals(ph.quad, {static_cast<py::ssize_t>(kQuadRows), np});
             d["centre"] = reals(ph.centre, {nhf, np});
             d["halfwidth"] = reals(ph.halfwidth, {nhf, np});
             return d;
           },
           py::arg("planes"), py::arg("nbins") = 128, py::arg("njoint") = 64, py::arg("span") = 8.0, py::arg("vorticity") = false,
           py::arg("centre") = std::vector<double>(), py::arg("halfwidth") = std::vector<double>(),
           "histograms of u, v, w (vorticity: and wx, wy, wz) at the given planes: hist (nhf, np, nbins + 2) and joint (u, v) "
           "(np, njoint + 2, njoint + 2) uint64 with under- and overflow bins, quad (8, np): plane means of u'v over Q1..Q4 "
           "and the quadrants' sample fractions, and the centre and halfwidth used, (nhf, np); centre / halfwidth are "
           "flattened (nhf, np) arrays or empty (one rank)")
      .def("gradient_sums",
           [](Solver& s) { return profile_rows(s, &Solver::gradient_sums, kGradRows); },
           "velocity-gradient plane sums wxwx, wywy, wzwz, guu, gvv, gww, guv of the current state: (7, NY), "
           "raw sums (no nu, no factor 2), global over the communicator")
      .def("transport_moments",
           [](Solver& s) { return profile_rows(s, &Solver::transport_moments, kTripleRows); },
           "plane means of u'u'v, wwv, u'vv: (3, NY) (one rank)")
      .def("pressure_hat",
           [](Solver& s) { return canonical_field(s, &Solver::pressure_hat); },
           "Pi = p + |u|^2 / 2 of the current state per (kx, kz) line, (NY, nkx, nkz), zero on the mean line (one rank)")
      .def("pressure_timing", &Solver::pressure_timing, py::call_guard<py::gil_scoped_release>(),
           "device ms of one pressure solve: [transform stage, y-line Poisson kernel] (one rank)")
      .def("pressure_moments",
           [](Solver& s) { return profile_rows(s, &Solver::pressure_moments, 4); },
           "plane means p'p', p'u', p'v, p'w of the fluctuating static pressure: (4, NY) (one rank)")
      .def("static_pressure_hat",
           [](Solver& s) { return canonical_field(s, &Solver::static_pressure_hat); },
           "the fluctuating static pressure p' per (kx, kz) line, (NY, nkx, nkz), zero on the mean line (one rank)")
      .def("pressure_strain",
           [](Solver& s) { return profile_rows(s, &Solver::pressure_strain, kPStrainRows); },
           "Parseval plane sums ps_uu, ps_vv, ps_ww, ps_uv, pu, pv, pp_band of p' with the strain factors: (7, NY) (one rank)")
      .def("plane_spectra",
           [](Solver& s, bool pressure) {
             // the arrays view the result in place (a capsule owns it): no second host copy
             auto sp = std::make_unique<Solver::PlaneSpectra>();
             {
               py::gil_scoped_release r;
               *sp = s.plane_spectra(pressure);
             }
             Solver::PlaneSpectra* raw = sp.release();
             py::capsule owner(raw, [](void* q) { delete static_cast<Solver::PlaneSpectra*>(q); });
             const Plan& p = s.plan();
             auto arr = [&](std::vector<double>& v, int nk) {
               return py::array_t<double>({static_cast<py::ssize_t>(kYSpecRows), static_cast<py::ssize_t>(p.NY),
                                           static_cast<py::ssize_t>(nk)}, v.data(), owner);
             };
             py::dict d;
             d["rows"] = raw->rows;
             d["ekx"] = arr(raw->ekx, p.Kx + 1);
             d["ekz"] = arr(raw->ekz, p.nkz);
             return d;
           },
           py::arg("pressure") = false,
           "1-D spectra and co-spectra uu, vv, ww, uv, wxwx, wywy, wzwz, pp of the current state at every plane: ekx "
           "(8, NY, Kx+1) by |kx|, ekz (8, NY, nkz) by kz, global over the communicator; row pp is zero unless "
           "pressure (one rank)")
      .def("plane_cross_spectra",
           [](Solver& s, const std::vector<int>& refs, const std::string& rows) {
             // the arrays view the result in place (a capsule owns it): no second host copy
             auto cs = std::make_unique<Solver::PlaneCrossSpectra>();
             {
               py::gil_scoped_release r;
               *cs = s.plane_cross_spectra(refs, rows);
             }
             Solver::PlaneCrossSpectra* raw = cs.release();
             py::capsule owner(raw, [](void* q) { delete static_cast<Solver::PlaneCrossSpectra*>(q); });
             const Plan& p = s.plan();
             auto arr = [&](const std::complex<double>* v, int nk) {
               return py::array_t<std::complex<double>>({static_cast<py::ssize_t>(4), static_cast<py::ssize_t>(raw->ref_planes.size()),
                                                         static_cast<py::ssize_t>(p.NY), static_cast<py::ssize_t>(nk)}, v, owner);
             };
             py::dict d;
             d["rows"] = raw->rows;
             d["ref_planes"] = raw->ref_planes;
             d["ckx"] = arr(raw->kx(), p.Kx + 1);
             d["ckz"] = arr(raw->kz(), p.nkz);
             return d;
           },
           py::arg("ref_planes"), py::arg("rows") = "velocity",
           "cross-spectra of every plane against the reference planes (distinct, at most 16), rows uu vv ww uv (velocity) or "
           "u_wz v_wz w_wx wz_wz (shear), the first factor at y and the conjugated second at the reference plane: ckx "
           "(4, nref, NY, Kx+1) by |kx|, ckz (4, nref, NY, nkz) by kz, complex, global over the communicator")
      .def("plane_cross_spectra_timing", &Solver::plane_cross_spectra_timing, py::call_guard<py::gil_scoped_release>(),
           py::arg("ref_planes"), py::arg("rows") = "velocity",
           "device ms of the launches of one plane_cross_spectra() and of one plane_spectra(): [ycross, yspectra]")
      .def("spectral_budgets",
           [](Solver& s) {
             // the arrays view the result in place (a capsule owns it): no second host copy
             auto sb = std::make_unique<Solver::SpectralBudgets>();
             {
               py::gil_scoped_release r;
               *sb = s.spectral_budgets();
             }
             Solver::SpectralBudgets* raw = sb.release();
             py::capsule owner(raw, [](void* q) { delete static_cast<Solver::SpectralBudgets*>(q); });
             const Plan& p = s.plan();
             auto arr = [&](std::vector<double>& v, int nk) {
               return py::array_t<double>({static_cast<py::ssize_t>(kSBudRows), static_cast<py::ssize_t>(p.NY),
                                           static_cast<py::ssize_t>(nk)}, v.data(), owner);
             };
             py::dict d;
             d["rows"] = raw->rows;
             d["ekx"] = arr(raw->ekx, p.Kx + 1);
             d["ekz"] = arr(raw->ekz, p.nkz);
             d["U"] = py::array_t<double>({static_cast<py::ssize_t>(p.NY)}, raw->U.data(), owner);
             d["dU"] = py::array_t<double>({static_cast<py::ssize_t>(p.NY)}, raw->dU.data(), owner);
             return d;
           },
           "spectral Reynolds-stress budget terms of the current state at every plane, rows n_uu n_vv n_ww n_uv g_uu g_vv "
           "g_ww g_uv gs_uu gs_vv gs_ww gs_uv gu gv ps_uu ps_vv ps_ww ps_uv pu pv: ekx (20, NY, Kx+1) by |kx|, ekz "
           "(20, NY, nkz) by kz, and the mean profile U and its derivative dU as used (one rank)")
      .def("spectral_budgets_timing", &Solver::spectral_budgets_timing, py::call_guard<py::gil_scoped_release>(),
           "device ms of the two stages of one spectral_budgets(): [rows 0..7, rows 8..19] (one rank)")
      .def("rotational_hat",
           [](Solver& s) {
             std::vector<std::complex<double>> v;
             {
               py::gil_scoped_release r;
               v = s.rotational_hat();
             }
             const Plan& p = s.plan();
             py::array_t<std::complex<double>> a({static_cast<py::ssize_t>(3), static_cast<py::ssize_t>(p.NY),
                                                  static_cast<py::ssize_t>(p.nkx_loc), static_cast<py::ssize_t>(p.nkz_loc)});
             std::copy(v.begin(), v.end(), a.mutable_data());
             return a;
           },
           "H = (u x omega)^ of the current state per (kx, kz) line, (3, NY, nkx, nkz) (one rank)");

  py::class_<ProcInfo>(m, "ProcInfo")
      .def(py::init<>())
      .def_static("from_env", &ProcInfo::from_env)
      .def_readwrite("rank", &ProcInfo::rank)
      .def_readwrite("size", &ProcInfo::size)
      .def_readwrite("local_rank", &ProcInfo::local_rank);
  m.def(
      "tcp_broadcast",
      [](const ProcInfo& pi, py::bytes payload, int timeout_s) {
        std::string in = payload;
        std::string out;
        {
          py::gil_scoped_release r;
          out = tcp_broadcast(pi, in, timeout_s);
        }
        return py::bytes(out);
      },
      py::arg("pi"), py::arg("payload"), py::arg("timeout_s") = 300,
      "rank 0's payload on every rank (TCP rendezvous at MASTER_ADDR:MASTER_PORT+11)");
  m.def("device_count", &device_count, "visible HIP devices (does not create a context)");
}
