// Regridding of a spectral state: the host tables of a restart onto another grid of the same box.
//
// A state (phi, omega_y, U) on a source grid (NX_s, NY_s, NZ_s, stretch_s) is carried to the solver's
// own grid.  Fourier modes map by index (truncation or zero padding in x and z: regrid_mode_map) and
// every (kx, kz) line is interpolated along y, the physical coordinate of the two tanh grids, by
// Lagrange polynomials over a contiguous stencil of W = min(kRegridWidth, NY_s) source nodes
// (regrid_table).  The tables are fp64, depend on the two grids only and are shared by every line;
// the kernel that applies them is regrid_launch (kernels.hpp, kernels/regrid.hip).
#pragma once

#include <vector>

namespace channel {

constexpr int kRegridWidth = 6;     // stencil nodes (exact for polynomials of degree W - 1)
constexpr int kRegridChunk = 8;     // target planes per workgroup (kSpecYBlock: one tile of the blocked layout)
constexpr double kRegridSnap = 1e-14;  // |y_d - y_s| at or below this: the target node takes the source node's value

struct RegridTable {
  int NY_s = 0, NY_d = 0, W = 0;
  std::vector<int> j0;        // [NY_d] first source node of the stencil
  std::vector<int> unit;      // [NY_d] m when row j is the unit row e_m (a shared node), else -1
  std::vector<double> w;      // [NY_d][W]
  // per chunk of kRegridChunk target planes: the source rows [win0, win0 + winlen) its stencils touch
  std::vector<int> win0, winlen;
  int max_window() const;
};
// y of the source grid: tanh grid of NY_s points at stretch s_s (YGrid::build), likewise the target
RegridTable regrid_table(int NY_s, double s_s, int NY_d, double s_d);

struct RegridModeMap {
  std::vector<int> plane;     // [nkx_loc] source plane (FFT position in an NX_s array) of local target kx i, or -1
  int nkz_take = 0;           // global target kz 0 .. nkz_take - 1 take the source column of the same kz
};
// target: retained kx in compact FFT order (plan.hpp), local range [kx0, kx0 + nkx_loc) of nkx = 2 Kx_d + 1
RegridModeMap regrid_mode_map(int NX_s, int NZ_s, int NX_d, int NZ_d, int kx0, int nkx_loc);

}  // namespace channel
