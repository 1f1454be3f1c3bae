// Regridding of spectral lines (kernels.hpp RegridArgs): a transposing, interpolating copy from the
// line-major fp64 staging buffer of a restart file (each line contiguous in y) into a spectral field
// of the solver (y outermost; blocked [y/8][line/8][y%8][line%8] or plain [y][line]).  Outside the
// step: it runs once per restart, and it is bound by the source reads and the tile stores.
//
// One wave per workgroup: one target kx, 8 kz lines, one chunk of 8 target planes.
//  * stage: the chunk's source window (the rows its 8 stencils touch, at most max_window) of the 8 lines
//    goes to LDS, read along y as 16-B double2 loads, consecutive lanes on consecutive rows of a line;
//  * form: lane t owns output (plane t / 8, line t % 8) and reads its W stencil values with 16-B LDS
//    reads.  The line pitch is odd in 16-B slots, so the 8 lines of one plane start on 8 different
//    slots of the 16-slot bank row (lanes of one line and neighbouring planes read overlapping or
//    identical rows, which broadcast or fall on neighbouring slots);
//  * store: line-fastest, lane t at element t of the 8 x 8 tile: one whole 512-B (fp32) or 1-KB (fp64)
//    tile in the blocked layout, 8 pieces of 64 / 128 B in the plain one.
// No atomics, no dependence between workgroups.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "channel/common.hpp"
#include "channel/fft_device.hpp"
#include "channel/kernels.hpp"
#include "channel/regrid.hpp"

namespace channel {

namespace {

constexpr int kLines = kSpecKzBlock;   // lines per workgroup
constexpr int kPlanes = kRegridChunk;  // planes per workgroup
constexpr int kThreads = kLines * kPlanes;
static_assert(kThreads == 64 && kRegridChunk == kSpecYBlock, "one wave forms one tile of the blocked layout");

__host__ __device__ inline int regrid_pitch(int max_window) { return max_window | 1; }

template <typename T2>
__global__ __launch_bounds__(kThreads) void regrid_kernel(RegridArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double2* lds = reinterpret_cast<double2*>(smem);
  const int t = threadIdx.x;
  const int kz0 = blockIdx.x * kLines, chunk = blockIdx.y, ik = blockIdx.z;
  const int slot = a.slot[ik];
  if (slot < 0) return;  // (the whole workgroup: no source plane, the field stays zero)
  const int pitch = regrid_pitch(a.max_window);
  if (a.lds_poison) {
    dev::lds_poison_fill(smem, kLines * pitch * static_cast<int>(sizeof(double2)));
    __syncthreads();
  }
  const int win0 = a.win[2 * chunk], winlen = a.win[2 * chunk + 1];
  const int nl = min(kLines, a.ncol - kz0);  // lines of this block with a source (>= 1: the grid covers ncol)
  const double2* src = reinterpret_cast<const double2*>(a.src) + (static_cast<size_t>(slot) * a.scols + kz0) * a.NY_s + win0;
  for (int idx = t; idx < nl * winlen; idx += kThreads) {
    const int l = idx / winlen, r = idx - l * winlen;
    lds[l * pitch + r] = src[static_cast<size_t>(l) * a.NY_s + r];
  }
  __syncthreads();
  const int l = t % kLines, y = chunk * kPlanes + t / kLines;
  if (y >= a.NY_d || kz0 + l >= a.nkzs) return;  // rows and lines past the ends (the blocked layout's padding stays zero)
  double2 v = {0.0, 0.0};
  if (l < nl) {
    const double2* f = lds + l * pitch + (a.j0[y] - win0);
    const int u = a.unit[y];
    if (u >= 0) {
      v = f[u];
    } else {
      const double* w = a.w + static_cast<size_t>(y) * a.W;
      for (int m = 0; m < a.W; ++m) {
        const double2 fm = f[m];
        v.x += w[m] * fm.x;
        v.y += w[m] * fm.y;
      }
    }
    v.x /= a.n2;
    v.y /= a.n2;
  }
  const int ikx = a.ikx0 + ik;
  if (a.U && ikx == a.u_ikx && kz0 + l == 0) v = {a.U[y], 0.0};
  T2 o;
  o.x = static_cast<decltype(o.x)>(v.x);
  o.y = static_cast<decltype(o.y)>(v.y);
  static_cast<T2*>(a.dst)[spec_index(a.kzb, a.nkx_blk, a.nkzs, y, ikx, kz0 + l)] = o;
}

}  // namespace

void regrid_launch(const RegridArgs& a, bool fp64, hipStream_t s) {
  if (a.nkx <= 0 || a.ncol <= 0) return;
  const int chunks = (a.NY_d + kPlanes - 1) / kPlanes;
  const size_t lds = static_cast<size_t>(kLines) * regrid_pitch(a.max_window) * sizeof(double2);
  CH_CHECK(lds <= static_cast<size_t>(kRegridLdsBytes),
           "regrid: a source window of " << a.max_window << " rows per " << kPlanes << " target planes needs " << lds
                                          << " B of LDS (budget " << kRegridLdsBytes << ")");
  CH_CHECK(a.W >= 1 && a.W <= kRegridWidth && a.ncol <= a.scols && a.ncol <= a.nkzs && a.ikx0 >= 0 &&
               a.ikx0 + a.nkx <= a.nkx_blk && (a.kzb == 0 || (a.kzb == kSpecKzBlock && a.nkzs % kSpecKzBlock == 0)),
           "regrid: inconsistent arguments");
  CH_CHECK(chunks <= 65535 && a.nkx <= 65535, "regrid: grid too large");
  const dim3 grid((a.ncol + kLines - 1) / kLines, chunks, a.nkx);
  if (fp64) hipLaunchKernelGGL(regrid_kernel<double2>, grid, dim3(kThreads), lds, s, a);
  else hipLaunchKernelGGL(regrid_kernel<float2>, grid, dim3(kThreads), lds, s, a);
  HIP_LAUNCH_CHECK(s);
}

}  // namespace channel
