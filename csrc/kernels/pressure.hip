// Pressure: the y-line Poisson solve of kernels.hpp PressureArgs (outside the step).
//
// One 64-lane wave per (kx, kz) line, lane l holding rows l R .. l R + R - 1 as in K-SPEC, W = 4 lines
// per workgroup.  The three inputs H_x, H_y, H_z of a tile are loaded into registers first (thread t:
// line t % W, rows t / W + 64 q, so a row's W lines are one contiguous piece in either spectral
// layout), then pass one by one through an LDS tile (pitch W + 1 slots per row, one more per R rows
// where R (W + 1) is even: the column read of rows lane R + r then strides an odd number of 8-byte
// words between lanes) from which every wave reads its line.  Per line, all in fp64:
//   S = i al H_x + i be H_z + D1 H_y, the four real right-hand sides Re / Im of M S, e_0, e_N of one
//   Helmholtz factorisation (K - k2 M, identity wall rows), the wall derivatives of the three solutions
//   by the dense D1's wall rows, the 2 x 2 system for c1, c2 from (D1 Pi)(+-1) = H_y(+-1) + nu phi(+-1),
//   Pi = Pi_p + c1 g1 + c2 g2.
// The result leaves through the same tile.  A workgroup reads and writes its own W lines only and has
// its inputs in registers before it stores, so Pi may overwrite H_x.  The mean line, padded kz lines
// and the rows N .. spec_rows - 1 of the blocked layout are written as zero.
#include <hip/hip_runtime.h>

#include "channel/common.hpp"
#include "channel/kernels.hpp"
#include "channel/kspec_config.hpp"
#include "channel/yline_device.hpp"

namespace channel {

using namespace dev;

namespace {

constexpr int kPresW = 4;  // lines per workgroup

// all three inputs in registers at once where that is at most 96 registers; else one field at a time
template <int R, typename T>
constexpr bool pres_prefetch_all() {
  return 3 * R * static_cast<int>(sizeof(typename Cplx<T>::type)) / 4 <= 96;
}

template <int R, typename T>
struct PresTile {
  using T2 = typename Cplx<T>::type;
  static constexpr int W = kPresW;
  static constexpr int PITCH = W + 1;
  static constexpr int G = (R * PITCH) % 2 == 1 ? 0 : 1;
  static constexpr int TILE = 64 * R * PITCH + (G ? 64 : 0);
  static __device__ __forceinline__ int row_off(int y) { return y * PITCH + (G ? y / R : 0); }
};

template <int R, typename T, int XM>
__global__ void __launch_bounds__(kPresW * 64) pressure_kernel(YTab t, PressureArgs a) {
  using T2 = typename Cplx<T>::type;
  using Ti = PresTile<R, T>;
  constexpr int W = kPresW;
  constexpr bool kAll = pres_prefetch_all<R, T>();
  __shared__ T2 tile[Ti::TILE];
  __shared__ double xs_mem[W * xl_scratch_doubles(4)];
  const int lane = __lane_id(), w = threadIdx.x / 64;
  const int N = a.N, lines = a.lines;
  const int line0 = blockIdx.x * W;
  const Xl<XM> xl{xs_mem + w * xl_scratch_doubles(4)};

  // cooperative copies: this thread's line (clamped: lines past the end are staged, never stored)
  const int cy = threadIdx.x / W, cl = threadIdx.x % W;
  const int cline = min(line0 + cl, lines - 1);
  const size_t coff = spec_line_off(a.kzb, cline);
  const T2* src[3] = {static_cast<const T2*>(a.hy), static_cast<const T2*>(a.hx), static_cast<const T2*>(a.hz)};
  T2 pend[kAll ? 3 : 1][R];
  auto issue = [&](int f, int slot) {
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int y = min(cy + 64 * q, N - 1);  // rows >= N read row N - 1 (never staged)
      pend[slot][q] = src[f][spec_row_off(a.kzb, lines, y) + coff];
    }
  };
  // stage slot's rows through the tile and read this wave's line (rows >= N as zero)
  auto stage = [&](int slot, double (&x)[2][R]) {
    __syncthreads();  // the previous column reads are done
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int y = cy + 64 * q;
      if (y < N) tile[Ti::row_off(y) + cl] = pend[slot][q];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int y = lane * R + r;
      const T2 v = tile[Ti::row_off(y < N ? y : 0) + w];
      x[0][r] = y < N ? static_cast<double>(v.x) : 0.0;
      x[1][r] = y < N ? static_cast<double>(v.y) : 0.0;
    }
  };
  if constexpr (kAll) {
    issue(0, 0);
    issue(1, 1);
    issue(2, 2);
  }

  const int line = min(line0 + w, lines - 1);
  const int ikx = line / a.nkz, kzl = line - ikx * a.nkz;
  const int kz = a.kz0 + kzl;
  const int ig = a.kx0 + ikx;
  const int kx = ig <= a.Kx ? ig : ig - a.nkx;
  const double al = a.ax * kx, be = a.az * kz;
  const double k2 = al * al + be * be;
  const bool zero_line = (kx == 0 && kz == 0) || kzl >= a.nkz_real;
  // the state's wall rows of this line (two elements per line, the same address in every lane)
  const T2* phi = static_cast<const T2*>(a.phi);
  const size_t loff = spec_line_off(a.kzb, line);
  const T2 ph0 = phi[spec_row_off(a.kzb, lines, 0) + loff], phN = phi[spec_row_off(a.kzb, lines, N - 1) + loff];

  double x[2][R], S[2][R];
  // S = D1 H_y and the wall values of H_y
  if constexpr (!kAll) issue(0, 0);
  stage(0, x);
  double b0[2], bN[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    b0[c] = row_value<R, XM>(x[c], 0, lane);
    bN[c] = row_value<R, XM>(x[c], N - 1, lane);
  }
  d1_apply_to<R, 2, XM>(t, x, S, xl, lane);
  // + i al H_x
  if constexpr (!kAll) issue(1, 0);
  stage(kAll ? 1 : 0, x);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    S[0][r] -= al * x[1][r];
    S[1][r] += al * x[0][r];
  }
  // + i be H_z
  if constexpr (!kAll) issue(2, 0);
  stage(kAll ? 2 : 0, x);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    S[0][r] -= be * x[1][r];
    S[1][r] += be * x[0][r];
  }
  // right-hand sides: Re, Im of M S (zero on the wall rows), e_0, e_N
  const int lN = (N - 1) / R, rN = (N - 1) - lN * R;
  double d[4][R];
  {
    double ms[2][R];
    apply_M<R, 2, XM>(t, S, ms, lane);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      d[0][r] = ms[0][r];
      d[1][r] = ms[1][r];
      d[2][r] = (lane == 0 && r == 0) ? 1.0 : 0.0;
      d[3][r] = (lane == lN && r == rN) ? 1.0 : 0.0;
    }
  }
  {
    PFac<R> F;
    const CoefHelm ch{t, lane, k2};
    pfactor<R, XM>(F, ch, xl, lane);
    psolve<R, 4, XM>(F, ch, d, xl, lane);
  }
  // wall derivatives of the four solutions: rows 0 and N - 1 of the dense D1 (zero past N)
  double s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double r0 = tab(t.d1row0, r, lane), r1 = tab(t.d1rowN, r, lane);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s[k] += r0 * d[k][r];
      s[4 + k] += r1 * d[k][r];
    }
  }
  wave_sum_n<8, XM>(s);
  // [a00 a01; a10 a11] (c1, c2)^T = (D1 Pi)(walls) - (D1 Pi_p)(walls), per real part
  const double a00 = s[2], a01 = s[3], a10 = s[6], a11 = s[7];
  const double idet = 1.0 / (a00 * a11 - a01 * a10);
  const double nu = a.nu;
  const double w0[2] = {b0[0] + nu * static_cast<double>(ph0.x) - s[0], b0[1] + nu * static_cast<double>(ph0.y) - s[1]};
  const double wN[2] = {bN[0] + nu * static_cast<double>(phN.x) - s[4], bN[1] + nu * static_cast<double>(phN.y) - s[5]};
  double c1[2], c2[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    c1[c] = (w0[c] * a11 - a01 * wN[c]) * idet;
    c2[c] = (a00 * wN[c] - a10 * w0[c]) * idet;
  }
  // Pi through the tile, rows N .. spec_rows - 1 as zero
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int y = lane * R + r;
    const double re = d[0][r] + c1[0] * d[2][r] + c2[0] * d[3][r];
    const double im = d[1][r] + c1[1] * d[2][r] + c2[1] * d[3][r];
    const bool z = zero_line || y >= N;
    tile[Ti::row_off(y) + w] = T2{static_cast<T>(z ? 0.0 : re), static_cast<T>(z ? 0.0 : im)};
  }
  __syncthreads();
  T2* dst = static_cast<T2*>(a.pi);
  const int rows = spec_rows(a.kzb, N);
  if (line0 + cl < lines) {
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int y = cy + 64 * q;
      if (y < rows) dst[spec_row_off(a.kzb, lines, y) + coff] = tile[Ti::row_off(y) + cl];
    }
  }
}

template <int R, typename T>
void pressure_launch(const YTablesDev& t, const PressureArgs& a, hipStream_t stream) {
  constexpr int XM = kspec_xmode<R, T>();
  const unsigned nblk = static_cast<unsigned>((a.lines + kPresW - 1) / kPresW);
  hipLaunchKernelGGL((pressure_kernel<R, T, XM>), dim3(nblk), dim3(kPresW * 64), 0, stream, t.tab, a);
}

}  // namespace

void pressure_solve(const YTablesDev& t, const PressureArgs& a, bool fp64, hipStream_t stream) {
  CH_CHECK(t.H == 1, "pressure: one wave per line (not with two-wave K-SPEC lines)");
  CH_CHECK(a.N == t.tab.N && a.N >= 3 && 64 * t.R >= a.N, "pressure: NY mismatch with tables");
  CH_CHECK(a.lines > 0 && a.nkz > 0 && a.lines % a.nkz == 0 && a.nkz_real > 0 && a.nkz_real <= a.nkz, "pressure: bad line geometry");
  CH_CHECK(a.hx && a.hy && a.hz && a.phi && a.pi, "pressure: missing field");
  CH_CHECK(!a.kzb || (a.kzb == kSpecKzBlock && a.nkz % kSpecKzBlock == 0), "pressure: the blocked spectral layout needs whole 8-line kz blocks");
  CH_CHECK(static_cast<long long>(spec_rows(a.kzb, a.N)) * a.lines < (1LL << 31), "pressure: field too large for one launch");
  if (fp64) {
    CH_DISPATCH_R(t.R, (pressure_launch<R, double>(t, a, stream)));
  } else {
    CH_DISPATCH_R(t.R, (pressure_launch<R, float>(t, a, stream)));
  }
  HIP_LAUNCH_CHECK(stream);
}

}  // namespace channel
