// Passive scalar: the y-line advance of one RK3 substep (kernels.hpp ScalarArgs), after K-SPEC.
//
// The geometry of pressure.hip: one 64-lane wave per (kx, kz) line, lane l holding rows l R .. l R + R - 1,
// W = 4 lines per workgroup; the five inputs F_y, F_x, F_z, theta, R_theta of a tile pass one by one
// through the LDS tile (PresTile's padding) from which every wave reads its line.  Per line, in fp64:
//   N = -(i al F_x + D1 F_y + i be F_z)           mean line: Re N + source
//   R_n = M N
//   r = M th + dt [a kappa (K th - k2 M th) + g R_n + z R_prev]     wall rows: 0 (mean line: lower, upper)
//   th_new = ((1 + c k2) M - c K, identity wall rows)^-1 r,  c = b dt kappa
// which is the omega_y equation of K-SPEC with nu -> kappa: one factorisation, two real right-hand sides.
// theta and R_n leave through the same tile, theta in place and R_n over R_prev (not on the last substep).
// A workgroup reads and writes its own W lines only.  The mean line's imaginary part, padded kz lines and
// the rows N .. spec_rows - 1 of the blocked layout are written as zero.
#include <hip/hip_runtime.h>

#include "channel/common.hpp"
#include "channel/kernels.hpp"
#include "channel/kspec_config.hpp"
#include "channel/yline_device.hpp"

namespace channel {

using namespace dev;

namespace {

constexpr int kScalW = 4;  // lines per workgroup

template <int R, typename T>
struct ScalTile {  // (pressure.hip PresTile)
  using T2 = typename Cplx<T>::type;
  static constexpr int W = kScalW;
  static constexpr int PITCH = W + 1;
  static constexpr int G = (R * PITCH) % 2 == 1 ? 0 : 1;
  static constexpr int TILE = 64 * R * PITCH + (G ? 64 : 0);
  static __device__ __forceinline__ int row_off(int y) { return y * PITCH + (G ? y / R : 0); }
};

template <int R, typename T, int XM>
__global__ void __launch_bounds__(kScalW * 64) scalar_kernel(YTab t, ScalarArgs a) {
  using T2 = typename Cplx<T>::type;
  using Ti = ScalTile<R, T>;
  constexpr int W = kScalW;
  __shared__ T2 tile[Ti::TILE];
  __shared__ double xs_mem[W * xl_scratch_doubles(4)];
  const int lane = __lane_id(), w = threadIdx.x / 64;
  const int N = a.N, lines = a.lines;
  const int line0 = blockIdx.x * W;
  if (a.lds_poison) {
    unsigned* pw = reinterpret_cast<unsigned*>(tile);
    for (int i = threadIdx.x; i < static_cast<int>(sizeof(tile) / 4); i += W * 64) pw[i] = 0xFFFFFFFFu;
    pw = reinterpret_cast<unsigned*>(xs_mem);
    for (int i = threadIdx.x; i < static_cast<int>(sizeof(xs_mem) / 4); i += W * 64) pw[i] = 0xFFFFFFFFu;
  }
  const Xl<XM> xl{xs_mem + w * xl_scratch_doubles(4)};

  // cooperative copies: this thread's line (clamped: lines past the end are staged, never stored)
  const int cy = threadIdx.x / W, cl = threadIdx.x % W;
  const int cline = min(line0 + cl, lines - 1);
  const size_t coff = spec_line_off(a.kzb, cline);
  const T2* src[5] = {static_cast<const T2*>(a.fy), static_cast<const T2*>(a.fx), static_cast<const T2*>(a.fz),
                      static_cast<const T2*>(a.th), static_cast<const T2*>(a.Rth)};
  // field f of the tile through LDS into this wave's line (rows >= N as zero)
  auto stage = [&](int f, double (&x)[2][R]) __attribute__((always_inline)) {
    T2 pend[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int y = min(cy + 64 * q, N - 1);  // rows >= N read row N - 1 (never staged)
      pend[q] = src[f][spec_row_off(a.kzb, lines, y) + coff];
    }
    __syncthreads();  // the previous column reads are done
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int y = cy + 64 * q;
      if (y < N) tile[Ti::row_off(y) + cl] = pend[q];
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
  // this wave's line (re, im) through the tile into the field dst, rows N .. spec_rows - 1 as zero
  auto unstage = [&](const double (&x)[2][R], bool zero_line, T2* dst) __attribute__((always_inline)) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int y = lane * R + r;
      const bool z = zero_line || y >= N;
      tile[Ti::row_off(y) + w] = T2{static_cast<T>(z ? 0.0 : x[0][r]), static_cast<T>(z ? 0.0 : x[1][r])};
    }
    __syncthreads();
    const int rows = spec_rows(a.kzb, N);
    if (line0 + cl < lines) {
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int y = cy + 64 * q;
        if (y < rows) dst[spec_row_off(a.kzb, lines, y) + coff] = tile[Ti::row_off(y) + cl];
      }
    }
  };

  const int line = min(line0 + w, lines - 1);
  const int ikx = line / a.nkz, kzl = line - ikx * a.nkz;
  const int kz = a.kz0 + kzl;
  const int ig = a.kx0 + ikx;
  const int kx = ig <= a.Kx ? ig : ig - a.nkx;
  const double al = a.ax * kx, be = a.az * kz;
  const double k2 = al * al + be * be;
  const bool mean = kx == 0 && kz == 0;
  const bool zero_line = kzl >= a.nkz_real;
  const double dt = *a.dt;
  const int lN = (N - 1) / R, rN = (N - 1) - lN * R;

  double x[2][R], S[2][R];
  // S = -N = D1 F_y + i al F_x + i be F_z
  stage(0, x);
  d1_apply_to<R, 2, XM>(t, x, S, xl, lane);
  stage(1, x);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    S[0][r] -= al * x[1][r];
    S[1][r] += al * x[0][r];
  }
  stage(2, x);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool in = lane * R + r < N;
    S[0][r] = -(S[0][r] - be * x[1][r]) + ((mean && in) ? a.source : 0.0);
    S[1][r] = mean ? 0.0 : -(S[1][r] + be * x[0][r]);
  }
  // R_n = M N
  double Rn[2][R];
  apply_M<R, 2, XM>(t, S, Rn, lane);
  // r = (1 - dt a kappa k2) M th + dt a kappa K th + dt (g R_n + z R_prev)
  double d[2][R];
  stage(3, x);
  bool bad = false;
#pragma unroll
  for (int r = 0; r < R; ++r) bad = bad || !(isfinite(x[0][r]) && isfinite(x[1][r]));
  {
    double mt[2][R], kt[2][R];
    apply_M<R, 2, XM>(t, x, mt, lane);
    apply_K<R, 2, XM>(t, x, kt, lane);
    const double ca = dt * a.rk_a * a.kappa;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      d[0][r] = mt[0][r] + ca * (kt[0][r] - k2 * mt[0][r]) + dt * a.rk_g * Rn[0][r];
      d[1][r] = mt[1][r] + ca * (kt[1][r] - k2 * mt[1][r]) + dt * a.rk_g * Rn[1][r];
    }
  }
  stage(4, x);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    d[0][r] += dt * a.rk_z * x[0][r];
    d[1][r] += dt * a.rk_z * x[1][r];
    // wall rows (M and K have zero wall rows, R_prev was stored with them): the Dirichlet values
    if (lane == 0 && r == 0) {
      d[0][r] = mean ? a.lower : 0.0;
      d[1][r] = 0.0;
    }
    if (lane == lN && r == rN) {
      d[0][r] = mean ? a.upper : 0.0;
      d[1][r] = 0.0;
    }
  }
  {
    const double c = a.rk_b * dt * a.kappa;
    PFac<R> F;
    const CoefImpl ci{t, lane, 1.0 + c * k2, c};
    pfactor<R, XM>(F, ci, xl, lane);
    psolve<R, 2, XM>(F, ci, d, xl, lane);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    bad = bad || !(isfinite(d[0][r]) && isfinite(d[1][r]));
    if (mean) d[1][r] = 0.0;
  }
  if (a.health && bad && !zero_line && line0 + w < lines) atomicOr(a.health, 1u);
  unstage(d, zero_line, static_cast<T2*>(a.th));
  if (a.store_r) unstage(Rn, zero_line, static_cast<T2*>(a.Rth));
}

template <int R, typename T>
void scalar_launch(const YTablesDev& t, const ScalarArgs& a, hipStream_t stream) {
  constexpr int XM = kspec_xmode<R, T>();
  const unsigned nblk = static_cast<unsigned>((a.lines + kScalW - 1) / kScalW);
  hipLaunchKernelGGL((scalar_kernel<R, T, XM>), dim3(nblk), dim3(kScalW * 64), 0, stream, t.tab, a);
}

}  // namespace

void scalar_advance(const YTablesDev& t, const ScalarArgs& a, bool fp64, hipStream_t stream) {
  CH_CHECK(t.H == 1, "scalar: one wave per line (not with two-wave K-SPEC lines)");
  CH_CHECK(a.N == t.tab.N && a.N >= 3 && 64 * t.R >= a.N, "scalar: NY mismatch with tables");
  CH_CHECK(a.lines > 0 && a.nkz > 0 && a.lines % a.nkz == 0 && a.nkz_real > 0 && a.nkz_real <= a.nkz, "scalar: bad line geometry");
  CH_CHECK(a.fx && a.fy && a.fz && a.th && a.Rth && a.dt, "scalar: missing field");
  CH_CHECK(!a.kzb || (a.kzb == kSpecKzBlock && a.nkz % kSpecKzBlock == 0), "scalar: the blocked spectral layout needs whole 8-line kz blocks");
  CH_CHECK(static_cast<long long>(spec_rows(a.kzb, a.N)) * a.lines < (1LL << 31), "scalar: field too large for one launch");
  if (fp64) {
    CH_DISPATCH_R(t.R, (scalar_launch<R, double>(t, a, stream)));
  } else {
    CH_DISPATCH_R(t.R, (scalar_launch<R, float>(t, a, stream)));
  }
  HIP_LAUNCH_CHECK(stream);
}

}  // namespace channel
