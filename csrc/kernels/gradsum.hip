// Velocity-gradient plane sums over the spectral fields (kernels.hpp GradSumArgs): a bandwidth-bound
// reduction outside the step.
//
// A row group is what the layout stores contiguously: one plane of `lines` elements (kzb = 0) or an
// 8-plane chunk of 8 * lines elements ordered [line / 8][y % 8][line % 8] (kzb = 8).  A block walks
// one slice of a row group with consecutive lanes on consecutive elements, so a wave's accesses are
// whole 64-byte [y % 8][line % 8] pieces; in the blocked fp32 layout each lane takes two complex
// elements per field (16-byte loads; the pieces are 64-byte aligned).  The slice length is a
// multiple of the block's stride, a multiple of 64 elements, so a lane stays on one plane of the
// chunk and keeps the kGradRows sums of that plane in registers.  The sums are reduced over the
// lanes of the same plane with shuffles, over the block's waves through LDS, and leave the block as
// one atomicAdd per (plane, row).  Padded planes (y >= N) are not loaded; padded kz lines are
// loaded with their piece and masked (they are not assumed to be zero).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "channel/common.hpp"
#include "channel/kernels.hpp"

namespace channel {

namespace {

constexpr int kGsNT = 256;           // threads per block
constexpr int kGsBlocks = 2048;      // blocks per launch aimed at (8 per CU)

template <typename T2, int V>
struct alignas(sizeof(T2) * V) GsVec {
  T2 c[V];
};

struct GsC {
  double x, y;
};

template <typename T2, int V, bool TILED>
__global__ void __launch_bounds__(kGsNT) gradsum_kernel(GradSumArgs a, int seg) {
  constexpr int PG = TILED ? kSpecYBlock : 1;  // planes per row group
  constexpr int NW = kGsNT / 64;
  using Vec = GsVec<T2, V>;
  const int tid = threadIdx.x;
  const int lines = a.nkx_loc * a.nkzs;
  const int span = TILED ? kSpecYBlock * lines : lines;
  const int rg = blockIdx.y;
  const size_t base = static_cast<size_t>(rg) * span;
  const int e0 = blockIdx.x * seg, e1 = min(span, e0 + seg);
  const int yy = TILED ? ((tid * V) >> 3) & 7 : 0;
  const int y = TILED ? rg * kSpecYBlock + yy : rg;
  const int nf = a.combine ? 5 : 6;
  double s[kGradRows];
#pragma unroll
  for (int q = 0; q < kGradRows; ++q) s[q] = 0.0;
  if (y < a.N) {
    for (int e = e0 + tid * V; e < e1; e += kGsNT * V) {
      Vec v[6];
#pragma unroll
      for (int f = 0; f < 6; ++f)
        if (f < nf) v[f] = *reinterpret_cast<const Vec*>(static_cast<const T2*>(a.f[f]) + base + e);
      // (the V elements of an access share the kx row: blocked lines come in eights and nkzs % 8 == 0)
      const int line = TILED ? ((e >> 6) << 3) | (e & 7) : e;
      const int ikx = line / a.nkzs, kl0 = line - ikx * a.nkzs;
      const int ig = a.kx0 + ikx;
      const int kx = ig <= a.Kx ? ig : ig - a.nkx;
      const double al = a.ax * kx;
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const int kl = kl0 + u, kz = a.kz0 + kl;
        if (kl >= a.nkz_loc || (kx == 0 && kz == 0)) continue;
        const double wgt = kz == 0 ? 1.0 : 2.0;
        const double be = a.az * kz, k2 = al * al + be * be;
        GsC cu, cv, cw, ox, oy, oz;
        cv = GsC{static_cast<double>(v[1].c[u].x), static_cast<double>(v[1].c[u].y)};
        if (a.combine) {
          // u = i (al D1v - be om) / k2, w = i (be D1v + al om) / k2, omega_x = i (be phi + al D1om) / k2,
          // omega_z = i (be D1om - al phi) / k2 (COMPAT.md "combine mode"; fft_impl.hpp cmb_pair)
          const double r = 1.0 / k2;
          const GsC d{static_cast<double>(v[0].c[u].x), static_cast<double>(v[0].c[u].y)};
          const GsC dom{static_cast<double>(v[2].c[u].x), static_cast<double>(v[2].c[u].y)};
          const GsC ph{static_cast<double>(v[4].c[u].x), static_cast<double>(v[4].c[u].y)};
          oy = GsC{static_cast<double>(v[3].c[u].x), static_cast<double>(v[3].c[u].y)};
          cu = GsC{-(al * d.y - be * oy.y) * r, (al * d.x - be * oy.x) * r};
          cw = GsC{-(be * d.y + al * oy.y) * r, (be * d.x + al * oy.x) * r};
          ox = GsC{-(be * ph.y + al * dom.y) * r, (be * ph.x + al * dom.x) * r};
          oz = GsC{-(be * dom.y - al * ph.y) * r, (be * dom.x - al * ph.x) * r};
        } else {
          cu = GsC{static_cast<double>(v[0].c[u].x), static_cast<double>(v[0].c[u].y)};
          cw = GsC{static_cast<double>(v[2].c[u].x), static_cast<double>(v[2].c[u].y)};
          ox = GsC{static_cast<double>(v[3].c[u].x), static_cast<double>(v[3].c[u].y)};
          oy = GsC{static_cast<double>(v[4].c[u].x), static_cast<double>(v[4].c[u].y)};
          oz = GsC{static_cast<double>(v[5].c[u].x), static_cast<double>(v[5].c[u].y)};
        }
        // D u = i al v - omega_z, D w = omega_x + i be v, D v = -i (al u + be w)
        const GsC du{-al * cv.y - oz.x, al * cv.x - oz.y};
        const GsC dw{ox.x - be * cv.y, ox.y + be * cv.x};
        const GsC dv{al * cu.y + be * cw.y, -(al * cu.x + be * cw.x)};
        s[0] += wgt * (ox.x * ox.x + ox.y * ox.y);
        s[1] += wgt * (oy.x * oy.x + oy.y * oy.y);
        s[2] += wgt * (oz.x * oz.x + oz.y * oz.y);
        s[3] += wgt * (k2 * (cu.x * cu.x + cu.y * cu.y) + du.x * du.x + du.y * du.y);
        s[4] += wgt * (k2 * (cv.x * cv.x + cv.y * cv.y) + dv.x * dv.x + dv.y * dv.y);
        s[5] += wgt * (k2 * (cw.x * cw.x + cw.y * cw.y) + dw.x * dw.x + dw.y * dw.y);
        s[6] += wgt * (k2 * (cu.x * cv.x + cu.y * cv.y) + du.x * dv.x + du.y * dv.y);
      }
    }
  }
  // lanes of one plane: all 64 (plain); lane bits 3..5 select the plane with one element per lane,
  // bits 2..4 with two
  __shared__ double red[NW][PG][kGradRows];
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int q = 0; q < kGradRows; ++q) {
    double x = s[q];
    if (!TILED) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    } else if (V == 2) {
      x += __shfl_xor(x, 1);
      x += __shfl_xor(x, 2);
      x += __shfl_xor(x, 32);
    } else {
      x += __shfl_xor(x, 1);
      x += __shfl_xor(x, 2);
      x += __shfl_xor(x, 4);
    }
    const bool first = !TILED ? lane == 0 : (V == 2 ? (lane & 0x23) == 0 : (lane & 7) == 0);
    if (first) red[w][yy][q] = x;
  }
  __syncthreads();
  if (tid < PG * kGradRows) {
    const int p = tid / kGradRows, q = tid - p * kGradRows;
    const int yo = TILED ? rg * kSpecYBlock + p : rg;
    double x = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) x += red[i][p][q];
    if (yo < a.N) atomicAdd(&a.sums[static_cast<size_t>(q) * a.N + yo], x);
  }
}

template <typename T2, int V, bool TILED>
void gradsum_launch(const GradSumArgs& a, hipStream_t s) {
  const long long lines = static_cast<long long>(a.nkx_loc) * a.nkzs;
  const long long span = TILED ? kSpecYBlock * lines : lines;
  CH_CHECK(span + kGsNT * V < (1LL << 31), "gradsum: row group too long for one launch");
  const int rgs = TILED ? (a.N + kSpecYBlock - 1) / kSpecYBlock : a.N;
  const long long per = kGsNT * V;  // elements per block iteration: a multiple of 64
  const long long iters = (span + per - 1) / per;
  const long long want = std::max<long long>(1, std::min<long long>(iters, kGsBlocks / rgs));
  const long long seg = (iters + want - 1) / want * per;
  const long long nsl = (span + seg - 1) / seg;
  hipLaunchKernelGGL((gradsum_kernel<T2, V, TILED>), dim3(static_cast<unsigned>(nsl), static_cast<unsigned>(rgs)),
                     dim3(kGsNT), 0, s, a, static_cast<int>(seg));
}

}  // namespace

void gradsum_accumulate(const GradSumArgs& a, bool fp64, hipStream_t s) {
  CH_CHECK(a.N > 0 && a.nkx_loc > 0 && a.nkz_loc > 0 && a.nkzs >= a.nkz_loc && a.sums, "gradsum: empty");
  CH_CHECK(a.kzb == 0 || (a.kzb == kSpecKzBlock && a.nkzs % kSpecKzBlock == 0), "gradsum: bad spectral layout");
  CH_CHECK(a.N <= 65535, "gradsum: too many planes");
  const int nf = a.combine ? 5 : 6;
  bool al16 = true;
  for (int f = 0; f < nf; ++f) {
    CH_CHECK(a.f[f], "gradsum: missing field " << f);
    al16 = al16 && reinterpret_cast<uintptr_t>(a.f[f]) % 16 == 0;
  }
  if (a.kzb) {
    if (fp64) gradsum_launch<double2, 1, true>(a, s);
    else if (al16) gradsum_launch<float2, 2, true>(a, s);
    else gradsum_launch<float2, 1, true>(a, s);
  } else {
    if (fp64) gradsum_launch<double2, 1, false>(a, s);
    else gradsum_launch<float2, 1, false>(a, s);
  }
  HIP_LAUNCH_CHECK(s);
}

}  // namespace channel
