// Pressure-strain plane sums over the spectral fields (kernels.hpp PStrainArgs): the Parseval products
// of the fluctuating static pressure with the strain factors, a bandwidth-bound reduction outside the
// step with the walk, the masks and the reduction of gradsum.hip.
//
// A row group is what the layout stores contiguously: one plane of `lines` elements (kzb = 0) or an
// 8-plane chunk of 8 * lines elements ordered [line / 8][y % 8][line % 8] (kzb = 8).  A block walks
// one slice of a row group with consecutive lanes on consecutive elements, so a wave's accesses are
// whole 64-byte [y % 8][line % 8] pieces; in the blocked fp32 layout each lane takes two complex
// elements per field (16-byte loads).  The slice length is a multiple of the block's stride, a
// multiple of 64 elements, so a lane stays on one plane of the chunk and keeps the kPStrainRows sums
// of that plane in registers.  The sums are reduced over the lanes of the same plane with shuffles,
// over the block's waves through LDS, and leave the block as one atomicAdd per (plane, row).  Padded
// planes (y >= N) are not loaded; padded kz lines are loaded with their piece and masked.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "channel/common.hpp"
#include "channel/kernels.hpp"

namespace channel {

namespace {

constexpr int kPsNT = 256;       // threads per block
constexpr int kPsBlocks = 2048;  // blocks per launch aimed at (8 per CU)

template <typename T2, int V>
struct alignas(sizeof(T2) * V) PsVec {
  T2 c[V];
};

struct PsC {
  double x, y;
};
// Re(a conj b)
__device__ __forceinline__ double ps_dot(PsC a, PsC b) { return a.x * b.x + a.y * b.y; }

template <typename T2, int V, bool TILED>
__global__ void __launch_bounds__(kPsNT) pstrain_kernel(PStrainArgs a, int seg) {
  constexpr int PG = TILED ? kSpecYBlock : 1;  // planes per row group
  constexpr int NW = kPsNT / 64;
  using Vec = PsVec<T2, V>;
  const int tid = threadIdx.x;
  const int lines = a.nkx_loc * a.nkzs;
  const int span = TILED ? kSpecYBlock * lines : lines;
  const int rg = blockIdx.y;
  const size_t base = static_cast<size_t>(rg) * span;
  const int e0 = blockIdx.x * seg, e1 = min(span, e0 + seg);
  const int yy = TILED ? ((tid * V) >> 3) & 7 : 0;
  const int y = TILED ? rg * kSpecYBlock + yy : rg;
  const int nf = a.combine ? 5 : 4;
  double s[kPStrainRows];
#pragma unroll
  for (int q = 0; q < kPStrainRows; ++q) s[q] = 0.0;
  if (y < a.N) {
    for (int e = e0 + tid * V; e < e1; e += kPsNT * V) {
      const Vec vp = *reinterpret_cast<const Vec*>(static_cast<const T2*>(a.p) + base + e);
      Vec v[5];
#pragma unroll
      for (int f = 0; f < 5; ++f)
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
        const double be = a.az * kz;
        const PsC cp{static_cast<double>(vp.c[u].x), static_cast<double>(vp.c[u].y)};
        const PsC cv{static_cast<double>(v[1].c[u].x), static_cast<double>(v[1].c[u].y)};
        PsC cu, cw, oz;
        if (a.combine) {
          // u = i (al D1v - be om) / k2, w = i (be D1v + al om) / k2, omega_z = i (be D1om - al phi) / k2
          // (COMPAT.md "combine mode"; fft_impl.hpp cmb_pair)
          const double r = 1.0 / (al * al + be * be);
          const PsC d{static_cast<double>(v[0].c[u].x), static_cast<double>(v[0].c[u].y)};
          const PsC dom{static_cast<double>(v[2].c[u].x), static_cast<double>(v[2].c[u].y)};
          const PsC om{static_cast<double>(v[3].c[u].x), static_cast<double>(v[3].c[u].y)};
          const PsC ph{static_cast<double>(v[4].c[u].x), static_cast<double>(v[4].c[u].y)};
          cu = PsC{-(al * d.y - be * om.y) * r, (al * d.x - be * om.x) * r};
          cw = PsC{-(be * d.y + al * om.y) * r, (be * d.x + al * om.x) * r};
          oz = PsC{-(be * dom.y - al * ph.y) * r, (be * dom.x - al * ph.x) * r};
        } else {
          cu = PsC{static_cast<double>(v[0].c[u].x), static_cast<double>(v[0].c[u].y)};
          cw = PsC{static_cast<double>(v[2].c[u].x), static_cast<double>(v[2].c[u].y)};
          oz = PsC{static_cast<double>(v[3].c[u].x), static_cast<double>(v[3].c[u].y)};
        }
        // strain factors: i al u, D v = -i (al u + be w), i be w, D u + i al v = 2 i al v - omega_z
        const PsC sxx{-al * cu.y, al * cu.x};
        const PsC szz{-be * cw.y, be * cw.x};
        const PsC syy{al * cu.y + be * cw.y, -(al * cu.x + be * cw.x)};
        const PsC sxy{-2.0 * al * cv.y - oz.x, 2.0 * al * cv.x - oz.y};
        s[0] += wgt * 2.0 * ps_dot(cp, sxx);
        s[1] += wgt * 2.0 * ps_dot(cp, syy);
        s[2] += wgt * 2.0 * ps_dot(cp, szz);
        s[3] += wgt * ps_dot(cp, sxy);
        s[4] += wgt * ps_dot(cp, cu);
        s[5] += wgt * ps_dot(cp, cv);
        s[6] += wgt * ps_dot(cp, cp);
      }
    }
  }
  // lanes of one plane: all 64 (plain); lane bits 3..5 select the plane with one element per lane,
  // bits 2..4 with two
  __shared__ double red[NW][PG][kPStrainRows];
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int q = 0; q < kPStrainRows; ++q) {
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
  if (tid < PG * kPStrainRows) {
    const int p = tid / kPStrainRows, q = tid - p * kPStrainRows;
    const int yo = TILED ? rg * kSpecYBlock + p : rg;
    double x = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) x += red[i][p][q];
    if (yo < a.N) atomicAdd(&a.sums[static_cast<size_t>(q) * a.N + yo], x);
  }
}

template <typename T2, int V, bool TILED>
void pstrain_launch(const PStrainArgs& a, hipStream_t s) {
  const long long lines = static_cast<long long>(a.nkx_loc) * a.nkzs;
  const long long span = TILED ? kSpecYBlock * lines : lines;
  CH_CHECK(span + kPsNT * V < (1LL << 31), "pstrain: row group too long for one launch");
  const int rgs = TILED ? (a.N + kSpecYBlock - 1) / kSpecYBlock : a.N;
  const long long per = kPsNT * V;  // elements per block iteration: a multiple of 64
  const long long iters = (span + per - 1) / per;
  const long long want = std::max<long long>(1, std::min<long long>(iters, kPsBlocks / rgs));
  const long long seg = (iters + want - 1) / want * per;
  const long long nsl = (span + seg - 1) / seg;
  hipLaunchKernelGGL((pstrain_kernel<T2, V, TILED>), dim3(static_cast<unsigned>(nsl), static_cast<unsigned>(rgs)),
                     dim3(kPsNT), 0, s, a, static_cast<int>(seg));
}

// the mean line (local kx 0, kz 0) of every plane of one spectral field becomes zero
template <typename T2>
__global__ void __launch_bounds__(64) zero_mean_line_kernel(T2* q, int N, int kzb, int lines) {
  const int y = blockIdx.x * 64 + threadIdx.x;
  if (y < N) q[spec_row_off(kzb, lines, y)] = T2{0, 0};
}

}  // namespace

void pstrain_accumulate(const PStrainArgs& a, bool fp64, hipStream_t s) {
  CH_CHECK(a.N > 0 && a.nkx_loc > 0 && a.nkz_loc > 0 && a.nkzs >= a.nkz_loc && a.sums && a.p, "pstrain: empty");
  CH_CHECK(a.kzb == 0 || (a.kzb == kSpecKzBlock && a.nkzs % kSpecKzBlock == 0), "pstrain: bad spectral layout");
  CH_CHECK(a.N <= 65535, "pstrain: too many planes");
  const int nf = a.combine ? 5 : 4;
  bool al16 = reinterpret_cast<uintptr_t>(a.p) % 16 == 0;
  for (int f = 0; f < nf; ++f) {
    CH_CHECK(a.f[f], "pstrain: missing field " << f);
    al16 = al16 && reinterpret_cast<uintptr_t>(a.f[f]) % 16 == 0;
  }
  if (a.kzb) {
    if (fp64) pstrain_launch<double2, 1, true>(a, s);
    else if (al16) pstrain_launch<float2, 2, true>(a, s);
    else pstrain_launch<float2, 1, true>(a, s);
  } else {
    if (fp64) pstrain_launch<double2, 1, false>(a, s);
    else pstrain_launch<float2, 1, false>(a, s);
  }
  HIP_LAUNCH_CHECK(s);
}

void zero_mean_line(void* q, int N, int kzb, int lines, bool fp64, hipStream_t s) {
  CH_CHECK(q && N > 0 && lines > 0, "zero_mean_line: empty");
  const dim3 grid(static_cast<unsigned>((N + 63) / 64));
  if (fp64) hipLaunchKernelGGL((zero_mean_line_kernel<double2>), grid, dim3(64), 0, s, static_cast<double2*>(q), N, kzb, lines);
  else hipLaunchKernelGGL((zero_mean_line_kernel<float2>), grid, dim3(64), 0, s, static_cast<float2*>(q), N, kzb, lines);
  HIP_LAUNCH_CHECK(s);
}

}  // namespace channel
