// Spectral Reynolds-stress budgets at every plane (kernels.hpp SBudgetArgs): the reduction of the
// plane spectra (yspectra.hip: the same walk of the layouts, weights, masks and outputs) over more
// inputs and more rows.  The 20 rows come in two stages, because the rotational term H and the pressure
// share a buffer: stage 0 reads the six fields and H_x, H_y, H_z (9 fields, 8 rows), stage 1 reads
// u, v, w, omega_z, Pi and p-hat' (6 fields, 12 rows).
//
// As in yspectra.hip a block takes one row group (a plane, or an 8-plane chunk of the blocked layout), one
// slice of kz lines and one slice of kx rows, and a lane keeps its (plane, kz) over the kx loop:
//  * its products are summed over kx in registers (fp64) and leave once at the end;
//  * per kx the products are summed over the lanes of the same plane with reduce-scatters of shuffles
//    (the rows in groups of eight and, stage 1, a group of four) and over the block's waves by LDS
//    atomics into one accumulator per (|kx| bin of the slice, plane, row).
// Both sets leave the block through LDS as contiguous runs: one atomicAdd per (row, plane, bin) and
// block, consecutive lanes on consecutive bins.  Padded planes (y >= N) and lines past the line stride
// are not loaded; padded kz lines (kl >= nkz_loc) are loaded with their piece and masked.
#include "specwalk.hpp"

namespace channel {

namespace {

using namespace specwalk;
constexpr int kSbNT = kNT, kSbBlocks = kBlocks;
constexpr int kSbKxMax = 64, kSbKxMin = 8;  // kx rows per block (yspectra.hip)

constexpr int sb_rows(int stage) { return stage == 0 ? kSBudStage0Rows : kSBudRows - kSBudStage0Rows; }
constexpr int sb_max(int a, int b) { return a > b ? a : b; }
// doubles of LDS: the |kx| accumulators [bin][slot + 1], later the kz sums [slot][lines + 1]
constexpr int sb_lds(int rows, bool tiled, int zl) {
  const int slots = tiled ? kSpecYBlock * rows : rows;
  return sb_max(kSbKxMax * (slots + 1), slots * (zl + 1));
}

// Sum of t[R0 + q], q < 8, over the 8 lanes that differ in the lane bits M0, M1, M2: the lane with bits
// (b0, b1, b2) returns row R0 + 4 b0 + 2 b1 + b2.
template <int R0, int M0, int M1, int M2, int NR>
__device__ __forceinline__ double sb_scatter8(const double (&t)[NR], int lane) {
  const bool b0 = lane & M0, b1 = lane & M1, b2 = lane & M2;
  double a[4], b[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = (b0 ? t[R0 + j + 4] : t[R0 + j]) + __shfl_xor(b0 ? t[R0 + j] : t[R0 + j + 4], M0);
#pragma unroll
  for (int j = 0; j < 2; ++j) b[j] = (b1 ? a[j + 2] : a[j]) + __shfl_xor(b1 ? a[j] : a[j + 2], M1);
  return (b2 ? b[1] : b[0]) + __shfl_xor(b2 ? b[0] : b[1], M2);
}
// The same for four rows: the lane with bits (b0, b1) returns row R0 + 2 b0 + b1, in both lanes of b2.
template <int R0, int M0, int M1, int M2, int NR>
__device__ __forceinline__ double sb_scatter4(const double (&t)[NR], int lane) {
  const bool b0 = lane & M0, b1 = lane & M1;
  double a[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) a[j] = (b0 ? t[R0 + j + 2] : t[R0 + j]) + __shfl_xor(b0 ? t[R0 + j] : t[R0 + j + 2], M0);
  double x = (b1 ? a[1] : a[0]) + __shfl_xor(b1 ? a[0] : a[1], M1);
  x += __shfl_xor(x, M2);
  return x;
}

__device__ __forceinline__ int sb_akx(const SBudgetArgs& a, int ig) { return ig <= a.Kx ? ig : a.nkx - ig; }

template <typename T2, int V, bool TILED, int STAGE>
__global__ void __launch_bounds__(kSbNT) sbudget_kernel(SBudgetArgs a, int kxs) {
  constexpr int NR = sb_rows(STAGE);                         // rows of this stage
  constexpr int ROW0 = STAGE == 0 ? 0 : kSBudStage0Rows;     // its first row of the outputs
  constexpr int ZL = TILED ? 4 * kSpecKzBlock * V : kSbNT;   // kz lines per slice
  constexpr int SL = kSpecYBlock * NR;                       // (plane of the chunk, row) pairs
  constexpr int NS = TILED ? SL : NR;                        // slots in use
  constexpr int LDS = sb_lds(NR, TILED, ZL);
  constexpr unsigned SIX = STAGE == 0 ? kAll : (kU | kV | kW | kOz);
  static_assert(NR == 8 || NR == 12, "the rows are reduced in a group of eight and a group of four");
  static_assert(NS * (ZL + 1) <= LDS && kSbKxMax * (NS + 1) <= LDS, "both sets of sums are staged in the same LDS");
  __shared__ double acc[LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int zs = blockIdx.x, rg = blockIdx.y;
  // this lane's plane of the chunk and first line of the slice; the element offset in a kx row
  const int yy = plane_of<V, TILED>(tid);
  const int kll = TILED ? (((tid * V) >> 6) << 3) | ((tid * V) & 7) : tid;
  const int kl0 = zs * ZL + kll;
  const int y = TILED ? rg * kSpecYBlock + yy : rg;
  const int rowlen = TILED ? kSpecYBlock * a.nkzs : a.nkzs;  // elements per kx row of the row group
  const int eoff = TILED ? zs * (kSbNT * V) + tid * V : kl0;
  const size_t base = static_cast<size_t>(rg) * rowlen * a.nkx_loc;
  const bool live = y < a.N && kl0 < (TILED ? a.nkzs : a.nkz_loc);
  const int i0 = blockIdx.z * kxs, i1 = min(a.nkx_loc, i0 + kxs);
  // |kx| bins of rows i0 .. i1 - 1: global indices 0 .. Kx hold kx >= 0, the rest kx = ig - nkx < 0
  const int g0 = a.kx0 + i0, g1 = a.kx0 + i1 - 1;
  const bool straddle = g0 <= a.Kx && g1 > a.Kx;
  const int amin = min(sb_akx(a, g0), sb_akx(a, g1));
  const int amax = straddle ? max(a.Kx, a.nkx - a.Kx - 1) : max(sb_akx(a, g0), sb_akx(a, g1));
  const int nb = amax - amin + 1;  // <= i1 - i0 <= kSbKxMax
  const unsigned need = inputs(a, SIX);
  const double U = y < a.N ? a.U[y] : 0.0;
  const double dU = (STAGE == 0 && y < a.N) ? a.dU[y] : 0.0;
  for (int i = tid; i < nb * (NS + 1); i += kSbNT) acc[i] = 0.0;
  __syncthreads();
  double s[V][NR];
#pragma unroll
  for (int u = 0; u < V; ++u)
#pragma unroll
    for (int q = 0; q < NR; ++q) s[u][q] = 0.0;
  for (int i = i0; i < i1; ++i) {
    const int ig = a.kx0 + i;
    const int kx = signed_kx(a, i);
    double t[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) t[q] = 0.0;
    if (live) {
      const size_t rb = base + static_cast<size_t>(i) * rowlen;
      Vec<T2, V> v[6], vh[3], vp;
#pragma unroll
      for (int f = 0; f < 6; ++f)
        if ((need >> f) & 1u) v[f] = load<T2, V>(a.f[f], rb, eoff);
#pragma unroll
      for (int f = 0; f < (STAGE == 0 ? 3 : 1); ++f) vh[f] = load<T2, V>(a.h[f], rb, eoff);
      if (STAGE == 1) vp = load<T2, V>(a.p, rb, eoff);
      const double al = a.ax * kx;
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const int kl = kl0 + u, kz = a.kz0 + kl;
        if (kl >= a.nkz_loc || (kx == 0 && kz == 0)) continue;
        const double be = mode_of(a, kz).be, wgt = mode_of(a, kz).wgt;
        Comp m;
        components<SIX>(m, v, u, a.combine, al, be);
        const C cu = m.u, cv = m.v, cw = m.w;
        double c[NR];
        if constexpr (STAGE == 0) {
          const C ox = m.ox, oy = m.oy, oz = m.oz;
          // H' = H - H_lin, H_lin = (-U' v, U' u - U omega_z, U omega_y)
          C hx = widen(vh[0].c[u]), hy = widen(vh[1].c[u]), hz = widen(vh[2].c[u]);
          hx.x += dU * cv.x;
          hx.y += dU * cv.y;
          hy.x -= dU * cu.x - U * oz.x;
          hy.y -= dU * cu.y - U * oz.y;
          hz.x -= U * oy.x;
          hz.y -= U * oy.y;
          const double k2 = al * al + be * be;
          // D u = i al v - omega_z, D w = omega_x + i be v, D v = -i (al u + be w)
          const C du{-al * cv.y - oz.x, al * cv.x - oz.y};
          const C dw{ox.x - be * cv.y, ox.y + be * cv.x};
          const C dv{al * cu.y + be * cw.y, -(al * cu.x + be * cw.x)};
          c[0] = wgt * dot(cu, hx);
          c[1] = wgt * dot(cv, hy);
          c[2] = wgt * dot(cw, hz);
          c[3] = wgt * (dot(cu, hy) + dot(cv, hx));
          c[4] = wgt * (k2 * sq(cu) + sq(du));
          c[5] = wgt * (k2 * sq(cv) + sq(dv));
          c[6] = wgt * (k2 * sq(cw) + sq(dw));
          c[7] = wgt * (k2 * dot(cu, cv) + dot(du, dv));
        } else {
          const C oz = m.oz;
          // G = Pi - U u; strain factors: i al u, D v = -i (al u + be w), i be w, D u + i al v = 2 i al v - omega_z
          C g = widen(vh[0].c[u]);
          g.x -= U * cu.x;
          g.y -= U * cu.y;
          const C cp = widen(vp.c[u]);
          const C sxx{-al * cu.y, al * cu.x};
          const C szz{-be * cw.y, be * cw.x};
          const C syy{al * cu.y + be * cw.y, -(al * cu.x + be * cw.x)};
          const C sxy{-2.0 * al * cv.y - oz.x, 2.0 * al * cv.x - oz.y};
          c[0] = wgt * 2.0 * dot(g, sxx);
          c[1] = wgt * 2.0 * dot(g, syy);
          c[2] = wgt * 2.0 * dot(g, szz);
          c[3] = wgt * dot(g, sxy);
          c[4] = wgt * dot(g, cu);
          c[5] = wgt * dot(g, cv);
          c[NR - 6] = wgt * 2.0 * dot(cp, sxx);
          c[NR - 5] = wgt * 2.0 * dot(cp, syy);
          c[NR - 4] = wgt * 2.0 * dot(cp, szz);
          c[NR - 3] = wgt * dot(cp, sxy);
          c[NR - 2] = wgt * dot(cp, cu);
          c[NR - 1] = wgt * dot(cp, cv);
        }
#pragma unroll
        for (int q = 0; q < NR; ++q) {
          s[u][q] += c[q];
          t[q] += c[q];
        }
      }
    }
    // over the lanes of the plane (specwalk.hpp: they differ in bits 1, 2, kLaneBit2, and in the plain
    // layout in the upper bits too)
    constexpr int B2 = kLaneBit2<V, TILED>;
    double* const bin = &acc[(sb_akx(a, ig) - amin) * (NS + 1) + yy * NR];
    {
      double x = sb_scatter8<0, 1, 2, B2>(t, lane);
      const int q = (lane & 1) << 2 | (lane & 2) | ((lane & B2) ? 1 : 0);
      if (!TILED) {
#pragma unroll
        for (int o = 8; o <= 32; o <<= 1) x += __shfl_xor(x, o);
      }
      if (TILED || (lane >> 3) == 0) atomicAdd(&bin[q], x);
    }
    if constexpr (NR == 12) {
      double x = sb_scatter4<NR - 4, 1, 2, B2>(t, lane);
      const int q = NR - 4 + ((lane & 1) << 1 | ((lane & 2) >> 1));
      if (!TILED) {
#pragma unroll
        for (int o = 8; o <= 32; o <<= 1) x += __shfl_xor(x, o);
      }
      if (!(lane & B2) && (TILED || (lane >> 3) == 0)) atomicAdd(&bin[q], x);
    }
  }
  __syncthreads();
  // the |kx| sums: runs of nb bins per (plane, row)
  for (int i = tid; i < NS * nb; i += kSbNT) {
    const int slot = i / nb, b = i - slot * nb;
    const int pl = slot / NR, q = slot - pl * NR;
    const int yo = TILED ? rg * kSpecYBlock + pl : rg;
    if (yo < a.N)
      atomicAdd(&a.ekx[(static_cast<size_t>(ROW0 + q) * a.N + yo) * (a.Kx + 1) + amin + b], acc[b * (NS + 1) + slot]);
  }
  __syncthreads();
  // the kz sums: through LDS as [slot][line of the slice], then runs of ZL lines per (plane, row)
#pragma unroll
  for (int u = 0; u < V; ++u)
#pragma unroll
    for (int q = 0; q < NR; ++q) acc[(yy * NR + q) * (ZL + 1) + kll + u] = s[u][q];
  __syncthreads();
  for (int i = tid; i < NS * ZL; i += kSbNT) {
    const int slot = i / ZL, k = i - slot * ZL;
    const int pl = slot / NR, q = slot - pl * NR;
    const int yo = TILED ? rg * kSpecYBlock + pl : rg;
    const int kl = zs * ZL + k;
    if (yo < a.N && kl < a.nkz_loc)
      atomicAdd(&a.ekz[(static_cast<size_t>(ROW0 + q) * a.N + yo) * a.nkz + a.kz0 + kl], acc[slot * (ZL + 1) + k]);
  }
}

template <typename T2, int V, bool TILED>
void sbudget_launch(const SBudgetArgs& a, hipStream_t s) {
  constexpr int ZL = TILED ? 4 * kSpecKzBlock * V : kSbNT;
  const long long lines = static_cast<long long>(a.nkx_loc) * a.nkzs;
  const long long span = TILED ? kSpecYBlock * lines : lines;
  CH_CHECK(span + kSbNT * V < (1LL << 31), "sbudget: row group too long for one launch");
  const int rgs = TILED ? (a.N + kSpecYBlock - 1) / kSpecYBlock : a.N;
  const int nzs = ((TILED ? a.nkzs : a.nkz_loc) + ZL - 1) / ZL;
  // kx rows per block: what gives about kSbBlocks blocks, within [kSbKxMin, kSbKxMax]
  const long long fair = (static_cast<long long>(a.nkx_loc) * rgs * nzs + kSbBlocks - 1) / kSbBlocks;
  const int want = static_cast<int>(std::min<long long>(kSbKxMax, std::max<long long>(kSbKxMin, fair)));
  const int nxs0 = (a.nkx_loc + want - 1) / want;
  const int kxs = (a.nkx_loc + nxs0 - 1) / nxs0;  // (evened out over the slices)
  const int nxs = (a.nkx_loc + kxs - 1) / kxs;
  CH_CHECK(kxs >= 1 && kxs <= kSbKxMax && nxs <= 65535, "sbudget: bad kx slices");
  const dim3 grid(static_cast<unsigned>(nzs), static_cast<unsigned>(rgs), static_cast<unsigned>(nxs));
  if (a.stage == 0) hipLaunchKernelGGL((sbudget_kernel<T2, V, TILED, 0>), grid, dim3(kSbNT), 0, s, a, kxs);
  else hipLaunchKernelGGL((sbudget_kernel<T2, V, TILED, 1>), grid, dim3(kSbNT), 0, s, a, kxs);
}

}  // namespace

void sbudget_accumulate(const SBudgetArgs& a, bool fp64, hipStream_t s) {
  CH_CHECK(a.Kx >= 0 && a.nkx == 2 * a.Kx + 1 && a.kx0 >= 0 && a.kx0 + a.nkx_loc <= a.nkx, "sbudget: bad kx range");
  CH_CHECK(a.kz0 >= 0 && a.kz0 + a.nkz_loc <= a.nkz, "sbudget: bad kz range");
  CH_CHECK(a.stage == 0 || a.stage == 1, "sbudget: bad stage");
  const int nh = a.stage == 0 ? 3 : 1;
  bool hal16 = true;
  for (int f = 0; f < nh; ++f) {
    CH_CHECK(a.h[f], "sbudget: missing field h[" << f << "]");
    hal16 = hal16 && reinterpret_cast<uintptr_t>(a.h[f]) % 16 == 0;
  }
  CH_CHECK(a.U && (a.stage == 1 || a.dU) && (a.stage == 0) == (a.p == nullptr), "sbudget: bad stage inputs");
  const unsigned six = a.stage == 0 ? kAll : (kU | kV | kW | kOz);
  dispatch(a, fp64, six, a.ekx && a.ekz, "sbudget", s, [&](auto i) {
    using I = decltype(i);
    // (16-byte loads need h aligned like the fields)
    if (I::V == 2 && !hal16) sbudget_launch<typename I::T2, 1, I::TILED>(a, s);
    else sbudget_launch<typename I::T2, I::V, I::TILED>(a, s);
  });
}

}  // namespace channel
