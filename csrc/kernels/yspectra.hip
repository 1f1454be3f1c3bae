// One-dimensional spectra and co-spectra at every plane (kernels.hpp YSpectraArgs): the read of the
// gradient sums (gradsum.hip: same fields, walk of the layouts, weights and masks) with a sum kept
// for every (plane, |kx|) and every (plane, kz) instead of one per plane.
//
// A block takes one row group (a plane, kzb = 0, or an 8-plane chunk, kzb = 8), one slice of kz
// lines and one slice of kx rows, and loops over its kx.  In the blocked layout the 8 planes x nkzs
// lines of one kx row are contiguous, [line / 8][y % 8][line % 8], and a block iteration covers
// 256 V consecutive elements of it (V complex per lane: 16-byte loads in fp32 when the fields are
// 16-byte aligned), i.e. 8 planes x 32 V lines; in the plain layout it covers 256 lines of one plane.
// So a lane keeps its (plane, kz) over the whole kx loop:
//  * its kYSpecRows products per element are summed over kx in registers and leave once at the end;
//  * per kx the products are summed over the lanes of the same plane with a reduce-scatter of
//    shuffles (7 instead of 3 per row: every lane ends with one (plane, row) sum of its wave) and
//    over the block's waves by LDS atomics into one accumulator per (|kx| bin of the slice, plane, row).
// Both sets leave the block through LDS as contiguous runs: one atomicAdd per (row, plane, bin) and
// block, consecutive lanes on consecutive bins.  Padded planes (y >= N) and lines past the line
// stride are not loaded; padded kz lines (kl >= nkz_loc) are loaded with their piece and masked.
#include "specwalk.hpp"

namespace channel {

namespace {

using namespace specwalk;
constexpr int kYsNT = kNT, kYsBlocks = kBlocks;  // threads per block, blocks per launch aimed at, as the gradient sums
// kx rows per block: at most kYsKxMax (the LDS accumulators: one per bin, plane and row), at least
// kYsKxMin where there are as many (the kz sums leave a block once, 8 atomics per element, whatever
// the number of rows it has read)
constexpr int kYsKxMax = 64, kYsKxMin = 8;
constexpr int kYsSlots = 64;      // (plane of the chunk, row) pairs
constexpr int kYsLds = kYsKxMax * (kYsSlots + 1);  // doubles; also holds the kz sums, [slot][lines + 1]

// Sum of t[q] over the 8 lanes that differ in the lane bits M0, M1, M2: the lane with bits (b0, b1,
// b2) returns row 4 b0 + 2 b1 + b2.
template <int M0, int M1, int M2>
__device__ __forceinline__ double ys_reduce_scatter(const double (&t)[kYSpecRows], int lane) {
  const bool b0 = lane & M0, b1 = lane & M1, b2 = lane & M2;
  double a[4], b[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = (b0 ? t[j + 4] : t[j]) + __shfl_xor(b0 ? t[j] : t[j + 4], M0);
#pragma unroll
  for (int j = 0; j < 2; ++j) b[j] = (b1 ? a[j + 2] : a[j]) + __shfl_xor(b1 ? a[j] : a[j + 2], M1);
  return (b2 ? b[1] : b[0]) + __shfl_xor(b2 ? b[0] : b[1], M2);
}

__device__ __forceinline__ int ys_akx(const YSpectraArgs& a, int ig) { return ig <= a.Kx ? ig : a.nkx - ig; }

template <typename T2, int V, bool TILED>
__global__ void __launch_bounds__(kYsNT) yspectra_kernel(YSpectraArgs a, int kxs) {
  constexpr int ZL = TILED ? 4 * kSpecKzBlock * V : kYsNT;  // kz lines per slice
  constexpr int NS = TILED ? kYsSlots : kYSpecRows;          // slots in use
  static_assert(kYSpecRows == 8 && kSpecYBlock * kYSpecRows == kYsSlots, "slots are (plane of the chunk, row)");
  static_assert(NS * (ZL + 1) <= kYsLds, "the kz sums are staged in the accumulators' LDS");
  __shared__ double acc[kYsLds];
  const int tid = threadIdx.x, lane = tid & 63;
  const int zs = blockIdx.x, rg = blockIdx.y;
  // this lane's plane of the chunk and first line of the slice; the element offset in a kx row
  const int yy = plane_of<V, TILED>(tid);
  const int kll = TILED ? (((tid * V) >> 6) << 3) | ((tid * V) & 7) : tid;
  const int kl0 = zs * ZL + kll;
  const int y = TILED ? rg * kSpecYBlock + yy : rg;
  const int rowlen = TILED ? kSpecYBlock * a.nkzs : a.nkzs;  // elements per kx row of the row group
  const int eoff = TILED ? zs * (kYsNT * V) + tid * V : kl0;
  const size_t base = static_cast<size_t>(rg) * rowlen * a.nkx_loc;
  const bool live = y < a.N && kl0 < (TILED ? a.nkzs : a.nkz_loc);
  const int i0 = blockIdx.z * kxs, i1 = min(a.nkx_loc, i0 + kxs);
  // |kx| bins of rows i0 .. i1 - 1: global indices 0 .. Kx hold kx >= 0, the rest kx = ig - nkx < 0
  const int g0 = a.kx0 + i0, g1 = a.kx0 + i1 - 1;
  const bool straddle = g0 <= a.Kx && g1 > a.Kx;
  const int amin = min(ys_akx(a, g0), ys_akx(a, g1));
  const int amax = straddle ? max(a.Kx, a.nkx - a.Kx - 1) : max(ys_akx(a, g0), ys_akx(a, g1));
  const int nb = amax - amin + 1;  // <= i1 - i0 <= kYsKxMax
  const unsigned need = inputs(a, kAll);
  const bool hasp = a.p != nullptr;
  for (int i = tid; i < nb * (kYsSlots + 1); i += kYsNT) acc[i] = 0.0;
  __syncthreads();
  double s[V][kYSpecRows];
#pragma unroll
  for (int u = 0; u < V; ++u)
#pragma unroll
    for (int q = 0; q < kYSpecRows; ++q) s[u][q] = 0.0;
  for (int i = i0; i < i1; ++i) {
    const int ig = a.kx0 + i;
    const int kx = signed_kx(a, i);
    double t[kYSpecRows];
#pragma unroll
    for (int q = 0; q < kYSpecRows; ++q) t[q] = 0.0;
    if (live) {
      const size_t rb = base + static_cast<size_t>(i) * rowlen;
      Vec<T2, V> v[6], vp;
#pragma unroll
      for (int f = 0; f < 6; ++f)
        if ((need >> f) & 1u) v[f] = load<T2, V>(a.f[f], rb, eoff);
      if (hasp) vp = load<T2, V>(a.p, rb, eoff);
      const double al = a.ax * kx;
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const int kl = kl0 + u, kz = a.kz0 + kl;
        if (kl >= a.nkz_loc || (kx == 0 && kz == 0)) continue;
        const double be = mode_of(a, kz).be, wgt = mode_of(a, kz).wgt;
        Comp m;
        components<kAll>(m, v, u, a.combine, al, be);
        double c[kYSpecRows];
        c[0] = wgt * sq(m.u);
        c[1] = wgt * sq(m.v);
        c[2] = wgt * sq(m.w);
        c[3] = wgt * (m.u.x * m.v.x + m.u.y * m.v.y);
        c[4] = wgt * sq(m.ox);
        c[5] = wgt * sq(m.oy);
        c[6] = wgt * sq(m.oz);
        c[7] = hasp ? wgt * sq(widen(vp.c[u])) : 0.0;
#pragma unroll
        for (int q = 0; q < kYSpecRows; ++q) {
          s[u][q] += c[q];
          t[q] += c[q];
        }
      }
    }
    // over the lanes of the plane (specwalk.hpp: they differ in bits 1, 2, kLaneBit2, and in the plain
    // layout in the upper bits too)
    constexpr int B2 = kLaneBit2<V, TILED>;
    double x = ys_reduce_scatter<1, 2, B2>(t, lane);
    const int q = (lane & 1) << 2 | (lane & 2) | ((lane & B2) ? 1 : 0);
    if (!TILED) {
#pragma unroll
      for (int o = 8; o <= 32; o <<= 1) x += __shfl_xor(x, o);
    }
    if (TILED || (lane >> 3) == 0) atomicAdd(&acc[(ys_akx(a, ig) - amin) * (kYsSlots + 1) + yy * kYSpecRows + q], x);
  }
  __syncthreads();
  // the |kx| sums: runs of nb bins per (plane, row)
  for (int i = tid; i < NS * nb; i += kYsNT) {
    const int slot = i / nb, b = i - slot * nb;
    const int q = slot & 7, yo = TILED ? rg * kSpecYBlock + (slot >> 3) : rg;
    if (yo < a.N && (q < 7 || hasp))
      atomicAdd(&a.ekx[(static_cast<size_t>(q) * a.N + yo) * (a.Kx + 1) + amin + b], acc[b * (kYsSlots + 1) + slot]);
  }
  __syncthreads();
  // the kz sums: through LDS as [slot][line of the slice], then runs of ZL lines per (plane, row)
#pragma unroll
  for (int u = 0; u < V; ++u)
#pragma unroll
    for (int q = 0; q < kYSpecRows; ++q) acc[(yy * kYSpecRows + q) * (ZL + 1) + kll + u] = s[u][q];
  __syncthreads();
  for (int i = tid; i < NS * ZL; i += kYsNT) {
    const int slot = i / ZL, k = i - slot * ZL;
    const int q = slot & 7, yo = TILED ? rg * kSpecYBlock + (slot >> 3) : rg;
    const int kl = zs * ZL + k;
    if (yo < a.N && kl < a.nkz_loc && (q < 7 || hasp))
      atomicAdd(&a.ekz[(static_cast<size_t>(q) * a.N + yo) * a.nkz + a.kz0 + kl], acc[slot * (ZL + 1) + k]);
  }
}

template <typename T2, int V, bool TILED>
void yspectra_launch(const YSpectraArgs& a, hipStream_t s) {
  constexpr int ZL = TILED ? 4 * kSpecKzBlock * V : kYsNT;
  const long long lines = static_cast<long long>(a.nkx_loc) * a.nkzs;
  const long long span = TILED ? kSpecYBlock * lines : lines;
  CH_CHECK(span + kYsNT * V < (1LL << 31), "yspectra: row group too long for one launch");
  const int rgs = TILED ? (a.N + kSpecYBlock - 1) / kSpecYBlock : a.N;
  const int nzs = ((TILED ? a.nkzs : a.nkz_loc) + ZL - 1) / ZL;
  // kx rows per block: what gives about kYsBlocks blocks, within [kYsKxMin, kYsKxMax]
  const long long fair = (static_cast<long long>(a.nkx_loc) * rgs * nzs + kYsBlocks - 1) / kYsBlocks;
  const int want = static_cast<int>(std::min<long long>(kYsKxMax, std::max<long long>(kYsKxMin, fair)));
  const int nxs0 = (a.nkx_loc + want - 1) / want;
  const int kxs = (a.nkx_loc + nxs0 - 1) / nxs0;  // (evened out over the slices)
  const int nxs = (a.nkx_loc + kxs - 1) / kxs;
  CH_CHECK(kxs >= 1 && kxs <= kYsKxMax && nxs <= 65535, "yspectra: bad kx slices");
  hipLaunchKernelGGL((yspectra_kernel<T2, V, TILED>),
                     dim3(static_cast<unsigned>(nzs), static_cast<unsigned>(rgs), static_cast<unsigned>(nxs)), dim3(kYsNT), 0,
                     s, a, kxs);
}

}  // namespace

void yspectra_accumulate(const YSpectraArgs& a, bool fp64, hipStream_t s) {
  CH_CHECK(a.Kx >= 0 && a.nkx == 2 * a.Kx + 1 && a.kx0 >= 0 && a.kx0 + a.nkx_loc <= a.nkx, "yspectra: bad kx range");
  CH_CHECK(a.kz0 >= 0 && a.kz0 + a.nkz_loc <= a.nkz, "yspectra: bad kz range");
  dispatch(a, fp64, kAll, a.ekx && a.ekz, "yspectra", s, [&](auto i) {
    using I = decltype(i);
    yspectra_launch<typename I::T2, I::V, I::TILED>(a, s);
  });
}

}  // namespace channel
