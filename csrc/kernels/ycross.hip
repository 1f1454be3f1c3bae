// Cross-spectra of every plane against a few reference planes (kernels.hpp YCrossArgs): the reduction of
// the plane spectra (yspectra.hip: the same walk of the layouts, weights, masks, slots and flushes) with
// the second factor of every product taken at a reference plane instead of the lane's own.
//
// As in yspectra.hip a block takes one row group (a plane, or an 8-plane chunk of the blocked layout), one
// slice of kz lines and one slice of kx rows, and a lane keeps its (plane, kz) over the kx loop.  Besides
// its own element a lane loads the same (kx, kz) at the reference plane of the same kx sub-block: in the
// blocked layout the V elements of a lane are contiguous there too ([line / 8][y_r % 8][line % 8]), so
// the same 16-byte load serves, and the 8 planes of a chunk read the same reference piece (one 64-byte
// request per wave and field; the reference plane of a block's kx rows stays in cache).  The four
// complex rows are kYSpecRows real ones, (Re, Im) of row q in rows 2 q and 2 q + 1.  The kz sums take e
// as it is; the |kx| sums take e of kx > 0, conj(e) of kx < 0 and Re e of kx = 0 (whose -kz twin has
// kx = 0 too), i.e. the sign of kx on the imaginary rows, which is uniform over a block iteration.
// The reference planes are a grid factor, the fastest one, so the blocks that read the same rows
// against different reference planes are dispatched together; each has its own sums.
#include "specwalk.hpp"

namespace channel {

namespace {

using namespace specwalk;
constexpr int kYcNT = kNT, kYcBlocks = kBlocks;
constexpr int kYcKxMax = 64, kYcKxMin = 8;  // kx rows per block (yspectra.hip)
constexpr int kYcSlots = 64;                // (plane of the chunk, row) pairs
constexpr int kYcLds = kYcKxMax * (kYcSlots + 1);  // doubles; also holds the kz sums, [slot][lines + 1]

// Sum of t[q] over the 8 lanes that differ in the lane bits M0, M1, M2: the lane with bits (b0, b1,
// b2) returns row 4 b0 + 2 b1 + b2 (yspectra.hip).
template <int M0, int M1, int M2>
__device__ __forceinline__ double yc_reduce_scatter(const double (&t)[kYSpecRows], int lane) {
  const bool b0 = lane & M0, b1 = lane & M1, b2 = lane & M2;
  double a[4], b[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = (b0 ? t[j + 4] : t[j]) + __shfl_xor(b0 ? t[j] : t[j + 4], M0);
#pragma unroll
  for (int j = 0; j < 2; ++j) b[j] = (b1 ? a[j + 2] : a[j]) + __shfl_xor(b1 ? a[j] : a[j + 2], M1);
  return (b2 ? b[1] : b[0]) + __shfl_xor(b2 ? b[0] : b[1], M2);
}

__device__ __forceinline__ int yc_akx(const YCrossArgs& a, int ig) { return ig <= a.Kx ? ig : a.nkx - ig; }

// The row sets: kOwn, the components read at the lane's plane, kRef, those read at the reference plane,
// and the four (first factor, conjugated second factor) pairs.
template <int SET>
struct RowSet;
template <>
struct RowSet<kYCrossVelocity> {
  static constexpr unsigned kOwn = kU | kV | kW, kRef = kU | kV | kW;
  __device__ static __forceinline__ void pairs(const Comp& m, const Comp& r, C (&x)[4], C (&y)[4]) {
    x[0] = m.u, y[0] = r.u;
    x[1] = m.v, y[1] = r.v;
    x[2] = m.w, y[2] = r.w;
    x[3] = m.u, y[3] = r.v;
  }
};
template <>
struct RowSet<kYCrossShear> {
  static constexpr unsigned kOwn = kU | kV | kW | kOz, kRef = kOx | kOz;
  __device__ static __forceinline__ void pairs(const Comp& m, const Comp& r, C (&x)[4], C (&y)[4]) {
    x[0] = m.u, y[0] = r.oz;
    x[1] = m.v, y[1] = r.oz;
    x[2] = m.w, y[2] = r.ox;
    x[3] = m.oz, y[3] = r.oz;
  }
};

template <typename T2, int V, bool TILED, int SET>
__global__ void __launch_bounds__(kYcNT) ycross_kernel(YCrossArgs a, int kxs) {
  using RS = RowSet<SET>;
  constexpr int ZL = TILED ? 4 * kSpecKzBlock * V : kYcNT;  // kz lines per slice
  constexpr int NS = TILED ? kYcSlots : kYSpecRows;          // slots in use
  static_assert(kYSpecRows == 8 && kSpecYBlock * kYSpecRows == kYcSlots, "slots are (plane of the chunk, row)");
  static_assert(NS * (ZL + 1) <= kYcLds, "the kz sums are staged in the accumulators' LDS");
  __shared__ double acc[kYcLds];
  const int tid = threadIdx.x, lane = tid & 63;
  const int ir = blockIdx.x % a.nref, zs = blockIdx.x / a.nref, rg = blockIdx.y;
  const int yr = a.yref[ir];
  // this lane's plane of the chunk and first line of the slice; the element offset in a kx row
  const int yy = plane_of<V, TILED>(tid);
  const int kll = TILED ? (((tid * V) >> 6) << 3) | ((tid * V) & 7) : tid;
  const int kl0 = zs * ZL + kll;
  const int y = TILED ? rg * kSpecYBlock + yy : rg;
  const int rowlen = TILED ? kSpecYBlock * a.nkzs : a.nkzs;  // elements per kx row of a row group
  const int eoff = TILED ? zs * (kYcNT * V) + tid * V : kl0;
  const size_t base = static_cast<size_t>(rg) * rowlen * a.nkx_loc;
  // the same lines at the reference plane: its row group, and its plane of the chunk in the element offset
  // (= spec_row_off(kzb, lines, yr) + spec_line_off(kzb, i nkzs + kl0) - i rowlen)
  const size_t rbase = static_cast<size_t>(TILED ? yr / kSpecYBlock : yr) * rowlen * a.nkx_loc;
  const int roff = TILED ? ((kl0 >> 3) << 6) | ((yr % kSpecYBlock) << 3) | (kl0 & 7) : kl0;
  const bool live = y < a.N && kl0 < (TILED ? a.nkzs : a.nkz_loc);
  const int i0 = blockIdx.z * kxs, i1 = min(a.nkx_loc, i0 + kxs);
  // |kx| bins of rows i0 .. i1 - 1: global indices 0 .. Kx hold kx >= 0, the rest kx = ig - nkx < 0
  const int g0 = a.kx0 + i0, g1 = a.kx0 + i1 - 1;
  const bool straddle = g0 <= a.Kx && g1 > a.Kx;
  const int amin = min(yc_akx(a, g0), yc_akx(a, g1));
  const int amax = straddle ? max(a.Kx, a.nkx - a.Kx - 1) : max(yc_akx(a, g0), yc_akx(a, g1));
  const int nb = amax - amin + 1;  // <= i1 - i0 <= kYcKxMax
  const unsigned own = inputs(a, RS::kOwn), ref = inputs(a, RS::kRef);
  double* const ckx = a.ckx + static_cast<size_t>(ir) * kYSpecRows * a.N * (a.Kx + 1);
  double* const ckz = a.ckz + static_cast<size_t>(ir) * kYSpecRows * a.N * a.nkz;
  for (int i = tid; i < nb * (kYcSlots + 1); i += kYcNT) acc[i] = 0.0;
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
      const size_t ro = static_cast<size_t>(i) * rowlen;
      Vec<T2, V> v[6], w[6];
#pragma unroll
      for (int f = 0; f < 6; ++f)
        if ((own >> f) & 1u) v[f] = load<T2, V>(a.f[f], base + ro, eoff);
#pragma unroll
      for (int f = 0; f < 6; ++f)
        if ((ref >> f) & 1u) w[f] = load<T2, V>(a.f[f], rbase + ro, roff);
      const double al = a.ax * kx;
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const int kl = kl0 + u, kz = a.kz0 + kl;
        if (kl >= a.nkz_loc || (kx == 0 && kz == 0)) continue;
        const double be = mode_of(a, kz).be, wgt = mode_of(a, kz).wgt;
        Comp m, r;
        components<RS::kOwn>(m, v, u, a.combine, al, be);
        components<RS::kRef>(r, w, u, a.combine, al, be);
        C x[4], z[4];
        RS::pairs(m, r, x, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // x conj(z)
          const double re = wgt * (x[q].x * z[q].x + x[q].y * z[q].y);
          const double im = wgt * (x[q].y * z[q].x - x[q].x * z[q].y);
          s[u][2 * q] += re;
          s[u][2 * q + 1] += im;
          t[2 * q] += re;
          t[2 * q + 1] += im;
        }
      }
    }
    // the |kx| bins take conj(e) of kx < 0 and the real part at kx = 0
    const double sgn = kx > 0 ? 1.0 : (kx < 0 ? -1.0 : 0.0);
#pragma unroll
    for (int q = 0; q < 4; ++q) t[2 * q + 1] *= sgn;
    // over the lanes of the plane (specwalk.hpp: they differ in bits 1, 2, kLaneBit2, and in the plain
    // layout in the upper bits too)
    constexpr int B2 = kLaneBit2<V, TILED>;
    double x = yc_reduce_scatter<1, 2, B2>(t, lane);
    const int q = (lane & 1) << 2 | (lane & 2) | ((lane & B2) ? 1 : 0);
    if (!TILED) {
#pragma unroll
      for (int o = 8; o <= 32; o <<= 1) x += __shfl_xor(x, o);
    }
    if (TILED || (lane >> 3) == 0) atomicAdd(&acc[(yc_akx(a, ig) - amin) * (kYcSlots + 1) + yy * kYSpecRows + q], x);
  }
  __syncthreads();
  // the |kx| sums: runs of nb bins per (plane, row)
  for (int i = tid; i < NS * nb; i += kYcNT) {
    const int slot = i / nb, b = i - slot * nb;
    const int q = slot & 7, yo = TILED ? rg * kSpecYBlock + (slot >> 3) : rg;
    if (yo < a.N) atomicAdd(&ckx[(static_cast<size_t>(q) * a.N + yo) * (a.Kx + 1) + amin + b], acc[b * (kYcSlots + 1) + slot]);
  }
  __syncthreads();
  // the kz sums: through LDS as [slot][line of the slice], then runs of ZL lines per (plane, row)
#pragma unroll
  for (int u = 0; u < V; ++u)
#pragma unroll
    for (int q = 0; q < kYSpecRows; ++q) acc[(yy * kYSpecRows + q) * (ZL + 1) + kll + u] = s[u][q];
  __syncthreads();
  for (int i = tid; i < NS * ZL; i += kYcNT) {
    const int slot = i / ZL, k = i - slot * ZL;
    const int q = slot & 7, yo = TILED ? rg * kSpecYBlock + (slot >> 3) : rg;
    const int kl = zs * ZL + k;
    if (yo < a.N && kl < a.nkz_loc)
      atomicAdd(&ckz[(static_cast<size_t>(q) * a.N + yo) * a.nkz + a.kz0 + kl], acc[slot * (ZL + 1) + k]);
  }
}

template <typename T2, int V, bool TILED>
void ycross_launch(const YCrossArgs& a, hipStream_t s) {
  constexpr int ZL = TILED ? 4 * kSpecKzBlock * V : kYcNT;
  const long long lines = static_cast<long long>(a.nkx_loc) * a.nkzs;
  const long long span = TILED ? kSpecYBlock * lines : lines;
  CH_CHECK(span + kYcNT * V < (1LL << 31), "ycross: row group too long for one launch");
  const int rgs = TILED ? (a.N + kSpecYBlock - 1) / kSpecYBlock : a.N;
  const int nzs = ((TILED ? a.nkzs : a.nkz_loc) + ZL - 1) / ZL;
  // kx rows per block: what gives about kYcBlocks blocks, within [kYcKxMin, kYcKxMax]
  const long long fair = (static_cast<long long>(a.nkx_loc) * rgs * nzs * a.nref + kYcBlocks - 1) / kYcBlocks;
  const int want = static_cast<int>(std::min<long long>(kYcKxMax, std::max<long long>(kYcKxMin, fair)));
  const int nxs0 = (a.nkx_loc + want - 1) / want;
  const int kxs = (a.nkx_loc + nxs0 - 1) / nxs0;  // (evened out over the slices)
  const int nxs = (a.nkx_loc + kxs - 1) / kxs;
  CH_CHECK(kxs >= 1 && kxs <= kYcKxMax && nxs <= 65535, "ycross: bad kx slices");
  const dim3 grid(static_cast<unsigned>(nzs * a.nref), static_cast<unsigned>(rgs), static_cast<unsigned>(nxs));
  if (a.rows == kYCrossVelocity) hipLaunchKernelGGL((ycross_kernel<T2, V, TILED, kYCrossVelocity>), grid, dim3(kYcNT), 0, s, a, kxs);
  else hipLaunchKernelGGL((ycross_kernel<T2, V, TILED, kYCrossShear>), grid, dim3(kYcNT), 0, s, a, kxs);
}

}  // namespace

void ycross_accumulate(const YCrossArgs& a, bool fp64, hipStream_t s) {
  CH_CHECK(a.Kx >= 0 && a.nkx == 2 * a.Kx + 1 && a.kx0 >= 0 && a.kx0 + a.nkx_loc <= a.nkx, "ycross: bad kx range");
  CH_CHECK(a.kz0 >= 0 && a.kz0 + a.nkz_loc <= a.nkz, "ycross: bad kz range");
  CH_CHECK(a.rows == kYCrossVelocity || a.rows == kYCrossShear, "ycross: bad row set");
  CH_CHECK(a.nref >= 1 && a.nref <= kYCrossMaxRefs, "ycross: 1 to " << kYCrossMaxRefs << " reference planes");
  for (int i = 0; i < a.nref; ++i) CH_CHECK(a.yref[i] >= 0 && a.yref[i] < a.N, "ycross: reference plane outside [0, N)");
  const unsigned six = a.rows == kYCrossVelocity ? (kU | kV | kW) : (kU | kV | kW | kOx | kOz);
  dispatch(a, fp64, six, a.ckx && a.ckz, "ycross", s, [&](auto i) {
    using I = decltype(i);
    ycross_launch<typename I::T2, I::V, I::TILED>(a, s);
  });
}

}  // namespace channel
