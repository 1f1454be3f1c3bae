// The walk of the spectral fields shared by the all-plane reductions outside the step (kernels.hpp
// SpecWalkArgs: gradsum.hip, pstrain.hip, yspectra.hip): the layouts, the element decode, the six
// velocity and vorticity components of either K-SPEC mode, the lanes of a plane, and for the plane
// sums the whole kernel around an operation's per-element body.
//
// A row group is what the layout stores contiguously: one plane of `lines` elements (kzb = 0) or an
// 8-plane chunk of 8 * lines elements ordered [line / 8][y % 8][line % 8] (kzb = 8).  Consecutive
// lanes take consecutive elements, so a wave's accesses are whole 64-byte [y % 8][line % 8] pieces;
// in the blocked fp32 layout each lane takes two complex elements per field (16-byte loads; the
// pieces are 64-byte aligned).  A block's stride is a multiple of 64 elements, so a lane stays on
// one plane of the chunk.  Padded planes (y >= N) are not loaded; padded kz lines are loaded with
// their piece and masked (they are not assumed to be zero).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "channel/common.hpp"
#include "channel/kernels.hpp"

namespace channel {
namespace specwalk {

constexpr int kNT = 256;         // threads per block
constexpr int kBlocks = 2048;    // blocks per launch aimed at (8 per CU)

template <typename T2, int V>
struct alignas(sizeof(T2) * V) Vec {
  T2 c[V];
};

struct C {
  double x, y;
};
__device__ __forceinline__ double sq(C a) { return a.x * a.x + a.y * a.y; }
// Re(a conj b)
__device__ __forceinline__ double dot(C a, C b) { return a.x * b.x + a.y * b.y; }
template <typename T2>
__device__ __forceinline__ C widen(T2 v) {
  return C{static_cast<double>(v.x), static_cast<double>(v.y)};
}

// ---- fields ---------------------------------------------------------------------------------
// Components as bits of a mask, in the six-output order of SpecWalkArgs::f.
enum : unsigned { kU = 1, kV = 2, kW = 4, kOx = 8, kOy = 16, kOz = 32, kAll = 63 };
// the combine-mode inputs (bits of D1 v, v, D1 omega, omega, phi) that form the components `six`
constexpr unsigned cmb_inputs(unsigned six) {
  return ((six & (kU | kW)) ? 1u | 8u : 0u) | ((six & kV) ? 2u : 0u) | ((six & (kOx | kOz)) ? 4u | 16u : 0u) |
         ((six & kOy) ? 8u : 0u);
}
__host__ __device__ inline unsigned inputs(const SpecWalkArgs& a, unsigned six) { return a.combine ? cmb_inputs(six) : six; }

// (base is uniform over the block and e a lane's 32-bit offset: one scalar base per field)
template <typename T2, int V>
__device__ __forceinline__ Vec<T2, V> load(const void* q, size_t base, int e) {
  return *reinterpret_cast<const Vec<T2, V>*>(static_cast<const T2*>(q) + base + e);
}

struct Comp {
  C u, v, w, ox, oy, oz;
};
// The components SIX of element u of the loaded vectors, at (al, be) off the mean line; the others
// are zero or unset and cost nothing.  (Filled in place, in this order of statements: returned by value,
// or with the loads grouped by component, the two-element spectra kernel takes 135 VGPRs, over the 128
// of four waves per SIMD.)
template <unsigned SIX, typename VecT>
__device__ __forceinline__ void components(Comp& c, const VecT (&v)[6], int u, int combine, double al, double be) {
  if (SIX & kV) c.v = widen(v[1].c[u]);
  if (combine) {
    // u = i (al D1v - be om) / k2, w = i (be D1v + al om) / k2, omega_x = i (be phi + al D1om) / k2,
    // omega_z = i (be D1om - al phi) / k2 (COMPAT.md "combine mode"; fft_impl.hpp cmb_pair)
    const double r = 1.0 / (al * al + be * be);
    const C d = (SIX & (kU | kW)) ? widen(v[0].c[u]) : C{};
    const C dom = (SIX & (kOx | kOz)) ? widen(v[2].c[u]) : C{};
    const C ph = (SIX & (kOx | kOz)) ? widen(v[4].c[u]) : C{};
    const C om = (SIX & (kU | kW | kOy)) ? widen(v[3].c[u]) : C{};
    c.oy = om;
    c.u = C{-(al * d.y - be * om.y) * r, (al * d.x - be * om.x) * r};
    c.w = C{-(be * d.y + al * om.y) * r, (be * d.x + al * om.x) * r};
    c.ox = C{-(be * ph.y + al * dom.y) * r, (be * ph.x + al * dom.x) * r};
    c.oz = C{-(be * dom.y - al * ph.y) * r, (be * dom.x - al * ph.x) * r};
  } else {
    if (SIX & kU) c.u = widen(v[0].c[u]);
    if (SIX & kW) c.w = widen(v[2].c[u]);
    if (SIX & kOx) c.ox = widen(v[3].c[u]);
    if (SIX & kOy) c.oy = widen(v[4].c[u]);
    if (SIX & kOz) c.oz = widen(v[5].c[u]);
  }
}

// ---- element decode -------------------------------------------------------------------------
__device__ __forceinline__ int signed_kx(const SpecWalkArgs& a, int ikx) {
  const int ig = a.kx0 + ikx;
  return ig <= a.Kx ? ig : ig - a.nkx;
}
// the kx and the first kz line of the access at element e of a row group (the V elements of an access
// share the kx row: blocked lines come in eights and nkzs % 8 == 0)
template <bool TILED>
__device__ __forceinline__ void row_of(const SpecWalkArgs& a, int e, int& kx, int& kl0) {
  const int line = TILED ? ((e >> 6) << 3) | (e & 7) : e;
  const int ikx = line / a.nkzs;
  kl0 = line - ikx * a.nkzs;
  kx = signed_kx(a, ikx);
}
// A kz line kl of row kx is skipped when it is padding or the mean line: kl >= nkz_loc || (kx == 0 &&
// kz == 0).  That test stays an `if` in the two kernel bodies: as a bool-valued helper it compiles to
// other control flow that costs the fp64 blocked plane sums two VGPRs and an occupancy step.
//
// be and the weight of a line that is not skipped: kz = 0 once, kz > 0 twice
struct Mode {
  double be, wgt;
};
__device__ __forceinline__ Mode mode_of(const SpecWalkArgs& a, int kz) { return Mode{a.az * kz, kz == 0 ? 1.0 : 2.0}; }

// ---- the lanes of one plane -----------------------------------------------------------------
// All 64 (plain); lane bits 3..5 select the plane with one element per lane, bits 2..4 with two: the
// lanes of a plane differ in the lane bits of value 1, 2 and kLaneBit2 (and, plain, in all the others).
template <int V, bool TILED>
constexpr int kLaneBit2 = TILED && V == 2 ? 32 : 4;
template <int V, bool TILED>
__device__ __forceinline__ int plane_of(int tid) {
  return TILED ? ((tid * V) >> 3) & 7 : 0;
}
template <int V, bool TILED>
__device__ __forceinline__ void plane_sum(double& x) {  // (in place: a returned value costs two VGPRs)
  if (!TILED) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  } else {
    x += __shfl_xor(x, 1);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, kLaneBit2<V, TILED>);
  }
}

// The block's ROWS sums per plane: over the lanes of a plane with shuffles, over the waves through
// LDS, then one atomicAdd per (plane, row) into sums[ROWS][N].
template <int ROWS, int V, bool TILED>
__device__ __forceinline__ void block_exit(const double (&s)[ROWS], int rg, int yy, int N, double* sums) {
  constexpr int PG = TILED ? kSpecYBlock : 1;  // planes per row group
  constexpr int NW = kNT / 64;
  __shared__ double red[NW][PG][ROWS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int q = 0; q < ROWS; ++q) {
    double x = s[q];
    plane_sum<V, TILED>(x);
    const bool first = !TILED ? lane == 0 : (lane & (3 | kLaneBit2<V, TILED>)) == 0;
    if (first) red[w][yy][q] = x;
  }
  __syncthreads();
  if (tid < PG * ROWS) {
    const int p = tid / ROWS, q = tid - p * ROWS;
    const int yo = TILED ? rg * kSpecYBlock + p : rg;
    double x = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) x += red[i][p][q];
    if (yo < N) atomicAdd(&sums[static_cast<size_t>(q) * N + yo], x);
  }
}

// ---- plane sums -----------------------------------------------------------------------------
// Op: Args (SpecWalkArgs and sums), kRows, kFields (the components its rows use), kPressure (p is
// read) and accumulate(s, c, cp, al, be, wgt), the sums of one element.  A block walks one slice of
// `seg` elements of a row group; a lane keeps the kRows sums of its plane in registers.
template <typename T2, int V, bool TILED, typename Op>
__global__ void __launch_bounds__(kNT) planesum_kernel(typename Op::Args a, int seg) {
  const int tid = threadIdx.x;
  const int lines = a.nkx_loc * a.nkzs;
  const int span = TILED ? kSpecYBlock * lines : lines;
  const int rg = blockIdx.y;
  const size_t base = static_cast<size_t>(rg) * span;
  const int e0 = blockIdx.x * seg, e1 = min(span, e0 + seg);
  const int yy = plane_of<V, TILED>(tid);
  const int y = TILED ? rg * kSpecYBlock + yy : rg;
  const unsigned need = inputs(a, Op::kFields);
  double s[Op::kRows];
#pragma unroll
  for (int q = 0; q < Op::kRows; ++q) s[q] = 0.0;
  if (y < a.N) {
    for (int e = e0 + tid * V; e < e1; e += kNT * V) {
      Vec<T2, V> v[6], vp;
      if (Op::kPressure) vp = load<T2, V>(a.p, base, e);
#pragma unroll
      for (int f = 0; f < 6; ++f)
        if ((need >> f) & 1u) v[f] = load<T2, V>(a.f[f], base, e);
      int kx, kl0;
      row_of<TILED>(a, e, kx, kl0);
      const double al = a.ax * kx;
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const int kl = kl0 + u, kz = a.kz0 + kl;
        if (kl >= a.nkz_loc || (kx == 0 && kz == 0)) continue;
        const Mode m = mode_of(a, kz);
        Comp c;
        components<Op::kFields>(c, v, u, a.combine, al, m.be);
        Op::accumulate(s, c, Op::kPressure ? widen(vp.c[u]) : C{0.0, 0.0}, al, m.be, m.wgt);
      }
    }
  }
  block_exit<Op::kRows, V, TILED>(s, rg, yy, a.N, a.sums);
}

template <typename T2, int V, bool TILED, typename Op>
void planesum_launch(const typename Op::Args& a, const char* name, hipStream_t s) {
  const long long lines = static_cast<long long>(a.nkx_loc) * a.nkzs;
  const long long span = TILED ? kSpecYBlock * lines : lines;
  CH_CHECK(span + kNT * V < (1LL << 31), name << ": row group too long for one launch");
  const int rgs = TILED ? (a.N + kSpecYBlock - 1) / kSpecYBlock : a.N;
  const long long per = kNT * V;  // elements per block iteration: a multiple of 64
  const long long iters = (span + per - 1) / per;
  const long long want = std::max<long long>(1, std::min<long long>(iters, kBlocks / rgs));
  const long long seg = (iters + want - 1) / want * per;
  const long long nsl = (span + seg - 1) / seg;
  hipLaunchKernelGGL((planesum_kernel<T2, V, TILED, Op>), dim3(static_cast<unsigned>(nsl), static_cast<unsigned>(rgs)),
                     dim3(kNT), 0, s, a, static_cast<int>(seg));
}

// ---- entry checks and dispatch --------------------------------------------------------------
template <typename T2_, int V_, bool TILED_>
struct Inst {
  using T2 = T2_;
  static constexpr int V = V_;
  static constexpr bool TILED = TILED_;
};
// The checks every entry point makes, then launch(Inst<T2, V, TILED>{}) for the layout, the
// precision and the alignment of the fields `six` and of p (16-byte loads in the blocked fp32 layout).
template <typename Launch>
void dispatch(const SpecWalkArgs& a, bool fp64, unsigned six, bool outputs, const char* name, hipStream_t s, Launch&& launch) {
  CH_CHECK(a.N > 0 && a.nkx_loc > 0 && a.nkz_loc > 0 && a.nkzs >= a.nkz_loc && outputs, name << ": empty");
  CH_CHECK(a.kzb == 0 || (a.kzb == kSpecKzBlock && a.nkzs % kSpecKzBlock == 0), name << ": bad spectral layout");
  CH_CHECK(a.N <= 65535, name << ": too many planes");
  const unsigned need = inputs(a, six);
  bool al16 = !a.p || reinterpret_cast<uintptr_t>(a.p) % 16 == 0;
  for (int f = 0; f < 6; ++f) {
    if (!((need >> f) & 1u)) continue;
    CH_CHECK(a.f[f], name << ": missing field " << f);
    al16 = al16 && reinterpret_cast<uintptr_t>(a.f[f]) % 16 == 0;
  }
  if (a.kzb) {
    if (fp64) launch(Inst<double2, 1, true>{});
    else if (al16) launch(Inst<float2, 2, true>{});
    else launch(Inst<float2, 1, true>{});
  } else {
    if (fp64) launch(Inst<double2, 1, false>{});
    else launch(Inst<float2, 1, false>{});
  }
  HIP_LAUNCH_CHECK(s);
}
template <typename Op>
void planesum_accumulate(const typename Op::Args& a, bool fp64, const char* name, hipStream_t s) {
  dispatch(a, fp64, Op::kFields, a.sums && (!Op::kPressure || a.p), name, s, [&](auto i) {
    using I = decltype(i);
    planesum_launch<typename I::T2, I::V, I::TILED, Op>(a, name, s);
  });
}

}  // namespace specwalk
}  // namespace channel
