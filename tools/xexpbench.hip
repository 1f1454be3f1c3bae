// Access patterns of the transform stage on the x-expanded intermediates, alone: no LDS traffic, no
// transforms, only the global loads and stores of the three kernels of one y chunk with their lane
// maps, tile orders, grids and LDS footprints (so two of them share a CU as the real ones do):
//   xb  the x-backward's store (K-SPEC's six outputs, as the headline grid runs: a tile = 2 planes x
//       8 kz of one field, 512 threads, lanes 0-3 / 4-7 of an x row = the 64-B piece of plane y /
//       y + 1; 6 fields written)
//   z   the z stage's rows (one wave per (y, x) row, lane t takes k = t + 64 i, 4 rows per block;
//       6 fields read, 3 written in place)
//   xf  the x-forward's load (a tile = 2 planes x 8 kz of one field, quad lane map; 3 fields read)
// over the candidate layouts of a chunk [6 planes][NX = 1024][nkz = 342] of complex fp32:
//   p342        [y][x][kz], row pitch nkz (the layout of CHANNEL_XEXP_LAYOUT=0)
//   p344, p352  the same with the pitch rounded up to 8 / 16 elements
//   p344n, p352n  ... and the x kernels' tile order changed so that the two kz-neighbour tiles that
//               share a 128-B line get consecutive indices
//   t8x8        [y][x/8][kz/8][x%8][kz%8]
// Each case runs alone and in the pairs the two chunk streams co-run (two streams, two chunk
// buffers), REPS times; the table gives the minimum, median and maximum TB/s of each.
// Build: hipcc --offload-arch=gfx950 -O3 tools/xexpbench.hip -o bin/xexpbench
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                   \
  do {                                                          \
    hipError_t e = (x);                                         \
    if (e != hipSuccess) {                                      \
      std::printf("%s failed: %s\n", #x, hipGetErrorString(e)); \
      std::exit(1);                                             \
    }                                                           \
  } while (0)

constexpr int NX = 1024, NKZ = 342, NKB = (NKZ + 7) / 8, NYC = 6;
constexpr int kMaxPitch = 352;
constexpr size_t kFieldElems = static_cast<size_t>(NYC) * NX * kMaxPitch;  // covers every layout

__device__ __forceinline__ unsigned xcd_remap(unsigned b, unsigned n) {
  const unsigned per = n / 8, rem = n % 8, x = b % 8, k = b / 8;
  return (x < rem ? x * (per + 1) : rem * (per + 1) + (x - rem) * per) + k;
}

// byte offset of element (y, x, kz) of a field
template <int P>
struct Lin {
  static __device__ __forceinline__ unsigned off(int y, int x, int kz) {
    return (static_cast<unsigned>(y * NX + x) * P + static_cast<unsigned>(kz)) * 8u;
  }
};
struct T88 {
  static __device__ __forceinline__ unsigned off(int y, int x, int kz) {
    return ((static_cast<unsigned>(y * (NX / 8) + x / 8) * NKB + static_cast<unsigned>(kz / 8)) * 64u +
            static_cast<unsigned>((x % 8) * 8 + kz % 8)) * 8u;
  }
};

// tile t -> (field or group f, first plane y, kz block kb); false: no such tile
// ORD = 0: planes fastest, then kz blocks, then fields (the x kernels' decode());
// ORD = 1: the two kz blocks of a 128-B line fastest, then planes, then line pairs, then fields
template <int ORD>
__device__ __forceinline__ bool decode(int t, int nyt, int& f, int& yt, int& kb) {
  if (ORD == 0) {
    yt = t % nyt;
    const int rest = t / nyt;
    kb = rest % NKB;
    f = rest / NKB;
    return true;
  }
  constexpr int NP = (NKB + 1) / 2;
  const int b = t & 1;
  int rest = t >> 1;
  yt = rest % nyt;
  rest /= nyt;
  kb = 2 * (rest % NP) + b;
  f = rest / NP;
  return kb < NKB;
}
template <int ORD>
__host__ __device__ constexpr int tiles(int nyt, int nf) {
  return ORD == 0 ? nyt * NKB * nf : 2 * nyt * ((NKB + 1) / 2) * nf;
}

extern __shared__ char lds_pad[];  // the real kernels' LDS footprint: it sets who shares a CU

__device__ __forceinline__ float4& at_byte(float2* base, unsigned off) {
  return *reinterpret_cast<float4*>(reinterpret_cast<char*>(base) + off);
}

// x-backward, six-output mode: one field per tile, LDS->global lane map (8 lanes per x row: 2 planes
// x 4 kz pairs)
template <class L, int ORD>
__global__ void __launch_bounds__(512) xb_store(float2* phys, float2* sink) {
  const int tid = threadIdx.x, G = gridDim.x;
  constexpr int NYT = (NYC + 1) / 2;
  const int ntiles = tiles<ORD>(NYT, 6);
  for (int t = static_cast<int>(xcd_remap(blockIdx.x, gridDim.x)); t < ntiles; t += G) {
    int f, yt, kb;
    if (!decode<ORD>(t, NYT, f, yt, kb)) continue;
    for (int e = tid; e < NX * 8; e += 512) {
      const int x = e / 8, c = (e % 8) * 2;
      const int kz = kb * 8 + c % 8, yy = yt * 2 + c / 8;
      if (kz < NKZ && yy < NYC) at_byte(phys + f * kFieldElems, L::off(yy, x, kz)) = float4{1.f * x, 0.f, 1.f * kz, 0.f};
    }
  }
  if (sink == phys) lds_pad[tid] = 0;
}

// x-forward: quad lane map (4 lanes = one plane's 64-B piece, planes in the two half-waves)
template <class L, int ORD>
__global__ void __launch_bounds__(512) xf_load(float2* phys, float2* sink) {
  const int tid = threadIdx.x, G = gridDim.x;
  constexpr int NYT = (NYC + 1) / 2;
  const int ntiles = tiles<ORD>(NYT, 3);
  const int qc = ((tid & 3) | ((tid >> 3) & 4)) * 2, qr = ((tid >> 2) & 7) | ((tid >> 6) << 3);
  float4 acc{0.f, 0.f, 0.f, 0.f};
  for (int t = static_cast<int>(xcd_remap(blockIdx.x, gridDim.x)); t < ntiles; t += G) {
    int f, yt, kb;
    if (!decode<ORD>(t, NYT, f, yt, kb)) continue;
    const int kz = min(kb * 8 + qc % 8, NKZ - 2), yy = min(yt * 2 + qc / 8, NYC - 1);
    float4 v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = at_byte(phys + f * kFieldElems, L::off(yy, qr + q * 64, kz));
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      acc.x += v[q].x;
      acc.y += v[q].y;
      acc.z += v[q].z;
      acc.w += v[q].w;
    }
  }
  if (sink) *reinterpret_cast<float4*>(sink + 2 * (blockIdx.x * 512 + tid)) = acc;
}

// z stage: 4 rows per block, persistent over row groups; three field pairs read, fields 0..2 written
template <class L>
__global__ void __launch_bounds__(256) z_rows(float2* phys, float2* sink) {
  const int tid = threadIdx.x, t = tid & 63, w = tid >> 6;
  constexpr int ngroups = NYC * NX / 4, MK = (NKZ + 63) / 64;
  float2 acc{0.f, 0.f};
  for (int g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int r = g * 4 + w, y = r / NX, x = r % NX;
    float2 v[6][MK];
#pragma unroll
    for (int f = 0; f < 6; ++f)
#pragma unroll
      for (int i = 0; i < MK; ++i)
        v[f][i] = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(phys + f * kFieldElems) +
                                                   L::off(y, x, min(t + 64 * i, NKZ - 1)));
#pragma unroll
    for (int i = 0; i < MK; ++i) {
      const int k = t + 64 * i;
      const float2 h0{v[0][i].x + v[3][i].y, v[0][i].y + v[3][i].x}, h1{v[1][i].x + v[4][i].y, v[1][i].y + v[4][i].x},
          h2{v[2][i].x + v[5][i].y, v[2][i].y + v[5][i].x};
      acc.x += h0.x;
      if (k < NKZ) {
        *reinterpret_cast<float2*>(reinterpret_cast<char*>(phys) + L::off(y, x, k)) = h0;
        *reinterpret_cast<float2*>(reinterpret_cast<char*>(phys + kFieldElems) + L::off(y, x, k)) = h1;
        *reinterpret_cast<float2*>(reinterpret_cast<char*>(phys + 2 * kFieldElems) + L::off(y, x, k)) = h2;
      }
    }
  }
  if (sink) sink[blockIdx.x * 256 + tid] = acc;
}

using Kern = void (*)(float2*, float2*);
struct Pat {
  const char* name;
  Kern k;
  int threads, grid, lds;
  double bytes;
};
struct Layout {
  const char* name;
  Pat xb, z, xf;
};

// LDS of the real kernels at the headline instantiation: x tiles 16 x (1024 + 64 + 2) + 1024-point
// twiddles, one block per CU; z stage 4 rows x 1040 + tables + slots, two blocks per CU
constexpr int kLdsX = 150 * 1024, kLdsZ = 44 * 1024;
template <class L, int ORD>
static Layout make(const char* name, int cus) {
  const double fb = static_cast<double>(NYC) * NX * NKZ * 8;
  Layout l;
  l.name = name;
  l.xb = Pat{"xb", xb_store<L, ORD>, 512, std::min(tiles<ORD>((NYC + 1) / 2, 6), cus), kLdsX, 6 * fb};
  l.z = Pat{"z", z_rows<L>, 256, std::min(NYC * NX / 4, 2 * cus), kLdsZ, 9 * fb};
  l.xf = Pat{"xf", xf_load<L, ORD>, 512, std::min(tiles<ORD>((NYC + 1) / 2, 3), cus), kLdsX, 3 * fb};
  for (const Pat* p : {&l.xb, &l.z, &l.xf})
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(p->k), hipFuncAttributeMaxDynamicSharedMemorySize, p->lds));
  return l;
}

static void launch(const Pat& p, float2* buf, hipStream_t s) {
  hipLaunchKernelGGL(p.k, dim3(p.grid), dim3(p.threads), p.lds, s, buf, static_cast<float2*>(nullptr));
}

// TB/s of `inner` back-to-back rounds of a (and b on the second stream and buffer), `reps` times
static void measure(const char* layout, const Pat& a, const Pat* b, float2* buf0, float2* buf1, hipStream_t s0, hipStream_t s1,
                    int reps, int inner) {
  hipEvent_t start, end, e1;
  CK(hipEventCreate(&start));
  CK(hipEventCreate(&end));
  CK(hipEventCreateWithFlags(&e1, hipEventDisableTiming));
  std::vector<double> tb;
  for (int r = -1; r < reps; ++r) {  // (r = -1: warm-up)
    CK(hipEventRecord(start, s0));
    if (b) CK(hipStreamWaitEvent(s1, start, 0));
    for (int i = 0; i < inner; ++i) {
      launch(a, buf0, s0);
      if (b) launch(*b, buf1, s1);
    }
    if (b) {
      CK(hipEventRecord(e1, s1));
      CK(hipStreamWaitEvent(s0, e1, 0));
    }
    CK(hipEventRecord(end, s0));
    CK(hipEventSynchronize(end));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, start, end));
    if (r >= 0) tb.push_back((a.bytes + (b ? b->bytes : 0.0)) * inner / ms / 1e9);
  }
  std::sort(tb.begin(), tb.end());
  char nm[32];
  std::snprintf(nm, sizeof(nm), "%s%s%s", a.name, b ? "+" : "", b ? b->name : "");
  std::printf("%-7s %-6s  min %5.2f  med %5.2f  max %5.2f TB/s  (%.1f us per round)\n", layout, nm, tb.front(), tb[tb.size() / 2],
              tb.back(), (a.bytes + (b ? b->bytes : 0.0)) / tb[tb.size() / 2] / 1e6);
  CK(hipEventDestroy(start));
  CK(hipEventDestroy(end));
  CK(hipEventDestroy(e1));
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? std::atoi(argv[1]) : 5, inner = argc > 2 ? std::atoi(argv[2]) : 20;
  int cus = 0;
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  float2 *buf0, *buf1;
  CK(hipMalloc(&buf0, 6 * kFieldElems * sizeof(float2)));
  CK(hipMalloc(&buf1, 6 * kFieldElems * sizeof(float2)));
  CK(hipMemset(buf0, 0, 6 * kFieldElems * sizeof(float2)));
  CK(hipMemset(buf1, 0, 6 * kFieldElems * sizeof(float2)));
  hipStream_t s0, s1;
  CK(hipStreamCreate(&s0));
  CK(hipStreamCreate(&s1));
  std::printf("chunk %d planes x %d x %d kz, complex fp32, %.1f MB per field, %d CUs, %d reps of %d rounds\n", NYC, NX, NKZ,
              NYC * NX * NKZ * 8 / 1e6, cus, reps, inner);
  const Layout ls[] = {make<Lin<342>, 0>("p342", cus),  make<Lin<344>, 0>("p344", cus),  make<Lin<352>, 0>("p352", cus),
                       make<Lin<344>, 1>("p344n", cus), make<Lin<352>, 1>("p352n", cus), make<T88, 0>("t8x8", cus)};
  for (const Layout& l : ls) {
    measure(l.name, l.xb, nullptr, buf0, buf1, s0, s1, reps, inner);
    measure(l.name, l.z, nullptr, buf0, buf1, s0, s1, reps, inner);
    measure(l.name, l.xf, nullptr, buf0, buf1, s0, s1, reps, inner);
    measure(l.name, l.xb, &l.z, buf0, buf1, s0, s1, reps, inner);
    measure(l.name, l.z, &l.xf, buf0, buf1, s0, s1, reps, inner);
    measure(l.name, l.xb, &l.xf, buf0, buf1, s0, s1, reps, inner);
    measure(l.name, l.z, &l.z, buf0, buf1, s0, s1, reps, inner);
  }
  CK(hipDeviceSynchronize());
  return 0;
}
