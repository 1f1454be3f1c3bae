// K-SPEC launcher and its default instantiations (compact D2, discrete Green's functions); the
// kernel is in kspec_impl.hpp, the reference-parity variants in kspec_par*.hip.
#include "kspec_impl.hpp"

namespace channel {

template void kspec_launch_par<0>(const YTablesDev&, const SpecArgs&, bool, hipStream_t, int*);

KspecVariant& kspec_variant_slot() {
  static thread_local KspecVariant v;
  return v;
}
std::string kspec_last_variant() {
  const KspecVariant& v = kspec_variant_slot();
  if (v.R == 0) return "";
  const std::string ty = v.f64 ? "double" : "float";
  std::string s = "kspec_kernel<" + std::to_string(v.R) + ", " + ty;
  for (int x : {v.W, v.NS, v.XM, v.PAR, v.GLM, v.SPLIT, v.H}) s += ", " + std::to_string(x);
  s += ">";
  if (v.W2)
    s += " + kspec_out_kernel<" + std::to_string(v.R) + ", " + ty + ", " + std::to_string(v.W2) + ", " +
         std::to_string(v.XM) + ">";
  return s;
}

// the parity variant's launcher; cap: kspec_launch_t
static void kspec_dispatch_par(const YTablesDev& t, const SpecArgs& a, bool fp64, hipStream_t stream, int* cap) {
  const int par = (a.explicit_dd ? kParDD : 0) | (a.analytic_influence ? kParAnalytic : 0);
  switch (par) {
    case 0: kspec_launch_par<0>(t, a, fp64, stream, cap); break;
    case kParDD: kspec_launch_par<kParDD>(t, a, fp64, stream, cap); break;
    case kParAnalytic: kspec_launch_par<kParAnalytic>(t, a, fp64, stream, cap); break;
    default: kspec_launch_par<kParDD | kParAnalytic>(t, a, fp64, stream, cap); break;
  }
}

void kspec_launch(const YTablesDev& t, const SpecArgs& a, bool fp64, hipStream_t stream) {
  CH_CHECK(a.N == t.tab.N, "kspec: NY mismatch with tables");
  CH_CHECK(!a.analytic_influence || a.ygrid, "kspec: analytic influence needs the y grid");
  CH_CHECK(a.lines > 0, "kspec: no lines");
  CH_CHECK(!a.kzb || (a.kzb == kSpecKzBlock && a.nkz % kSpecKzBlock == 0 && a.lines % kSpecKzBlock == 0),
           "kspec: the blocked spectral layout needs whole 8-line kz blocks");
  CH_CHECK(static_cast<long long>(a.N) * a.lines < (1LL << 32), "kspec: field exceeds 32-bit element offsets");
  kspec_dispatch_par(t, a, fp64, stream, nullptr);
  HIP_LAUNCH_CHECK(stream);
}

int kspec_grid_capacity(const YTablesDev& t, const SpecArgs& a, bool fp64) {
  const KspecVariant keep = kspec_variant_slot();  // (the record of the last launch stays)
  int cap = 0;
  kspec_dispatch_par(t, a, fp64, nullptr, &cap);
  kspec_variant_slot() = keep;
  return cap;
}

// Thread i sums slot i of the workgroups' rows in row order and writes the plane the slot stands
// for: slot (hr 64 + l) of statistic s is row j = (hr / R) HR + l R + hr % R (kspec_kernel; rows
// >= N are padding).  Consecutive threads read consecutive slots of a row.
__global__ void __launch_bounds__(256) kspec_stats_reduce_kernel(const double* __restrict__ part, int stride, int blocks,
                                                                 int R, int H, int N, double* __restrict__ stats) {
  const int ROWS = 64 * R * H, HR = 64 * R;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 4 * ROWS) return;
  const int s = i / ROWS, rem = i - s * ROWS, hr = rem / 64, l = rem - hr * 64;
  const int j = (hr / R) * HR + l * R + hr % R;
  if (j >= N) return;
  const double* p = part + i;
  double sum = 0.0;
#pragma unroll 8
  for (int b = 0; b < blocks; ++b) sum += p[static_cast<size_t>(b) * stride];
  stats[s * N + j] = sum;
}

void kspec_stats_reduce(const YTablesDev& t, const double* part, int stride, int blocks, double* stats, hipStream_t stream) {
  const int slots = 4 * 64 * t.R * t.H;
  CH_CHECK(part && stats && blocks > 0 && stride >= slots, "kspec_stats_reduce: partial buffer");
  hipLaunchKernelGGL(kspec_stats_reduce_kernel, dim3((slots + 255) / 256), dim3(256), 0, stream, part, stride, blocks, t.R, t.H,
                     t.tab.N, stats);
  HIP_LAUNCH_CHECK(stream);
}

}  // namespace channel
