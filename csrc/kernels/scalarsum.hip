// Scalar plane sums over the spectral fields (kernels.hpp ScalarSumArgs): theta-hat rides in the place of
// p-hat'; the walk, the loads and the reduction are specwalk.hpp's plane-sum kernel.
#include "specwalk.hpp"

namespace channel {

namespace {

struct ScalarSum {
  using Args = ScalarSumArgs;
  static constexpr int kRows = kScalarSumRows;
  static constexpr unsigned kFields = specwalk::kU | specwalk::kV | specwalk::kW;
  static constexpr bool kPressure = true;
  __device__ static __forceinline__ void accumulate(double (&s)[kRows], const specwalk::Comp& c, specwalk::C th, double,
                                                    double, double wgt) {
    s[0] += wgt * specwalk::sq(th);
    s[1] += wgt * specwalk::dot(c.u, th);
    s[2] += wgt * specwalk::dot(c.v, th);
    s[3] += wgt * specwalk::dot(c.w, th);
  }
};

}  // namespace

void scalarsum_accumulate(const ScalarSumArgs& a, bool fp64, hipStream_t s) {
  specwalk::planesum_accumulate<ScalarSum>(a, fp64, "scalarsum", s);
}

}  // namespace channel
