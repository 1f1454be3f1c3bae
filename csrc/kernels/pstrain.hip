// Pressure-strain plane sums over the spectral fields (kernels.hpp PStrainArgs): the Parseval products
// of the fluctuating static pressure with the strain factors, a bandwidth-bound reduction outside the
// step; the walk, the loads and the reduction are specwalk.hpp's plane-sum kernel.
#include "specwalk.hpp"

namespace channel {

namespace {

struct PStrain {
  using Args = PStrainArgs;
  static constexpr int kRows = kPStrainRows;
  static constexpr unsigned kFields = specwalk::kU | specwalk::kV | specwalk::kW | specwalk::kOz;
  static constexpr bool kPressure = true;
  __device__ static __forceinline__ void accumulate(double (&s)[kRows], const specwalk::Comp& c, specwalk::C cp, double al,
                                                    double be, double wgt) {
    using specwalk::C;
    using specwalk::dot;
    const C cu = c.u, cv = c.v, cw = c.w, oz = c.oz;
    // strain factors: i al u, D v = -i (al u + be w), i be w, D u + i al v = 2 i al v - omega_z
    const C sxx{-al * cu.y, al * cu.x};
    const C szz{-be * cw.y, be * cw.x};
    const C syy{al * cu.y + be * cw.y, -(al * cu.x + be * cw.x)};
    const C sxy{-2.0 * al * cv.y - oz.x, 2.0 * al * cv.x - oz.y};
    s[0] += wgt * 2.0 * dot(cp, sxx);
    s[1] += wgt * 2.0 * dot(cp, syy);
    s[2] += wgt * 2.0 * dot(cp, szz);
    s[3] += wgt * dot(cp, sxy);
    s[4] += wgt * dot(cp, cu);
    s[5] += wgt * dot(cp, cv);
    s[6] += wgt * dot(cp, cp);
  }
};

}  // namespace

void pstrain_accumulate(const PStrainArgs& a, bool fp64, hipStream_t s) {
  specwalk::planesum_accumulate<PStrain>(a, fp64, "pstrain", s);
}

}  // namespace channel
