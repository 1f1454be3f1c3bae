// Velocity-gradient plane sums over the spectral fields (kernels.hpp GradSumArgs): a bandwidth-bound
// reduction outside the step; the walk, the loads and the reduction are specwalk.hpp's plane-sum kernel.
#include "specwalk.hpp"

namespace channel {

namespace {

struct GradSum {
  using Args = GradSumArgs;
  static constexpr int kRows = kGradRows;
  static constexpr unsigned kFields = specwalk::kAll;
  static constexpr bool kPressure = false;
  __device__ static __forceinline__ void accumulate(double (&s)[kRows], const specwalk::Comp& c, specwalk::C, double al,
                                                    double be, double wgt) {
    using specwalk::C;
    const C cu = c.u, cv = c.v, cw = c.w, ox = c.ox, oy = c.oy, oz = c.oz;
    const double k2 = al * al + be * be;
    // D u = i al v - omega_z, D w = omega_x + i be v, D v = -i (al u + be w)
    const C du{-al * cv.y - oz.x, al * cv.x - oz.y};
    const C dw{ox.x - be * cv.y, ox.y + be * cv.x};
    const C dv{al * cu.y + be * cw.y, -(al * cu.x + be * cw.x)};
    s[0] += wgt * (ox.x * ox.x + ox.y * ox.y);
    s[1] += wgt * (oy.x * oy.x + oy.y * oy.y);
    s[2] += wgt * (oz.x * oz.x + oz.y * oz.y);
    s[3] += wgt * (k2 * (cu.x * cu.x + cu.y * cu.y) + du.x * du.x + du.y * du.y);
    s[4] += wgt * (k2 * (cv.x * cv.x + cv.y * cv.y) + dv.x * dv.x + dv.y * dv.y);
    s[5] += wgt * (k2 * (cw.x * cw.x + cw.y * cw.y) + dw.x * dw.x + dw.y * dw.y);
    s[6] += wgt * (k2 * (cu.x * cv.x + cu.y * cv.y) + du.x * dv.x + du.y * dv.y);
  }
};

}  // namespace

void gradsum_accumulate(const GradSumArgs& a, bool fp64, hipStream_t s) {
  specwalk::planesum_accumulate<GradSum>(a, fp64, "gradsum", s);
}

}  // namespace channel
