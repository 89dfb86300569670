// kernel_common.hpp -- the few device helpers that kernels.hip (the LP kernels) and node_kernels.hip (the node-entry kernels)
// both use.  Device code only: included by the two .hip files.
#pragma once

#include <hip/hip_runtime.h>

#include "mvx_internal.hpp"

namespace mvx {

#define TIDX ((int)threadIdx.x)

// a / b, correctly rounded.  The fp64 division sequence of gfx950 is almost, not exactly, IEEE: a quotient that lies
// very close to the midpoint of two doubles can come out one ulp off (-0x1.6666666666663p-1 / -0x1.ffffffffffffbp-1
// gives ...666p-1, the nearest double is ...667p-1).  Random operands never hit it (scripts/divcheck.py: 0 of 3e8), the
// near-rational entries of a tableau do: one such quotient parted a 641-node B&B run from the oracle.  The residual a - q*b of a quotient that is
// within one ulp is exact in one fma, so the better of q and its neighbour on the side the residual points to is
// the correctly rounded quotient, whatever the native division returned.  The oracle runs the same function
// (there the native quotient is already the nearest and comes back unchanged).
__device__ __forceinline__ double xdiv(double a, double b) {
  const double q = a / b;
  const double aq = fabs(q);
  if (!(aq > 1e-290 && aq < 1e290)) return q; // zero, subnormal range, inf, nan
  const double r = fma(-q, b, a);
  if (r == 0.0) return q;
  const bool up = (r > 0.0) == (b > 0.0); // the true quotient lies above q
  long long bits = __double_as_longlong(q);
  bits += ((q > 0.0) == up) ? 1 : -1;
  const double q1 = __longlong_as_double(bits);
  const double r1 = fma(-q1, b, a);
  return (fabs(r1) < fabs(r)) ? q1 : q;
}

// the value a non-basic variable rests at: the bound its status names
__device__ __forceinline__ double dev_nb_value(int flag, double lb, double ub) {
  return flag == MVX_NL ? lb : flag == MVX_NU ? ub : flag == MVX_NS ? lb : 0.0;
}

} // namespace mvx
