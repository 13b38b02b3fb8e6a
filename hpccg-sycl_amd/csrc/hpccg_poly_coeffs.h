// hpccg_poly_coeffs.h -- the scalars of the Chebyshev preconditioner
// (include/hpccg_hip_poly.h), computed on the host in double, exactly these
// expressions with no contraction. Plain C++ with no HIP in it, so that
// tests/test_poly_cpu.py can compile it alone and compare it with its NumPy
// restatement bit for bit.
#pragma once

namespace hpccg {

constexpr int kPolyMaxDegree = 16;     // the cap on `degree`
constexpr double kPolyEigRatio = 30.0;  // lmin == 0.0 means lmax / kPolyEigRatio

// For the interval [lmin, lmax], 0 < lmin < lmax, and degree d <= kPolyMaxDegree:
// *c0 of step 0 and a[j], b[j] of step j = 1 .. d (a[0], b[0] unused, 0.0).
inline void poly_coefficients(double lmin, double lmax, int d, double* c0, double* a, double* b)
{
    const double theta = 0.5 * (lmax + lmin);
    const double delta = 0.5 * (lmax - lmin);
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    *c0 = 1.0 / theta;
    a[0] = b[0] = 0.0;
    for (int j = 1; j <= d; j++) {
        const double rho_new = 1.0 / (2.0 * sigma - rho);
        a[j] = rho_new * rho;
        b[j] = 2.0 * rho_new / delta;
        rho = rho_new;
    }
}

}  // namespace hpccg
