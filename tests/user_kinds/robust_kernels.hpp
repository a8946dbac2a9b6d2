// tests/user_kinds/robust_kernels.hpp -- a worked example of USER robust kernels (include/nlls_amd.h, NLLS_ROBUST_USER0 .. 7; `make user USER_KINDS=...`).
// What a user of the reference writes as an AbstractRobustifier -- robustify(kernel, cost), and optionally robustifydcost in a closed form (src/robust.jl) -- is here ONE
// templated robustify<T>, generic in the scalar type, and an optional dcost().  Without dcost the library takes rho, rho' and rho'' from robustify<nlls::Jet2>
// (autorobustifydcost, src/autodiff.jl:163).  Every kernel of the path (accumulate sweeps, cost sweep, matrix-free trial, optimizesingles) reaches them through
// robustify_fixed / robustifydcost_fixed, so they compose with NLLS_ROBUST_SCALED and every residual kind.  Parameters: p[0] = robust_params[0], p[1] = robust_params[2].
// This header adds robust kernels only: no residual or variable kinds.
#pragma once
namespace nlls {
// USER0: Huber2oKernel(w) restated (src/robust.jl:46-47), its derivatives by autodiff -- the twin of NLLS_ROBUST_HUBER2O.
template <> struct Robust<NLLS_ROBUST_USER0> {
    static constexpr int NPARAM = 1;
    template <class T> static NLLS_DEV T robustify(const double* p, T cost) {
        const double w = p[0], w2 = w * w;
        if (dval(cost) < w2) return cost;
        return dsqrt(cost) * (w * 2) - w2;
    }
};
// USER1: HuberKernel(w) (src/robust.jl:40-45) with its own robustifydcost, whose second derivative is 0 (src/robust.jl:48-55) -- the twin of NLLS_ROBUST_HUBER.
template <> struct Robust<NLLS_ROBUST_USER1> {
    static constexpr int NPARAM = 1;
    template <class T> static NLLS_DEV T robustify(const double* p, T cost) { return Robust<NLLS_ROBUST_USER0>::robustify<T>(p, cost); }
    static NLLS_DEV void dcost(const double* p, double cost, double& rho, double& d1, double& d2) {
        const double w = p[0], w2 = w * w;
        if (cost < w2) { rho = cost; d1 = 1.0; d2 = 0.0; }
        else { const double sq = sqrt(cost); rho = sq * (w * 2) - w2; d1 = w / sq; d2 = 0.0; }
    }
};
// USER2: GemanMcclureKernel(w) (src/robust.jl:63-77) by autodiff -- the twin of NLLS_ROBUST_GEMAN_MCCLURE.  rho = s w^2 / (s + w^2), written on each side of w^2 so that
// neither the value nor the derivatives cancel: the quotient rule of s / (s + w^2) subtracts nearly equal numbers for s >> w^2, w^2 - w^4 / (s + w^2) does for s << w^2.
template <> struct Robust<NLLS_ROBUST_USER2> {
    static constexpr int NPARAM = 1;
    template <class T> static NLLS_DEV T robustify(const double* p, T cost) {
        const double w2 = p[0] * p[0];
        if (dval(cost) < w2) return cost * w2 / (cost + w2);
        return w2 - (w2 * w2) / (cost + w2);
    }
};
// USER3: Cauchy, rho = w^2 log(1 + s / w^2):  rho' = 1 / (1 + s / w^2).
template <> struct Robust<NLLS_ROBUST_USER3> {
    static constexpr int NPARAM = 1;
    template <class T> static NLLS_DEV T robustify(const double* p, T cost) {
        const double w2 = p[0] * p[0];
        return dlog1p(cost / w2) * w2;
    }
};
// USER4: Barron's general loss with scale c = p[0] and shape alpha = p[1] (not 0 or 2):  b = c^2 |alpha - 2|,
//   rho = 2 b / alpha ((s / b + 1)^(alpha / 2) - 1),   rho' = (s / b + 1)^(alpha / 2 - 1).   alpha = -2 is Geman-McClure with w = 2 c, alpha = 1 a pseudo-Huber.
template <> struct Robust<NLLS_ROBUST_USER4> {
    static constexpr int NPARAM = 2;
    template <class T> static NLLS_DEV T robustify(const double* p, T cost) {
        const double c = p[0], alpha = p[1], b = c * c * fabs(alpha - 2.0);
        return dexpm1(dlog1p(cost / b) * (0.5 * alpha)) * (2.0 * b / alpha);
    }
};
// USER5: Tukey's biweight, rho = w^2 / 3 (1 - (1 - s / w^2)^3) up to w^2 and w^2 / 3 beyond: rho' = (1 - s / w^2)^2, then 0.  A branch on the value.
template <> struct Robust<NLLS_ROBUST_USER5> {
    static constexpr int NPARAM = 1;
    template <class T> static NLLS_DEV T robustify(const double* p, T cost) {
        const double w2 = p[0] * p[0];
        if (dval(cost) >= w2) return Lift<T>::c(w2 / 3.0);
        const T u = 1.0 - cost / w2;
        return (1.0 - u * u * u) * (w2 / 3.0);
    }
};
}  // namespace nlls
#define NLLS_USER_ROBUST(X) X(NLLS_ROBUST_USER0) X(NLLS_ROBUST_USER1) X(NLLS_ROBUST_USER2) X(NLLS_ROBUST_USER3) X(NLLS_ROBUST_USER4) X(NLLS_ROBUST_USER5)
