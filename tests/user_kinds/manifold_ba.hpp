// tests/user_kinds/manifold_ba.hpp -- a worked example of USER variable kinds (include/nlls_amd.h, NLLS_VAR_USER0 .. 7) next to the user residual kinds over them
// (NLLS_RES_USER0 .. 7; `make user USER_KINDS=...`).  What a user of the reference writes as a Julia variable type -- nvars() and update() (src/variable.jl) -- is here
// ONE struct: STORAGE, DOF and a templated update<T>(v, d, out), generic in the scalar type.  The library differentiates update() at d = 0 by dual numbers for the Jacobian
// (the reference's update(var, dualzeros), src/autodiff.jl:57-61) and calls update<double> to retract an LM step.
//
// The pitfall: update() is differentiated AT d = 0, so its derivatives there must be finite -- sqrt(|w|^2) of a zero dual has NaN partials.  Every function below whose
// argument can be a zero tangent takes a series branch for small arguments (as the library's so3_exp does).
#pragma once
namespace nlls {
namespace manifold_ba {
template <class T> NLLS_HD T zero() { return Lift<T>::c(0.0); }
// expm([w]x), column-major 3x3, generic in T: Rodrigues with the series of A = sin(th) / th, B = (1 - cos(th)) / th^2 near 0
template <class T> NLLS_HD void so3_exp_t(const T* w, T* E) {
    const T th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    T A, B;
    if (dval(th2) < 1e-12) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; }
    else { const T th = dsqrt(th2); A = dsin(th) / th; B = (1.0 - dcos(th)) / th2; }
    const T z = zero<T>();
    const T K[9] = {z, w[2], -w[1], -w[2], z, w[0], w[1], -w[0], z};
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) {
            T k2 = K[r] * K[3 * c] + K[r + 3] * K[1 + 3 * c] + K[r + 6] * K[2 + 3 * c];
            E[r + 3 * c] = (r == c ? 1.0 : 0.0) + A * K[r + 3 * c] + B * k2;      // (the library's order of the sums)
        }
}
// the pinhole of NLLS_RES_BA_SO3 over a pose whose rotation is a column-major 3x3 R and whose translation follows it: (Y0, Y1) / Y2 - measurement,  Y = R X + t
template <class T> NLLS_HD void pinhole_rt(const double* data, const T* P, const T* X, T* r) {
    T Y[3];
    for (int i = 0; i < 3; ++i) Y[i] = P[i] * X[0] + P[i + 3] * X[1] + P[i + 6] * X[2] + P[9 + i];
    r[0] = Y[0] / Y[2] - data[0]; r[1] = Y[1] / Y[2] - data[1];
}
}  // namespace manifold_ba

// USERVAR0: the SO(3) pose of NLLS_VAR_POSE_SO3 restated generically -- R (3x3 column-major) + t, R <- R expm([w]x), t <- t + tau.  No closed-form Jacobian: the twin of
// the built-in kind, whose derivatives the library writes out by hand.
template <> struct Var<NLLS_VAR_USER0> {
    static constexpr int STORAGE = 12, DOF = 6;
    template <class T> static NLLS_HD void update(const double* v, const T* d, T* out) {
        T E[9]; manifold_ba::so3_exp_t(d, E);
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) out[r + 3 * c] = v[r] * E[3 * c] + v[r + 3] * E[1 + 3 * c] + v[r + 6] * E[2 + 3 * c];
        for (int i = 0; i < 3; ++i) out[9 + i] = d[3 + i] + v[9 + i];
    }
};
// USER0: the pinhole of NLLS_RES_BA_SO3 over USERVAR0 and a point (EuclideanVector{3}); the same data layout (the measured (u, v))
template <> struct Res<NLLS_RES_USER0> {
    static constexpr int NDEPS = 2, M = 2, NDATA = 2, ADAPT = 0;
    static constexpr int SK[2] = {NLLS_VAR_USER0, NLLS_VAR_EUCLIDEAN};
    static constexpr int SD[2] = {6, 3};
    template <class T> static NLLS_DEV void eval(const double* data, const T (*sv)[MAXST], T* r) { manifold_ba::pinhole_rt(data, sv[0], sv[1], r); }
};

// USERVAR1: a unit-quaternion pose, storage (qw, qx, qy, qz, tx, ty, tz), dof 6:  q <- normalize(q * exp(w / 2)),  t <- t + tau
//   exp(w / 2) = (cos(th / 2), sin(th / 2) / th w),  th = |w|, with the series (1 - th^2 / 8, 1 / 2 - th^2 / 48) near 0
template <> struct Var<NLLS_VAR_USER1> {
    static constexpr int STORAGE = 7, DOF = 6;
    template <class T> static NLLS_HD void update(const double* v, const T* d, T* out) {
        const T th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        T c, s;
        if (dval(th2) < 1e-12) { c = 1.0 - th2 / 8.0; s = 0.5 - th2 / 48.0; }
        else { const T th = dsqrt(th2); c = dcos(th * 0.5); s = dsin(th * 0.5) / th; }
        const T ex = s * d[0], ey = s * d[1], ez = s * d[2];
        // q * e  (Hamilton product, q on the left: the step is in the body frame, as R expm([w]x) of the SO(3) pose)
        const T w = v[0] * c - v[1] * ex - v[2] * ey - v[3] * ez;
        const T x = v[0] * ex + v[1] * c + v[2] * ez - v[3] * ey;
        const T y = v[0] * ey - v[1] * ez + v[2] * c + v[3] * ex;
        const T z = v[0] * ez + v[1] * ey - v[2] * ex + v[3] * c;
        const T in = 1.0 / dsqrt(w * w + x * x + y * y + z * z);   // (|q e| = |q| = 1 at d = 0: finite)
        out[0] = w * in; out[1] = x * in; out[2] = y * in; out[3] = z * in;
        for (int i = 0; i < 3; ++i) out[4 + i] = d[3 + i] + v[4 + i];
    }
};
// USER1: a pinhole over USERVAR1 and a point (EuclideanVector{3}):  Y = R(q) X + t,  r = (Y0, Y1) / Y2 - measurement.  R(q) X = X + 2 qw (u x X) + 2 u x (u x X), u = (qx, qy, qz)
template <> struct Res<NLLS_RES_USER1> {
    static constexpr int NDEPS = 2, M = 2, NDATA = 2, ADAPT = 0;
    static constexpr int SK[2] = {NLLS_VAR_USER1, NLLS_VAR_EUCLIDEAN};
    static constexpr int SD[2] = {6, 3};
    template <class T> static NLLS_DEV void eval(const double* data, const T (*sv)[MAXST], T* r) {
        const T* q = sv[0]; const T* X = sv[1];
        const T cx = q[2] * X[2] - q[3] * X[1], cy = q[3] * X[0] - q[1] * X[2], cz = q[1] * X[1] - q[2] * X[0];           // u x X
        const T dx = q[2] * cz - q[3] * cy, dy = q[3] * cx - q[1] * cz, dz = q[1] * cy - q[2] * cx;                        // u x (u x X)
        const T Y0 = X[0] + 2.0 * (q[0] * cx + dx) + q[4], Y1 = X[1] + 2.0 * (q[0] * cy + dy) + q[5], Y2 = X[2] + 2.0 * (q[0] * cz + dz) + q[6];
        r[0] = Y0 / Y2 - data[0]; r[1] = Y1 / Y2 - data[1];
    }
};

// USERVAR2: a unit 3-vector, storage 3, dof 2.  The tangent basis comes from the current value: b1 = normalize(a x v) with a the axis least aligned with v
// (e_x unless |v_x| > 0.5, then e_y), b2 = v x b1;  v <- normalize(v + d0 b1 + d1 b2).
template <> struct Var<NLLS_VAR_USER2> {
    static constexpr int STORAGE = 3, DOF = 2;
    template <class T> static NLLS_HD void update(const double* v, const T* d, T* out) {
        double b1[3];
        if (fabs(v[0]) > 0.5) { b1[0] = v[2]; b1[1] = 0.0; b1[2] = -v[0]; }     // e_y x v
        else { b1[0] = 0.0; b1[1] = -v[2]; b1[2] = v[1]; }                      // e_x x v
        const double n1 = 1.0 / sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
        for (int i = 0; i < 3; ++i) b1[i] *= n1;
        const double b2[3] = {v[1] * b1[2] - v[2] * b1[1], v[2] * b1[0] - v[0] * b1[2], v[0] * b1[1] - v[1] * b1[0]};
        T u[3];
        for (int i = 0; i < 3; ++i) u[i] = d[0] * b1[i] + d[1] * b2[i] + v[i];
        const T in = 1.0 / dsqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);      // (|v| = 1 at d = 0: finite)
        for (int i = 0; i < 3; ++i) out[i] = u[i] * in;
    }
};
// USER2: a measured direction:  r = dir - measured  (M = 3)
template <> struct Res<NLLS_RES_USER2> {
    static constexpr int NDEPS = 1, M = 3, NDATA = 3, ADAPT = 0;
    static constexpr int SK[1] = {NLLS_VAR_USER2};
    static constexpr int SD[1] = {2};
    template <class T> static NLLS_DEV void eval(const double* data, const T (*sv)[MAXST], T* r) {
        for (int i = 0; i < 3; ++i) r[i] = sv[0][i] - data[i];
    }
};
}  // namespace nlls
#define NLLS_USER_VAR(X) X(NLLS_VAR_USER0) X(NLLS_VAR_USER1) X(NLLS_VAR_USER2)
#define NLLS_USER_RES(X) X(NLLS_RES_USER0) X(NLLS_RES_USER1) X(NLLS_RES_USER2)
