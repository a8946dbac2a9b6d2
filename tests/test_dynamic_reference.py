"""A long-double reference of the dynamic-size blocks, written out plainly, and the float64 CPU oracle held to it at the lengths the device kernels branch on.

The dynamic-size kinds (NLLS_VAR_DYNAMIC under NLLS_RES_DYN_LINEAR, NLLS_RES_DYN_NORM, NLLS_RES_DYN_LINEARSQ, NLLS_COST_DYN_LINEAR) are the one place where a block's
length n is a run-time number (1 .. NLLS_MAX_DYN_DIM = 4096; 512 for DYN_LINEARSQ).  tests/test_gpu_dynamic_lengths.py moves n across every boundary of the kernels
that take them; this file is its reference and shows, without a GPU, that the reference and the committed oracle agree to the same bound.

The reference.  With c = r'r and (rho, rho', rho'') the robust kernel's value and derivatives at c (closed forms as tests/test_oracle_pins.py pins them):
    cost = rho / 2        g = rho' J'r        H = rho' J'J + 2 rho'' (J'r)(J'r)'
    DYN_LINEAR   r = X'w - y (one residual), J = X'          DYN_NORM  r = w, J = I          DYN_LINEARSQ  r = X w - y, J = X (n x n, column-major in the payload)
    COST_DYN_LINEAR   the non-squared cost y'w: value y'w, gradient y, Hessian 0, no kernel
every product and every sum in np.longdouble (64-bit significand: n u_ld <= 4096 * 5.5e-20 = 2.2e-16 of the absolute-value sum, four orders below the bound).

The absolute-value companion q_abs of a quantity q is the same formula with every product and term replaced by its absolute value:
    r_abs = |J||w| + |y|      c_abs = r_abs'r_abs      g_abs = |rho'| |J|'r_abs      H_abs = |rho'| |J|'|J| + 2 |rho''| (|J|'r_abs)(|J|'r_abs)'
(for DYN_LINEAR: H_abs = (|rho'| + 2 |rho''| r_abs^2) |X||X|').  Through the kernel the companion is the first-order one: rho(c) = rho'(c) c + (rho(c) - rho'(c) c),
the first term carries the rounding of the sum c (relative to c_abs, not to c), the second a handful of operations of its own, so
    cost_abs = (|rho'| c_abs + |rho - rho' c|) / 2          weight_abs = |rho'| + |rho''| c_abs          (weight = rho', what nlls_eval_blocks returns)
which is c_abs / 2 without a kernel and never below |cost|.  The companions are scales of a tolerance: the n x n ones are formed in float64 (sums of non-negative
terms: good to 1e-13 of themselves), everything else in long double.

The bound.  For an output array q of a block (r, the cost, b, the block of A):      max |q - q_ref| <= 8 (n + 8) u max q_abs,      u = 2^-53.
(n + 8) u is the a-priori bound of an n-term sum plus a handful of further operations, in any order, with or without fma (so it covers atomics and the reduction
tree); 8 = 2 (the square c = r'r) x 2 (the kernels' conditioning: |c rho'' / rho'| <= 2 for Huber, Huber2o and Geman-McClure) x 2 (DYN_LINEARSQ: J'r is a sum over
sums).  A dropped or misplaced element changes a result by O(1 / n) of its size, ten orders above this bound.

The problems.  `start` and `payload` fix c = r'r at 2.25 mag^2 for every residual kind and every n, so that mag = 0.01 lies inside the quadratic region of the
kernels below (c < w^2) and mag = 2.0 outside it, n = 1 included; `check_regions` asserts it."""
import functools
import hashlib

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from tests.helpers import LD, oracle_problem, blockindices

U = 2.0 ** -53
RES_KINDS = (K.RES_DYN_LINEAR, K.RES_DYN_NORM, K.RES_DYN_LINEARSQ)
KIND_NAME = {K.RES_DYN_LINEAR: "LINEAR", K.RES_DYN_NORM: "NORM", K.RES_DYN_LINEARSQ: "LINEARSQ", K.COST_DYN_LINEAR: "COST"}
SQ_MAX, DYN_MAX = 512, 4096                                   # include/nlls_amd.h: NLLS_RES_DYN_LINEARSQ's limit, NLLS_MAX_DYN_DIM
# a single lane, the first pair | one wavefront of block_sum | one workgroup's lanes (TPB = 256) | the LDS arrays rs[512] / gs[512] | third and later trips
H_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024)
VALUE_LENGTHS = H_LENGTHS + (DYN_MAX,)                        # (no n x n array is formed at 4096)
KERNELS = {"none": None, "huber": N.HuberKernel(0.4), "geman": N.GemanMcclureKernel(0.7), "scaled_huber2o": N.Scaled(N.Huber2oKernel(0.5), 1.7)}
MAGS = (0.01, 2.0)


def bound(n):
    return 8.0 * (n + 8) * U


def admits(kind, n):
    return n <= (SQ_MAX if kind == K.RES_DYN_LINEARSQ else DYN_MAX)


def kinds_at(n):
    return [k for k in RES_KINDS + (K.COST_DYN_LINEAR,) if admits(k, n)]


# ---- the robust kernels (src/robust.jl:11-12,26-31,47-55,71-77) ------------------------------------------------------------------------------------------------
def kernel_ld(robust, c):
    """(rho, rho', rho'') at c, long double"""
    c = LD(c); kind = 0 if robust is None else int(robust.kind); base = kind & 0xF; one, zero = LD(1), LD(0)
    if base in (K.ROBUST_HUBER, K.ROBUST_HUBER2O):
        w = LD(robust.params[0]); w2 = w * w
        if c < w2: o = (c, one, zero)
        else:
            sq = np.sqrt(c); o = (2 * w * sq - w2, w / sq, -w / (2 * c * sq) if base == K.ROBUST_HUBER2O else zero)
    elif base == K.ROBUST_GEMAN_MCCLURE:
        w2 = LD(robust.params[0]) ** 2; t = one / (c + w2); o = (c * w2 * t, (w2 * t) ** 2, -2 * w2 * w2 * t ** 3)
    else:
        assert base == K.ROBUST_NONE; o = (c, one, zero)
    s = LD(robust.params[1]) if kind & K.ROBUST_SCALED else one
    return tuple(s * v for v in o)


def kernel_width2(robust):
    """w^2 of the kernel: below it the Huber kernels are the identity, Geman-McClure close to it"""
    return None if robust is None or robust.kind == K.ROBUST_NONE else float(robust.params[0]) ** 2


# ---- one block ----------------------------------------------------------------------------------------------------------------------------------------------
_GRAMS = {}


def _gram(X):
    """X'X in long double, kept per matrix (0.6 s at n = 512): the kernels and magnitudes of a length share their X"""
    key = hashlib.sha1(np.ascontiguousarray(X).tobytes()).hexdigest()
    if key not in _GRAMS:
        if len(_GRAMS) >= 8: _GRAMS.pop(next(iter(_GRAMS)))
        Xl = np.asarray(X).astype(LD); _GRAMS[key] = np.einsum("ij,ik->jk", Xl, Xl)
    return _GRAMS[key]


def block_reference(kind, robust, w, data, want_H=True):
    """One block of `kind` over the variable w with payload `data` (float64, as the device gets them) -> dict: n, r / r_abs, c / c_abs (r'r), rho / rho_abs,
    weight / weight_abs (rho'), cost / cost_abs, g / g_abs (length n), H / H_abs (n x n; None if not wanted or identically zero)."""
    w = np.asarray(w, np.float64).ravel(); n = w.size; wl = w.astype(LD); aw = np.abs(wl)
    d = np.asarray(data, np.float64).ravel(); dl = d.astype(LD)
    out = dict(n=n, kind=kind)
    if kind == K.COST_DYN_LINEAR:
        assert d.size == n and (robust is None or robust.kind == K.ROBUST_NONE)
        out.update(cost=dl @ wl, cost_abs=np.abs(dl) @ aw, g=dl, g_abs=np.abs(dl), H=None, H_abs=None)
        return out
    if kind == K.RES_DYN_LINEAR:
        assert d.size == 1 + n
        y, X = dl[0], dl[1:]; r = np.array([X @ wl - y]); r_abs = np.array([np.abs(X) @ aw + abs(y)])
        Jr, Jr_abs = X * r[0], np.abs(X) * r_abs[0]
        JtJ = lambda: np.outer(X, X); JtJ_abs = lambda: np.outer(np.abs(d[1:]), np.abs(d[1:]))
    elif kind == K.RES_DYN_NORM:
        assert d.size == 0
        r, r_abs = wl, aw; Jr, Jr_abs = wl, aw
        JtJ = lambda: np.eye(n, dtype=LD); JtJ_abs = lambda: np.eye(n)
    else:
        assert kind == K.RES_DYN_LINEARSQ and d.size == n + n * n and n <= SQ_MAX
        y = dl[:n]; Xd = d[n:].reshape(n, n, order="F"); X = Xd.astype(LD); aX = np.abs(X)
        r = X @ wl - y; r_abs = aX @ aw + np.abs(y)
        Jr, Jr_abs = X.T @ r, aX.T @ r_abs
        JtJ = lambda: _gram(Xd); JtJ_abs = lambda: np.abs(Xd).T @ np.abs(Xd)
    c, c_abs = r @ r, r_abs @ r_abs
    rho, d1, d2 = kernel_ld(robust, c)
    w2 = kernel_width2(robust)
    if w2 is not None: assert abs(float(c) - w2) > 1e-6 * w2, "the block sits on the kernel's branch point: the device may take the other side"
    out.update(r=r, r_abs=r_abs, c=c, c_abs=c_abs, rho=rho, rho_abs=abs(d1) * c_abs + abs(rho - d1 * c), weight=d1, weight_abs=abs(d1) + abs(d2) * c_abs)
    out.update(cost=rho / 2, cost_abs=out["rho_abs"] / 2, g=d1 * Jr, g_abs=abs(d1) * Jr_abs, H=None, H_abs=None)
    if want_H:
        out["H"] = d1 * JtJ() + (2 * d2) * np.outer(Jr, Jr)
        ja = Jr_abs.astype(np.float64)
        out["H_abs"] = float(abs(d1)) * JtJ_abs() + float(2 * abs(d2)) * np.outer(ja, ja)
    return out


# ---- whole problems of dynamic-size groups ---------------------------------------------------------------------------------------------------------------------
def problem_reference(problem, groups=None, variables=None, want_H=True):
    """The dynamic-size groups of `problem` (its other groups are left out), block by block -> dict: cost / cost_abs (their sum), nblocks, and per variable
    (1-based) var[v] = dict(n, g, g_abs, H, H_abs, blocks): the sums of its blocks, whether or not the variable is fixed.  groups / variables: in place of the
    problem's own (a payload replaced on the device, a trial point)."""
    groups = problem.groups() if groups is None else groups
    x = np.asarray(problem.variables if variables is None else variables, np.float64); off = problem.var_offsets
    rob = [g.robust for g in problem.costs.values()]
    ref = dict(cost=LD(0), cost_abs=LD(0), nblocks=0, var={}, blocks=[])
    for gi, g in enumerate(groups):
        if g["res_kind"] not in KIND_NAME: continue
        vi = np.asarray(g["varind"]).reshape(-1); da = np.asarray(g["data"]).reshape(vi.size, -1)
        for k, v in enumerate(vi):
            blk = block_reference(g["res_kind"], rob[gi], x[off[v - 1]:off[v]], da[k], want_H)
            blk.update(group=gi, index=k, var=int(v), robust=rob[gi]); ref["blocks"].append(blk)
            ref["cost"] += blk["cost"]; ref["cost_abs"] += blk["cost_abs"]; ref["nblocks"] += 1
            n = blk["n"]
            V = ref["var"].setdefault(int(v), dict(n=n, g=np.zeros(n, LD), g_abs=np.zeros(n, LD), H=np.zeros((n, n), LD) if want_H else None,
                                                   H_abs=np.zeros((n, n)) if want_H else None, blocks=[]))
            V["g"] += blk["g"]; V["g_abs"] += blk["g_abs"]; V["blocks"].append(blk)
            if want_H and blk["H"] is not None: V["H"] += blk["H"]; V["H_abs"] += blk["H_abs"]
    return ref


# ---- the data ----------------------------------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.standard_normal(n); return v / np.linalg.norm(v)


@functools.lru_cache(maxsize=None)
def _matrices(n, tag=0):
    """per length: X of DYN_LINEAR (entries N(0, 1)) and the well-conditioned square X of DYN_LINEARSQ, shared by every kernel and magnitude of the length"""
    rng = np.random.default_rng(1000 * (tag + 1) + n)
    X = rng.standard_normal(n)
    Xs = rng.standard_normal((n, n)) / np.sqrt(n) + np.eye(n) if n <= SQ_MAX else None
    return X, Xs


def start(n, mag, rng):
    """a variable of norm 1.5 mag: c = 2.25 mag^2 for DYN_NORM"""
    return 1.5 * mag * _unit(rng, n)


def payload(kind, w, mag, rng, tag=0):
    """the payload of a block of `kind` over w with r'r = 2.25 mag^2 (to the rounding of y); COST_DYN_LINEAR: y ~ N(0, 1)"""
    n = w.size; X, Xs = _matrices(n, tag)
    if kind == K.RES_DYN_LINEAR: return np.concatenate([[X @ w + 1.5 * mag], X])
    if kind == K.RES_DYN_NORM: return np.zeros(0)
    if kind == K.RES_DYN_LINEARSQ: return np.concatenate([Xs @ w - 1.5 * mag * _unit(rng, n), Xs.ravel(order="F")])
    assert kind == K.COST_DYN_LINEAR
    return rng.standard_normal(n)


def add_all_kinds(p, v, mag, robust, rng, tag=0):
    """one block of every kind that admits the length on variable v (1-based) of p"""
    w = p.variable(v).copy()
    for kind in kinds_at(w.size):
        p.addcosts(kind, [[v]], payload(kind, w, mag, rng, tag)[None, :], robust=None if kind == K.COST_DYN_LINEAR else robust)


def one_variable_problem(n, kname, mag):
    """case a: one variable of length n under every kind that admits it, the residual kinds under KERNELS[kname]"""
    rng = np.random.default_rng([n, list(KERNELS).index(kname), int(mag * 100)])
    p = N.NLLSProblem(); v = p.addvariable(start(n, mag, rng), K.VAR_DYNAMIC)
    add_all_kinds(p, v, mag, KERNELS[kname], rng)
    return p


def check_regions(ref, mag):
    """the condition the magnitudes are chosen for: every residual block at mag 0.01 inside its kernel's quadratic region (c < w^2), at 2.0 outside it.
    mag: one magnitude, or one per variable (a dict by the variable's 1-based number)"""
    for b in ref["blocks"]:
        if b["kind"] == K.COST_DYN_LINEAR: continue
        m = mag[b["var"]] if isinstance(mag, dict) else mag; w2 = kernel_width2(b["robust"]); c = float(b["c"])
        assert np.isclose(c, 2.25 * m * m, rtol=1e-6), (KIND_NAME[b["kind"]], b["n"], c)
        if w2 is not None: assert (c < w2) == (m == MAGS[0]) and (c > w2) == (m == MAGS[1]), (KIND_NAME[b["kind"]], c, w2)


def share(dev, ref, ref_abs, n):
    """the share of the bound 8 (n + 8) u max ref_abs that max |dev - ref| uses; a quantity whose companion is zero must be zero"""
    dev = np.asarray(dev); ref = np.asarray(ref); scale = float(np.max(np.abs(ref_abs))) if np.size(ref_abs) else 0.0
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    if dev.size == 0: return 0.0
    err = float(np.max(np.abs(dev.astype(LD) - ref.astype(LD))))
    if not np.isfinite(err): return np.inf
    if scale == 0.0: return 0.0 if err == 0.0 else np.inf
    return err / (bound(n) * scale)


# ---- the oracle against the reference -----------------------------------------------------------------------------------------------------------------------------
ORACLE_SHARE = {}


def _note(what, s):
    ORACLE_SHARE[what] = max(ORACLE_SHARE.get(what, 0.0), s)


@pytest.mark.parametrize("n", H_LENGTHS)
def test_oracle_holds_the_bound(n):
    """cost, b and the lower triangle of H of the float64 oracle against the long-double closed forms, one variable under all kinds, four kernels, both regions"""
    worst = {}
    for kname, robust in KERNELS.items():
        for mag in MAGS:
            p = one_variable_problem(n, kname, mag); ref = problem_reference(p); check_regions(ref, mag)
            assert ref["nblocks"] == len(kinds_at(n)) and list(ref["var"]) == [1]
            ols = oracle_problem(p).linear_system(blockindices(p)); cost = ols.costgradhess()
            assert not ols.info.is_sparse and ols.info.ndof == n
            V = ref["var"][1]; H = ols.data.reshape(n, n).T; lo = np.tril_indices(n)                  # (column-major: H[i, j] = data[j n + i]; the lower triangle is filled)
            for what, s in (("cost", share(cost, ref["cost"], ref["cost_abs"], n)), ("b", share(ols.b, V["g"], V["g_abs"], n)), ("H", share(H[lo], V["H"][lo], V["H_abs"][lo], n))):
                worst[what] = max(worst.get(what, 0.0), s); _note(what, s)
                assert s <= 1.0, f"oracle {what} at n={n} {kname} mag={mag}: {s:.3g} of the bound"
            assert np.isclose(oracle_problem(p).cost(), float(ref["cost"]), rtol=0, atol=bound(n) * float(ref["cost_abs"]))
    print(f"ORACLE n={n} kinds={'+'.join(KIND_NAME[k] for k in kinds_at(n))} share of the bound: " + " ".join(f"{k}={v:.3%}" for k, v in worst.items()))


def test_oracle_cost_at_the_largest_variable():
    """n = 4096: the cost only (no n x n array), the three kinds that admit it"""
    n = DYN_MAX
    for kname, robust in KERNELS.items():
        for mag in MAGS:
            p = one_variable_problem(n, kname, mag); ref = problem_reference(p, want_H=False); check_regions(ref, mag)
            assert [b["kind"] for b in ref["blocks"]] == [K.RES_DYN_LINEAR, K.RES_DYN_NORM, K.COST_DYN_LINEAR]
            s = share(oracle_problem(p).cost(), ref["cost"], ref["cost_abs"], n); _note("cost", s)
            assert s <= 1.0, (kname, mag, s)


def test_reference_against_central_differences():
    """the closed forms themselves: g against central differences of the reference's own cost, H against central differences of g, at a length past one workgroup's
    lanes for nothing but variety (n = 7 would do): pins the signs and the factor 2 of the rho'' term independently of the oracle"""
    n, h = 9, 1e-5
    for kname, robust in KERNELS.items():
        for mag in MAGS:
            p = one_variable_problem(n, kname, mag); w0 = p.variables.copy(); V = problem_reference(p)["var"][1]
            at = lambda w: problem_reference(p, variables=w)
            gfd = np.array([float(at(w0 + h * e)["cost"] - at(w0 - h * e)["cost"]) / (2 * h) for e in np.eye(n)])
            Hfd = np.array([((at(w0 + h * e)["var"][1]["g"] - at(w0 - h * e)["var"][1]["g"]) / (2 * h)).astype(np.float64) for e in np.eye(n)])
            assert np.allclose(V["g"].astype(np.float64), gfd, rtol=1e-6, atol=1e-8 * np.max(np.abs(gfd))), (kname, mag)
            if robust is None or (robust.kind & 0xF) != K.ROBUST_HUBER:       # (HuberKernel drops rho'' outside the quadratic region by definition: src/robust.jl:40-45)
                assert np.allclose(V["H"].astype(np.float64), Hfd, rtol=1e-5, atol=1e-7 * np.max(np.abs(Hfd))), (kname, mag)


def test_companions_dominate():
    """every companion is at least the magnitude of its quantity (so a bound of the form eps * q_abs also bounds the quantity's own rounding)"""
    for n in (1, 5, 65):
        for kname in KERNELS:
            for mag in MAGS:
                for b in problem_reference(one_variable_problem(n, kname, mag))["blocks"]:
                    for q in ("cost", "g", "H") + (("r", "rho", "weight") if b["kind"] != K.COST_DYN_LINEAR else ()):
                        if b[q] is None: continue
                        assert np.all(np.abs(np.asarray(b[q]).astype(np.float64)) <= np.asarray(b[q + "_abs"]).astype(np.float64) * (1 + 1e-12)), (n, kname, mag, KIND_NAME[b["kind"]], q)
