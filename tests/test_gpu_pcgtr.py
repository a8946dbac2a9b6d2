"""nlls_solve_pcg_tr: Steihaug-Toint conjugate gradients inside the trust region ||y||_M <= radius, on the device's matrix-free operator (include/nlls_amd.h).

The host reference is `steihaug_mirror`: tests/test_gpu_pcg.py::pcg_mirror with the three recurrences of the trust region (yy = ||y||_M^2, yp = y'Mp, pp = ||p||_M^2)
and the model value.  Every case runs it on the HOST's A + lambda I first and asserts what it rests on -- convergence, the iteration of the crossing, the negative
eigenvalue -- so that a bad input blames the input; then on the device's own operator (ctx.hess_apply, ctx.hess_block_diag) for the comparison.

Tolerances of the boundary exits are measured against the reference: the host mirror runs a second time in np.longdouble, and the float64 mirror's distance from it is
the drift of the recurrences on that input (the norm at exit against the radius, the iterate, the model value).  The device is held to TEN times that drift -- it adds in
another order -- and to no less than 1e-11 (of the radius; of the iterate's largest entry: the suite's bound for a truncated iterate, tests/test_gpu_pcg.py).  The case
asserts that the host drift itself stays below 1e-9.  With radius = +inf the call is held to nlls_solve_pcg byte for byte, and its two new statistics to 1e-9 of the
host's (the bound tests/test_gpu_apply.py holds a trial to).  The bit rules are exact."""
import functools

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import blockindices
from tests.test_gpu_linearize import affine_two_groups, rel
from tests.test_gpu_apply import PROBLEMS, hub_problem
from tests.test_gpu_pcg import pcg_mirror, host_blocks, pd_lambda, swept, affine, system_state

pytestmark = pytest.mark.gpu
NONE, JACOBI = _capi.PCG_PRECOND_NONE, _capi.PCG_PRECOND_BLOCK_JACOBI
ELIMINATING = {"affine two groups": 558, "so3 adaptive": 117, "mixed linear3 + cost3": 562}
FRACTIONS = (0.001, 0.01, 0.05, 0.2, 0.5, 0.7, 0.9, 0.99, 0.999)


# ---- the reference --------------------------------------------------------------------------------------------------------------------------------------
def block_inverses(blocks, F):
    """the inverses of the diagonal blocks in precision F (longdouble: numpy's inverse, refined by two Newton steps X <- X (2 I - D X))"""
    out = []
    for d in blocks:
        X = np.linalg.inv(d).astype(F); D = d.astype(F); I2 = 2 * np.eye(d.shape[0], dtype=F)
        if F is not np.float64:
            for _ in range(2):
                X = X @ (I2 - D @ X)
        out.append(X)
    return out


def m_norm(y, blocks, bo):
    """||y||_M with M the diagonal blocks (None: the identity), in y's precision"""
    if blocks is None:
        return np.sqrt(y @ y)
    s = y.dtype.type(0)
    for k, d in enumerate(blocks):
        v = y[bo[k]:bo[k] + d.shape[0]]; s = s + v @ (d.astype(y.dtype) @ v)
    return np.sqrt(s)


class Exit:
    def __init__(self, y, iterations, status, yy, model, r):
        self.y, self.iterations, self.status, self.mnorm, self.model, self.rnorm = y, iterations, status, np.sqrt(yy), model, np.sqrt(r @ r)


def steihaug_mirror(matvec, blocks, bo, rhs, cap, rtol, radius, F=np.float64):
    """pcg_mirror inside ||y||_M <= radius, with the library's statuses: 0 converged and 1 the cap, inside the region; 4 the next iterate would leave it and 5 d'q <= 0:
    y goes to the boundary along d; 2 a scalar not finite, or d'q <= 0 without a finite radius; 3 a diagonal block without a Cholesky factor.  The norms come from
    the recurrences, never from a product with M.  matvec takes and returns precision F."""
    inv = None
    if blocks is not None:
        try:
            for d in blocks:
                np.linalg.cholesky(d)
        except np.linalg.LinAlgError:
            return Exit(np.zeros_like(rhs), 0, 3, 0.0, 0.0, np.zeros_like(rhs))
        inv = block_inverses(blocks, F)
    def prec(r):
        if inv is None:
            return r.copy()
        z = np.empty_like(r)
        for b, m in enumerate(inv):
            z[bo[b]:bo[b] + m.shape[0]] = m @ r[bo[b]:bo[b] + m.shape[0]]
        return z
    rhs = rhs.astype(F); y = np.zeros_like(rhs); r = rhs.copy(); z = prec(r); d = z.copy(); rz = r @ z; stop = rtol * np.sqrt(rhs @ rhs)
    yy = F(0); yp = F(0); pp = rz; model = F(0); bounded = np.isfinite(radius); r2 = F(radius) * F(radius) if bounded else F(np.inf)
    if np.sqrt(r @ r) <= stop:
        return Exit(y, 0, 0, yy, model, r)
    for it in range(1, cap + 1):
        q = matvec(d); dq = d @ q
        with np.errstate(all="ignore"):
            alpha = rz / dq
        ex = 0
        if bounded:
            if dq <= 0:
                ex = 5
            elif np.isfinite(alpha) and yy + 2 * alpha * yp + alpha * alpha * pp >= r2:
                ex = 4
        if ex:
            with np.errstate(all="ignore"):
                gap = r2 - yy; tau = gap / (yp + np.sqrt(yp * yp + pp * gap))
            if not (np.isfinite(tau) and tau >= 0):
                return Exit(y, it, 2, yy, model, r)
            return Exit(y + tau * d, it, ex, r2, model + tau * rz - tau * tau * dq / 2, r - tau * q)
        if not (dq > 0) or not np.isfinite(alpha):
            return Exit(y, it, 2, yy, model, r)
        y = y + alpha * d; r = r - alpha * q; yy = yy + 2 * alpha * yp + alpha * alpha * pp; model = model + alpha * rz / 2
        if np.sqrt(r @ r) <= stop:
            return Exit(y, it, 0, yy, model, r)
        z = prec(r); rz, old = r @ z, rz; beta = rz / old; d = z + beta * d
        yp = beta * (yp + alpha * pp); pp = rz + beta * beta * pp
    return Exit(y, cap, 1, yy, model, r)


def true_model(y, Al, b):
    return b @ y - (y @ (Al @ y)) / 2


def host_drift(Al, blocks, bo, b, cap, radius):
    """the float64 mirror on the host's matrix against the same mirror in longdouble -> (the float64 exit, drift of the norm, of the iterate, of the model value)"""
    m64 = steihaug_mirror(lambda v: Al @ v, blocks, bo, b, cap, 1e-10, radius)
    L = np.longdouble; AL = Al.astype(L)
    mld = steihaug_mirror(lambda v: AL @ v, blocks, bo, b, cap, 1e-10, radius, L)
    assert (m64.status, m64.iterations) == (mld.status, mld.iterations), "the float64 and the longdouble mirror part ways: the input is at fault"
    n64 = float(m_norm(m64.y, blocks, bo)); nld = float(m_norm(mld.y, blocks, bo))
    dn = max(abs(n64 - radius), abs(n64 - nld)) / radius
    dy = float(np.max(np.abs(m64.y - mld.y)) / np.max(np.abs(mld.y)))
    tm = float(true_model(mld.y, AL, b.astype(L))); dm = abs(float(m64.model) - tm) / abs(tm)
    assert max(dn, dy, dm) < 1e-9, f"the host mirror drifts by {dn:.2e} (norm) {dy:.2e} (iterate) {dm:.2e} (model): the input is at fault"
    return m64, dn, dy, dm


_HOST = {}


CROSSINGS = ((lambda k: k == 1, FRACTIONS), (lambda k: k >= 3, FRACTIONS))       # the smallest fraction that crosses in iteration 1, the smallest that crosses in one >= 3


def boundary_setup(name, pc, make=None, lam_of=None, wants=CROSSINGS):
    """the problem swept, damped with lambda = 1e-4 max|diag A| (or lam_of(A)), and -- computed ONCE per (name, pc) on the host -- the M-norm of the converged step and
    the radii `wants` asks for (by default two: the crossings in iteration 1 and in the first iteration >= 3), each with the drift of the host recurrences there"""
    p, unfixed = (make or PROBLEMS[name])()
    ctx, A, b, bo, bs = swept(p, unfixed); ndof = b.size
    if (name, pc) not in _HOST:
        lam = lam_of(A) if lam_of else 1e-4 * np.max(np.abs(np.diag(A)))
        Al = A + lam * np.eye(ndof); blocks = host_blocks(A, lam, bo, bs) if pc == JACOBI else None
        full = steihaug_mirror(lambda v: Al @ v, blocks, bo, b, 4 * ndof, 1e-10, np.inf)
        assert full.status == 0, f"{name}: the host mirror did not converge in {4 * ndof} iterations (status {full.status}): the input is at fault"
        nf = float(m_norm(full.y, blocks, bo)); picks = []
        assert abs(float(full.mnorm) - nf) <= 1e-9 * nf, "the recurrence of the norm left the true norm on the host: the input is at fault"
        for want, fractions in wants:
            for f in fractions:
                m = steihaug_mirror(lambda v: Al @ v, blocks, bo, b, 4 * ndof, 1e-10, f * nf)
                if m.status == 4 and want(m.iterations):
                    picks.append((f, m.iterations) + host_drift(Al, blocks, bo, b, 4 * ndof, f * nf)[1:]); break
        assert len(picks) == len(wants), f"{name}: no fraction of {FRACTIONS} crosses where the case wants it (by default in iteration 1 and in one >= 3): {picks}"
        _HOST[(name, pc)] = dict(lam=lam, nf=nf, full_iterations=full.iterations, picks=picks)
    H = _HOST[(name, pc)]; ctx.damp(H["lam"])
    return ctx, A, b, bo, bs, H


def check_boundary(tag, ctx, pc, lam, radius, Al, b, bo, drift, status=4, slack=0):
    """one call at `radius` against the mirror on the device's own operator -> (x, stats, the mirror's exit)"""
    dn, dy, dm = drift; tn, ty, tm = max(10 * dn, 1e-11), max(10 * dy, 1e-11), max(10 * dm, 1e-11)
    blocks = ctx.hess_block_diag(lam) if pc == JACOBI else None
    m = steihaug_mirror(lambda v: ctx.hess_apply(v, lam), blocks, bo, b, 4 * b.size, 1e-10, radius)
    x, st = ctx.solve_pcg_tr(radius, pc, None, 1e-10, want_x=True); y = -x
    en = abs(float(m_norm(y, blocks, bo)) - radius) / radius; ey = rel(y, m.y); host = true_model(y, Al, b); em = abs(st["model"] - host) / abs(host)
    er = abs(st["rnorm"] - np.linalg.norm(b - Al @ y)) / np.linalg.norm(b)
    print(f"PCGTR {tag} precond {pc} radius {radius:.6e}: status {st['status']} iteration {st['iterations']} (mirror {m.status}, {m.iterations}); ||x||_M against the radius "
          f"{en:.3e} (of {tn:.1e}, host drift {dn:.2e}); against the mirror's iterate {ey:.3e} (of {ty:.1e}, host drift {dy:.2e}); model {st['model']:.12e} against the host's "
          f"{em:.3e} (of {tm:.1e}, host drift {dm:.2e}); residual at the returned point against the true one {er:.2e} of ||b||")
    assert m.status == status, f"{tag}: the mirror on the device's operator ended with status {m.status}: the input is at fault"
    assert st["status"] == status and abs(st["iterations"] - m.iterations) <= slack, (tag, st, m.iterations)
    assert x.tobytes() == ctx.get_step().tobytes()
    assert st["mnorm"] == radius and en <= tn, tag
    assert ey <= ty, tag
    assert st["model"] > 0 and em <= tm, tag
    assert er <= 1e-9, tag                               # (the recurrence's residual against the true one: rounding, as in tests/test_gpu_pcg.py)
    return x, st, m


# ---- 1. an infinite radius is nlls_solve_pcg --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _capi.FLAG_MATERIALIZE], ids=["default", "materialize"])
def test_infinite_radius_is_the_plain_solve(flags):
    ctx, A, b, bo, bs, lam, k = affine(flags); Al = A + lam * np.eye(b.size)
    for pc in (JACOBI, NONE):
        blocks = host_blocks(A, lam, bo, bs) if pc == JACOBI else None
        assert pcg_mirror(lambda v: Al @ v, blocks, bo, b, 4 * b.size, 1e-10)[2] == 0, "the host mirror did not converge: the input is at fault"
        x0, s0 = ctx.solve_pcg(pc, None, 1e-10, want_x=True); s0 = dict(s0)
        x1, s1 = ctx.solve_pcg_tr(np.inf, pc, None, 1e-10, want_x=True)
        assert s0["status"] == 0 and x1.tobytes() == x0.tobytes() and x1.tobytes() == ctx.get_step().tobytes()
        assert {key: s1[key] for key in s0} == s0, (s0, s1)            # iterations, status, ||b||, ||r||, synchronisations AND launches: none was added
        y = -x1; hn = float(m_norm(y, blocks, bo)); hm = true_model(y, Al, b)
        en, em = abs(s1["mnorm"] - hn) / hn, abs(s1["model"] - hm) / hm
        print(f"PCGTR infinite radius flags {flags} precond {pc}: {s1['iterations']} iterations, {s1['launches']} launches; ||x||_M {s1['mnorm']:.9e} against the host's "
              f"{en:.3e}, model {s1['model']:.9e} against the host's {em:.3e} (of 1e-9)")
        assert en <= 1e-9 and em <= 1e-9 and hm > 0
        x5, s5 = ctx.solve_pcg_tr(np.inf, pc, 5, 1e-10, want_x=True)     # truncated: as nlls_solve_pcg truncates
        assert (s5["status"], s5["iterations"]) == (1, 5) and x5.tobytes() == ctx.solve_pcg(pc, 5, 1e-10, want_x=True)[0].tobytes()
    ctx.close()


# ---- 2. boundary exits ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [NONE, JACOBI], ids=["none", "blockjacobi"])
@pytest.mark.parametrize("name", list(ELIMINATING))
def test_boundary_exits(name, pc):
    ctx, A, b, bo, bs, H = boundary_setup(name, pc); lam = H["lam"]; Al = A + lam * np.eye(b.size)
    assert b.size == ELIMINATING[name] and ctx.info.nschur_blocks > 0
    assert H["picks"][0][1] == 1 and H["picks"][1][1] >= 3
    for f, k, dn, dy, dm in H["picks"]:
        _, st, m = check_boundary(f"{name} at {f} of the converged norm ({H['full_iterations']} iterations)", ctx, pc, lam, f * H["nf"], Al, b, bo, (dn, dy, dm))
        assert m.iterations == k, f"{name}: the mirror on the device's operator crosses in iteration {m.iterations}, on the host's matrix in {k}: the input is at fault"
    ctx.close()


# ---- 3. non-positive curvature ----------------------------------------------------------------------------------------------------------------------------
def own_drift(matvec, blocks, bo, b, radius):
    """where no longdouble run is possible (the device's operator) or wanted: the float64 mirror's own distance between its true norm and the radius"""
    m = steihaug_mirror(matvec, blocks, bo, b, 4 * b.size, 1e-10, radius)
    return m, abs(float(m_norm(m.y, blocks, bo)) - radius) / radius


def refused(ctx, pc, radius, status):
    ndof = ctx.info.ndof; sentinel = np.linspace(-1.0, 2.0, ndof); ctx.set_step(sentinel); before = system_state(ctx)
    out = np.full(ndof, 7.25); st = np.full(8, -1.0)
    rc = ctx.L.nlls_solve_pcg_tr(ctx.h, pc, 4 * ndof, 1e-10, radius, _capi._p(out), _capi._p(st))
    assert rc == _capi.ERR_NOT_SPD and int(st[1]) == status, (rc, st)
    assert np.all(out == 7.25) and ctx.get_step().tobytes() == sentinel.tobytes() and system_state(ctx) == before
    with pytest.raises(_capi.NllsError) as e:
        ctx.solve_pcg_tr(radius, pc, None, 1e-10)
    assert e.value.code == _capi.ERR_NOT_SPD and ctx.last_pcg_tr["status"] == status
    return int(st[0])


def test_negative_curvature_without_a_preconditioner():
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); ndof = b.size
    low = np.linalg.eigvalsh(A)[0]
    assert low < 0, f"the smallest eigenvalue of A is {low}: the input is at fault"
    lam4 = 1e-4 * np.max(np.abs(np.diag(A))); radius = float(np.linalg.norm(np.linalg.solve(A + lam4 * np.eye(ndof), b)))
    first, d1 = own_drift(lambda v: A @ v, None, bo, b, radius)
    assert first.status in (4, 5), f"the host mirror ended with status {first.status} inside the step of lambda {lam4:.3e}: the input is at fault"
    dev, dd = own_drift(lambda v: ctx.hess_apply(v, 0.0), None, bo, b, radius)
    x, st = ctx.solve_pcg_tr(radius, NONE, None, 1e-10, want_x=True); en = abs(np.linalg.norm(x) - radius) / radius
    print(f"PCGTR lambda 0, smallest eigenvalue {low:.4f}, radius {radius:.4e}: host status {first.status} iteration {first.iterations}, device {st['status']}, "
          f"{st['iterations']}; ||x|| against the radius {en:.3e} (mirror's own {dd:.2e})")
    assert st["status"] == dev.status and abs(st["iterations"] - dev.iterations) <= 1 and en <= max(10 * dd, 1e-11) and st["mnorm"] == radius and st["model"] > 0
    # a radius so large that the curvature is met first
    big = radius
    for _ in range(12):
        if steihaug_mirror(lambda v: A @ v, None, bo, b, 4 * ndof, 1e-10, big).status == 5:
            break
        big *= 10.0
    host = steihaug_mirror(lambda v: A @ v, None, bo, b, 4 * ndof, 1e-10, big)
    assert host.status == 5, "no radius up to 1e12 times the first lets the host mirror meet the curvature: the input is at fault"
    dev, dd = own_drift(lambda v: ctx.hess_apply(v, 0.0), None, bo, b, big); assert dev.status == 5
    x, st = ctx.solve_pcg_tr(big, NONE, None, 1e-10, want_x=True); en = abs(np.linalg.norm(x) - big) / big; y = -x
    print(f"PCGTR negative curvature, radius {big:.4e}: host iteration {host.iterations}, mirror on the device's operator {dev.iterations}, device {st['iterations']}; "
          f"||x|| against the radius {en:.3e} (mirror's own {dd:.2e}); model {st['model']:.9e} (host's {true_model(y, A, b):.9e}); p'Hp at the exit <= 0")
    assert st["status"] == 5 and abs(st["iterations"] - dev.iterations) <= 1 and en <= max(10 * dd, 1e-11) and st["mnorm"] == big and st["model"] > 0
    assert x.tobytes() == ctx.get_step().tobytes() and true_model(y, A, b) > 0
    # block Jacobi: a diagonal block has no factor -- status 3; no boundary to go to -- status 2; both leave everything as it was
    assert steihaug_mirror(lambda v: A @ v, host_blocks(A, 0.0, bo, bs), bo, b, 4 * ndof, 1e-10, big).status == 3, "every diagonal block has a Cholesky factor: the input is at fault"
    assert refused(ctx, JACOBI, big, 3) == 0
    inf = steihaug_mirror(lambda v: A @ v, None, bo, b, 4 * ndof, 1e-10, np.inf); assert inf.status == 2
    assert abs(refused(ctx, NONE, np.inf, 2) - inf.iterations) <= 1
    ctx.close()


def test_negative_curvature_under_block_jacobi():
    """a damping below zero, between the smallest eigenvalue of A (0.0854) and that of its diagonal blocks (0.465): every block keeps its factor, the matrix does not.
    lambda = -2 lambda_min(A), taken from the host's eigenvalue: at -1.3e-5 max|diag A| = -0.0852 the oracle's linearisation of this problem is still positive definite
    by 2.5e-4, and the host mirror converges at every radius (notes/r25.md)"""
    p, unfixed = PROBLEMS["mixed linear3 + cost3"](); ctx, A, b, bo, bs = swept(p, unfixed); ndof = b.size
    lam = -2.0 * np.linalg.eigvalsh(A)[0]; Al = A + lam * np.eye(ndof); blocks = host_blocks(A, lam, bo, bs)        # (A + lambda I then has the eigenvalue -0.0854)
    low = np.linalg.eigvalsh(Al)[0]; lowb = min(np.linalg.eigvalsh(d)[0] for d in blocks)
    assert low < 0 < lowb, f"smallest eigenvalue of A + lambda I {low}, of its diagonal blocks {lowb}: the input is at fault"
    ctx.damp(lam); big = 1.0
    for _ in range(16):
        if steihaug_mirror(lambda v: Al @ v, blocks, bo, b, 4 * ndof, 1e-10, big).status == 5:
            break
        big *= 10.0
    host = steihaug_mirror(lambda v: Al @ v, blocks, bo, b, 4 * ndof, 1e-10, big)
    assert host.status == 5, f"the host mirror ends with status {host.status} at every radius up to 1e16: the input is at fault"
    dblocks = ctx.hess_block_diag(lam)
    dev, dd = own_drift(lambda v: ctx.hess_apply(v, lam), dblocks, bo, b, big); assert dev.status == 5
    x, st = ctx.solve_pcg_tr(big, JACOBI, None, 1e-10, want_x=True); y = -x; en = abs(float(m_norm(y, dblocks, bo)) - big) / big
    print(f"PCGTR negative curvature under block Jacobi, lambda {lam:.3e} (eigenvalues {low:.3e} / blocks {lowb:.3e}), radius {big:.1e}: host iteration {host.iterations}, "
          f"mirror on the device's operator {dev.iterations}, device {st['iterations']}; ||x||_M against the radius {en:.3e} (mirror's own {dd:.2e}); model {st['model']:.9e}")
    assert st["status"] == 5 and abs(st["iterations"] - dev.iterations) <= 1 and en <= max(10 * dd, 1e-11) and st["mnorm"] == big and st["model"] > 0
    assert true_model(y, Al, b) > 0 and x.tobytes() == ctx.get_step().tobytes()
    ctx.close()


# ---- 4. the bit rules -------------------------------------------------------------------------------------------------------------------------------------
def test_bit_rules():
    name = "affine two groups"
    ctx, A, b, bo, bs, H = boundary_setup(name, JACOBI); lam = H["lam"]; Al = A + lam * np.eye(b.size); f, k, dn, dy, dm = H["picks"][1]; r4 = f * H["nf"]
    assert b.size % 256 != 0 and b.size > 2 * 256                         # three workgroups by default: late ones exist
    x4, s4 = ctx.solve_pcg_tr(r4, JACOBI, None, 1e-10, want_x=True); x4b, s4b = ctx.solve_pcg_tr(r4, JACOBI, None, 1e-10, want_x=True)
    assert s4["status"] == 4 and s4["iterations"] == k and x4.tobytes() == x4b.tobytes() and s4 == s4b, "two calls on the same sweep differ"
    for rnd in (1, 3, 1000):
        ctx.set_option(_capi.OPT_PCG_ROUND, rnd)
        x, st = ctx.solve_pcg_tr(r4, JACOBI, None, 1e-10, want_x=True)
        print(f"PCGTR status 4, round {rnd}: iterations {st['iterations']} synchronisations {st['rounds']} launches {st['launches']}")
        assert x.tobytes() == x4.tobytes() and (st["status"], st["iterations"], st["mnorm"], st["model"], st["rnorm"]) == (4, k, s4["mnorm"], s4["model"], s4["rnorm"]), rnd
        assert st["rounds"] == -(-k // rnd) + 1, (rnd, st)
    ctx.set_option(_capi.OPT_PCG_ROUND, 1); ctx.set_option(_capi.OPT_PCG_GRID_MAX, 1)             # one workgroup does everything
    x, st, _ = check_boundary("one workgroup", ctx, JACOBI, lam, r4, Al, b, bo, (dn, dy, dm))
    assert rel(x, x4) <= max(10 * dy, 1e-11) and st["iterations"] == k
    ctx.close()
    # the exit on the curvature: affine two groups at lambda 0 without a preconditioner, the radius of test_negative_curvature_without_a_preconditioner
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); big = 1e6 * float(np.linalg.norm(b))
    assert steihaug_mirror(lambda v: A @ v, None, bo, b, 4 * b.size, 1e-10, big).status == 5, "the host mirror does not meet the curvature: the input is at fault"
    x5, s5 = ctx.solve_pcg_tr(big, NONE, None, 1e-10, want_x=True); assert s5["status"] == 5
    for rnd in (1, 3, 1000):
        ctx.set_option(_capi.OPT_PCG_ROUND, rnd)
        x, st = ctx.solve_pcg_tr(big, NONE, None, 1e-10, want_x=True)
        print(f"PCGTR status 5, round {rnd}: iterations {st['iterations']} synchronisations {st['rounds']} launches {st['launches']}")
        assert x.tobytes() == x5.tobytes() and (st["status"], st["iterations"], st["model"]) == (5, s5["iterations"], s5["model"]), rnd
    ctx.close()


def small_hub():
    """the first hub shape of tests/test_gpu_apply.py::HUBS with three of its variables fixed: 62 unknowns, fewer than a wavefront has lanes"""
    p = hub_problem(61, 1)[0]; unfixed = np.ones(p.nvariables, bool); unfixed[:3] = False
    return p, unfixed


@pytest.mark.parametrize("pc", [NONE, JACOBI], ids=["none", "blockjacobi"])
def test_fewer_unknowns_than_a_wavefront(pc):
    """(its conjugate gradients converge in a handful of iterations: the smallest fraction, which crosses in iteration 1, and the largest, wherever it crosses)"""
    ctx, A, b, bo, bs, H = boundary_setup("hub of 61", pc, small_hub, pd_lambda, ((lambda k: k == 1, FRACTIONS), (lambda k: True, FRACTIONS[::-1])))
    lam = H["lam"]; Al = A + lam * np.eye(b.size)
    assert b.size < 64
    for f, k, dn, dy, dm in H["picks"]:
        _, st, m = check_boundary(f"hub of 61 at {f} of the converged norm", ctx, pc, lam, f * H["nf"], Al, b, bo, (dn, dy, dm))
        assert m.iterations == k
    ctx.close()


# ---- 5. state and refusals --------------------------------------------------------------------------------------------------------------------------------
def test_calls_leave_the_linear_system_untouched():
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed, _capi.FLAG_MATERIALIZE); ndof = b.size
    lam = 1e-2 * np.max(np.abs(np.diag(A))); ctx.damp(lam); Al = A + lam * np.eye(ndof)
    assert pcg_mirror(lambda v: Al @ v, host_blocks(A, lam, bo, bs), bo, b, 4 * ndof, 1e-10)[2] == 0, "the host mirror did not converge: the input is at fault"
    x0, s0 = ctx.solve_pcg(JACOBI, None, 1e-10, want_x=True); counters = ctx.solve_stats(); last = dict(ctx.last_pcg)
    probe = np.cos(np.arange(ndof)); ctx.set_step(probe); damped = ctx.quadform()                # x'(H + lambda I)x: the damping the context holds
    before = system_state(ctx)
    radius = 0.3 * float(m_norm(-x0, host_blocks(A, lam, bo, bs), bo))
    x, st = ctx.solve_pcg_tr(radius, JACOBI, None, 1e-10, want_x=True)
    assert st["status"] == 4 and 0 < st["iterations"] < s0["iterations"] and system_state(ctx) == before
    after = ctx.solve_stats()
    assert all(counters[key] == after[key] for key in counters if not key.startswith("apply")), (counters, after)       # [53..55] still describe the last nlls_solve_pcg
    assert (after["pcg_iterations"], after["pcg_status"]) == (s0["iterations"], 0) and ctx.last_pcg == last
    # the step is the caller's: nlls_get_step, nlls_step_norm, nlls_step_maxabs, nlls_retract
    assert ctx.get_step().tobytes() == x.tobytes() and abs(ctx.step_norm() - np.linalg.norm(x)) <= 1e-11 * np.linalg.norm(x) and abs(ctx.step_maxabs() - np.max(np.abs(x))) <= 1e-11 * np.max(np.abs(x))
    ctx.retract(_capi.VARS_NEXT, _capi.VARS_CURRENT); got = ctx.get_variables(_capi.VARS_NEXT).tobytes()
    ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT); ctx.set_step(x); ctx.retract(_capi.VARS_NEXT, _capi.VARS_CURRENT)
    assert got == ctx.get_variables(_capi.VARS_NEXT).tobytes() and got != ctx.get_variables(_capi.VARS_CURRENT).tobytes()
    ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT)
    ctx.set_step(probe); assert ctx.quadform() == damped and system_state(ctx) == before
    # a refused call: the damping taken down to 0 exactly, where a diagonal block has no factor
    ctx.damp(-lam)
    assert pcg_mirror(lambda v: A @ v, host_blocks(A, 0.0, bo, bs), bo, b, 4 * ndof, 1e-10)[2] == 3, "every diagonal block has a factor at lambda 0: the input is at fault"
    ctx.set_step(probe); undamped = ctx.quadform()
    refused(ctx, JACOBI, radius, 3)
    ctx.set_step(probe); assert ctx.quadform() == undamped and ctx.solve_stats()["pcg_iterations"] == s0["iterations"] and ctx.last_pcg == last
    ctx.close()


def test_refusals():
    p, unfixed = affine_two_groups(); L = _capi.lib(); P = _capi._p
    ctx = _capi.Context(); out = np.full(600, 7.25); st = np.full(8, 7.25)
    call = lambda radius=1.0, pc=JACOBI, mi=10, rtol=1e-8: L.nlls_solve_pcg_tr(ctx.h, pc, mi, rtol, radius, P(out), P(st))
    assert call() == _capi.ERR_NOT_READY                                                                          # no upload yet
    ctx.upload(p.var_kind, p.var_dim, blockindices(p, unfixed), p.groups()); ctx.set_variables(p.variables)
    assert call() == _capi.ERR_NOT_READY                                                                          # no sweep yet
    ctx.sweep_gradhess(); ctx.damp(1e-2 * ctx.max_abs_diag()); sentinel = np.linspace(-1.0, 2.0, ctx.info.ndof); ctx.set_step(sentinel)
    for radius in (0.0, -0.0, -1.0, -np.inf, np.nan):
        assert call(radius) == _capi.ERR_INVALID_ARG, radius
    for kw in (dict(pc=-1), dict(pc=2), dict(mi=0), dict(mi=-3), dict(rtol=np.nan), dict(rtol=np.inf), dict(rtol=-1e-3)):
        assert call(**kw) == _capi.ERR_INVALID_ARG, kw
    assert np.all(out == 7.25) and np.all(st == 7.25) and ctx.get_step().tobytes() == sentinel.tobytes(), "a refused call wrote to an output"
    assert L.nlls_solve_pcg_tr(ctx.h, JACOBI, 100, 1e-8, np.inf, None, None) == _capi.OK                           # both outputs may be NULL; +inf is a radius
    assert call(1e-3) == _capi.OK and int(st[1]) == 4 and st[6] == 1e-3 and st[7] > 0 and np.all(out[:558] != 7.25) and np.all(out[558:] == 7.25)
    ctx.close()
    # every variable fixed: ndof == 0
    from nllssolver_jl_amd import kinds as K
    q = N.NLLSProblem(); a = q.addvariable([0.1, 0.2, 0.3]); q.addcosts(K.RES_LINEAR3, [[a]], np.random.default_rng(2).standard_normal((1, 12)))
    ctx = _capi.Context(); ctx.upload(q.var_kind, q.var_dim, blockindices(q, np.zeros(1, bool)), q.groups()); ctx.set_variables(q.variables); ctx.sweep_gradhess()
    out[:] = 7.25; st[:] = 7.25
    assert ctx.info.ndof == 0 and call() == _capi.OK and np.all(out == 7.25) and np.all(st == 0.0)
    ctx.close()
    # b == 0: status 0, no iteration, x = 0
    q = N.NLLSProblem(); a = q.addvariable([0.0, 0.0, 0.0]); q.addcosts(K.RES_LINEAR3, [[a]], np.concatenate((np.eye(3).ravel(), np.zeros(3)))[None, :])
    ctx = _capi.Context(); ctx.upload(q.var_kind, q.var_dim, blockindices(q), q.groups()); ctx.set_variables(q.variables); ctx.sweep_gradhess()
    assert np.all(ctx.get_grad() == 0.0), "the gradient of the zero residual is not zero: the input is at fault"
    x, s = ctx.solve_pcg_tr(2.0, NONE, None, 1e-8, want_x=True)
    assert (s["status"], s["iterations"], s["mnorm"], s["model"]) == (0, 0, 0.0, 0.0) and np.all(x == 0.0)
    ctx.close()


def test_sharded_contexts_are_refused():
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)
    c = _capi.Context()
    try:
        c.set_shard(0, 2); c.upload(p.var_kind, p.var_dim, blockindices(p), p.groups(), _capi.FLAG_FORCE_SPARSE); c.set_variables(p.variables)
        assert c.shard_info()["nranks"] == 2 and c.shard_info()["replicated"] == 0
        c.sweep_gradhess_local()
        out = np.full(c.info.ndof, 7.25); st = np.full(8, 7.25)
        assert c.L.nlls_solve_pcg_tr(c.h, JACOBI, 10, 1e-8, 1.0, _capi._p(out), _capi._p(st)) == _capi.ERR_UNSUPPORTED and np.all(out == 7.25) and np.all(st == 7.25)
    finally:
        c.close()


# ---- 6. optimize ------------------------------------------------------------------------------------------------------------------------------------------
def problem_a(robust=None):
    kw = dict(robust=robust) if robust is not None else {}
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3, **kw), 1e-3, 1e-3)
    unfixed = np.ones(p.nvariables, bool); unfixed[[0, 1]] = False
    return p, unfixed


OPTIMIZE = {"ba 10 x 200, two cameras fixed": problem_a, "the same under Huber(0.002)": lambda: problem_a(N.HuberKernel(0.002)),
            "mixed linear3 + cost3": PROBLEMS["mixed linear3 + cost3"]}


@functools.lru_cache(maxsize=None)
def levenberg_marquardt(name):
    p, unfixed = OPTIMIZE[name](); res = N.optimize(p, N.NLLSOptions(maxiters=100), unfixed)
    return res.startcost, res.bestcost, res.niterations


@pytest.mark.parametrize("precond", ["none", "blockjacobi"])
@pytest.mark.parametrize("name", list(OPTIMIZE))
def test_optimize_with_steihaug(name, precond):
    """the final cost is Levenberg-Marquardt's, to 1e-15 of the start cost: the bound tests/test_gpu_schur.py::test_optimize_with_reduced_pcg_steps holds its runs to"""
    start, control, nlm = levenberg_marquardt(name)
    p, unfixed = OPTIMIZE[name](); statuses = []
    def watch(cost, problem, data, sd):
        statuses[:] = sd.statuses
        return cost, 0
    res = N.optimize(p, N.NLLSOptions(maxiters=100, iterator=N.steihaug, linearsolver=N.PCG(rtol=1e-2, precond=precond)), unfixed, callback=watch)
    print(f"STEIHAUG optimize {name} precond {precond}: cost {res.startcost:.6e} -> {res.bestcost:.12e} in {res.niterations} iterations, {res.linearsolvers} trials, exits "
          f"{ {s: statuses.count(s) for s in sorted(set(statuses))} }; Levenberg-Marquardt {control:.12e} in {nlm}; difference {abs(res.bestcost - control):.3e} "
          f"(of {1e-15 * start:.3e})")
    assert res.startcost == start and res.linearsolvers > 0 and all(s in (0, 1, 4, 5) for s in statuses)
    assert abs(res.bestcost - control) <= 1e-15 * start, name


@pytest.mark.parametrize("name", ["affine two groups", "so3 adaptive"])
def test_optimize_descends_where_the_hessian_is_indefinite(name):
    """gauge-free or slow: both methods stop on their caps at different points, so only the descent is asserted -- and that the trust region was met"""
    p, unfixed = PROBLEMS[name](); costs = []; statuses = []
    def watch(cost, problem, data, sd):
        costs.append(cost); statuses[:] = sd.statuses
        return cost, 0
    res = N.optimize(p, N.NLLSOptions(maxiters=15, iterator=N.steihaug, linearsolver=N.PCG(rtol=1e-2, precond="none")), unfixed, callback=watch)
    print(f"STEIHAUG optimize {name}: cost {res.startcost:.6e} -> {res.bestcost:.6e} in {res.niterations} iterations, {res.linearsolvers} trials, exits "
          f"{ {s: statuses.count(s) for s in sorted(set(statuses))} }")
    assert len(costs) >= 2 and all(c1 <= c0 for c0, c1 in zip([res.startcost] + costs, costs)), costs
    assert res.bestcost < res.startcost and any(s in (4, 5) for s in statuses), statuses
