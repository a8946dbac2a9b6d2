"""Shared helpers for the tests: build oracle problems from host NLLSProblem objects."""
import numpy as np

from oracle import oracle as O


def oracle_problem(problem):
    """The same packed description that crosses the C ABI, handed to the CPU oracle."""
    op = O.OracleProblem(problem.var_kind, problem.var_dim, problem.groups())
    op.set_variables(problem.variables)
    return op


def blockindices(problem, unfixed=None):
    """linearsystem.jl:93-102: 1-based block number per variable, 0 = fixed."""
    n = problem.nvariables
    unfixed = np.ones(n, bool) if unfixed is None else np.asarray(unfixed, bool)
    bi = np.zeros(n, np.uint64)
    bi[unfixed] = np.arange(1, unfixed.sum() + 1, dtype=np.uint64)
    return bi


def bsm_to_csr(index, data, ndof):
    """The symmetric H of a block-sparse linear system as scipy CSR, from the BlockSparseMatrix layout (src/BlockSparseMatrix.jl:30-47): index = (colptr, rowval,
    nzval, boffsets) as nlls_get_bsm_index returns them (1-based), data = A.data.  Block rows hold the blocks at or left of the diagonal; diagonal blocks full."""
    import scipy.sparse as sp
    cp, rv, nz, bo = (np.asarray(a, np.int64) for a in index); nb = len(cp) - 1
    bo0 = bo - 1; bs = np.diff(np.r_[bo0, ndof])
    rows = np.repeat(np.arange(nb), np.diff(cp)); cols = rv - 1; offs = nz - 1
    I, J, V = [], [], []
    for (br, bc) in {(int(a), int(b)) for a, b in zip(bs[rows], bs[cols])}:
        m = (bs[rows] == br) & (bs[cols] == bc)
        r0, c0, o0 = bo0[rows[m]], bo0[cols[m]], offs[m]
        ii, jj = np.meshgrid(np.arange(br), np.arange(bc), indexing="ij")          # a block is column-major br x bc
        idx = o0[:, None, None] + ii[None] + br * jj[None]
        I.append((r0[:, None, None] + ii[None]).ravel()); J.append((c0[:, None, None] + jj[None]).ravel()); V.append(data[idx].ravel())
    L = sp.coo_matrix((np.concatenate(V), (np.concatenate(I), np.concatenate(J))), shape=(ndof, ndof)).tocsr()
    strict = sp.tril(L, -1)
    return (strict + strict.T + sp.diags(L.diagonal())).tocsr()


def device_solve_residual(ctx, lam):
    """|| (H + lam I) x + g || / || g ||  of the device's own damped solve -- H, g as its gradient sweep left them, x as nlls_solve returns it: a check of the
    linear solve that needs no second solver (sizes the oracle's factorisation would take minutes for)."""
    H = bsm_to_csr(ctx.bsm_index(), ctx.get_bsm_data(), ctx.info.ndof); g = ctx.get_grad()
    ctx.damp(lam); x = ctx.solve(want_x=True)
    return float(np.linalg.norm(H @ x + lam * x + g) / np.linalg.norm(g))


# ---- extended-precision reference of the damped step ---------------------------------------------------------------------------------------
# The step of a damped Gauss-Newton system is checked against a tolerance on x that conditioning sets (kappa ~ 1e6 at lambda = 1e-6 max|diag| on a
# gauge-free problem): a kernel error at the 1e-12 .. 1e-10 level passes it.  The normwise backward error below does not depend on conditioning; it
# is formed in x86-64 extended precision (64-bit significand), so the rounding of the measure itself stays ~1e-19 below what a float64 solve can reach.
assert np.finfo(np.longdouble).nmant >= 63, "the extended-precision references need an 80-bit long double (x86-64)"
LD = np.longdouble


def bsm_coo(index, data, ndof):
    """(rows, cols, values) of the STORED half of the block-sparse H (blocks at or left of the diagonal, diagonal blocks full), values as stored:
    the layout of bsm_to_csr without the cast to scipy (float64 sums)."""
    cp, rv, nz, bo = (np.asarray(a, np.int64) for a in index); nb = len(cp) - 1
    bo0 = bo - 1; bs = np.diff(np.r_[bo0, ndof])
    rows = np.repeat(np.arange(nb), np.diff(cp)); cols = rv - 1; offs = nz - 1
    I, J, V = [], [], []
    for (br, bc) in sorted({(int(a), int(b)) for a, b in zip(bs[rows], bs[cols])}):
        m = (bs[rows] == br) & (bs[cols] == bc)
        r0, c0, o0 = bo0[rows[m]], bo0[cols[m]], offs[m]
        ii, jj = np.meshgrid(np.arange(br), np.arange(bc), indexing="ij")
        idx = o0[:, None, None] + ii[None] + br * jj[None]
        I.append((r0[:, None, None] + ii[None]).ravel()); J.append((c0[:, None, None] + jj[None]).ravel()); V.append(np.asarray(data)[idx].ravel())
    I, J, V = np.concatenate(I), np.concatenate(J), np.concatenate(V)
    keep = I >= J                                            # (a diagonal block's upper half is its lower half's mirror)
    return I[keep], J[keep], V[keep]


def _ld_sym_matvec(I, J, V, x, n):
    """(H x) in long double from the lower half (I >= J) of a symmetric H: every product and every sum in extended precision (np.add.at, not bincount)."""
    V, x = V.astype(LD), np.asarray(x).astype(LD)
    y = np.zeros(n, LD)
    np.add.at(y, I, V * x[J])
    s = I != J
    np.add.at(y, J[s], V[s] * x[I[s]])
    return y


def _ld_sym_rowabs(I, J, V, lam, n):
    """the row sums of |H + lam I| in long double, from the lower half of H."""
    V = V.astype(LD); r = np.zeros(n, LD); dg = np.zeros(n, LD)
    d = I == J
    np.add.at(r, I[~d], np.abs(V[~d])); np.add.at(r, J[~d], np.abs(V[~d])); np.add.at(dg, I[d], V[d])
    return r + np.abs(dg + LD(lam))


def longdouble_backward_error(A_data, bsm_index, b, lam, x):
    """eta = || (H + lam I) x + g ||_inf / ( || H + lam I ||_inf || x ||_inf + || g ||_inf ) in long double: H, g the linearisation as A.data / b hold it
    (the oracle's ols.data, ols.b) through the BlockSparseMatrix layout of bsm_to_csr -- or, bsm_index None, a dense system's full column-major n x n
    A.data (its lower triangle is read).  A backward-stable solve gives eta ~ u = 1.1e-16 whatever the conditioning; an error in one entry of the
    factorisation shows at (its relative size) x (its share of ||H||)."""
    ndof = len(b)
    if bsm_index is None:
        J, I = np.triu_indices(ndof); V = np.asarray(A_data).reshape(ndof, ndof)[J, I]     # (column-major: data[col * n + row], row >= col)
    else:
        I, J, V = bsm_coo(bsm_index, A_data, ndof)
    xl, gl = np.asarray(x).astype(LD), np.asarray(b).astype(LD)
    r = _ld_sym_matvec(I, J, V, xl, ndof) + LD(lam) * xl + gl
    nH = np.max(_ld_sym_rowabs(I, J, V, lam, ndof))
    return float(np.max(np.abs(r)) / (nH * np.max(np.abs(xl)) + np.max(np.abs(gl))))


def _ld_ldlt_solve(M, rhs):
    """Solve M X = rhs (M symmetric, long double) by a plain LDL' without pivoting, right-looking: for the damped (positive definite) systems here."""
    A = np.array(M, LD, copy=True); n = A.shape[0]; X = np.array(rhs, LD, copy=True)
    if X.ndim == 1: X = X[:, None]
    d = np.zeros(n, LD)
    for j in range(n):
        d[j] = A[j, j]
        assert d[j] > 0, f"pivot {j} of the damped system is {d[j]}"
        l = A[j + 1:, j] / d[j]
        A[j + 1:, j + 1:] -= np.outer(l, A[j + 1:, j])
        A[j + 1:, j] = l
    for j in range(n):                      # L y = rhs
        X[j + 1:] -= np.outer(A[j + 1:, j], X[j])
    X /= d[:, None]
    for j in range(n - 1, -1, -1):          # L' x = y / d
        X[j] -= A[j + 1:, j] @ X[j + 1:]
    return X


def longdouble_schur_step(A_data, bsm_index, b, lam, elim_blocks):
    """An independent reference of the damped step x = -(H + lam I)^-1 g in long double, for small problems: every eliminated block v (elim_blocks: a
    boolean per block, an independent set -- no two share a stored block) is eliminated with its own (C_v + lam I)^-1, the dense reduced system
    S = H_RR + lam I - sum_v E_v (C_v + lam I)^-1 E_v' is factored by a plain long-double LDL' (n <= ~500), and the eliminated unknowns follow by
    back-substitution.  Returns (x_ref, S as float64) -- S for the conditioning that bounds how far a float64 step may lie from x_ref."""
    ndof = len(b); cp, rv, nz, bo = (np.asarray(a, np.int64) for a in bsm_index); nb = len(cp) - 1
    bo0 = bo - 1; bs = np.diff(np.r_[bo0, ndof]); elim = np.asarray(elim_blocks, bool); assert elim.size == nb
    I, J, V = bsm_coo(bsm_index, A_data, ndof)
    blk = np.repeat(np.arange(nb), bs)                                    # block of every dof
    edof = elim[blk]; red = np.nonzero(~edof)[0]; nr = red.size
    rpos = -np.ones(ndof, np.int64); rpos[red] = np.arange(nr)
    assert not np.any(edof[I] & edof[J] & (blk[I] != blk[J])), "two eliminated blocks share a stored block"
    g = np.asarray(b).astype(LD); V = V.astype(LD)
    S = np.zeros((nr, nr), LD); s = -g[red].copy()
    rr = ~edof[I] & ~edof[J]
    S[rpos[I[rr]], rpos[J[rr]]] += V[rr]; o = rr & (I != J); S[rpos[J[o]], rpos[I[o]]] += V[o]
    S[np.arange(nr), np.arange(nr)] += LD(lam)
    # the eliminated blocks: C_v (its diagonal block) and E_v (its reduced rows), in one pass over the coupling entries
    ce = edof[I] & edof[J]; er = edof[I] != edof[J]
    pe, pr = np.where(edof[I], I, J)[er], np.where(edof[I], J, I)[er]; ve = V[er]     # (eliminated dof, reduced dof, value)
    order = np.argsort(blk[pe], kind="stable"); pe, pr, ve = pe[order], pr[order], ve[order]
    eb = np.nonzero(elim)[0]; starts = np.searchsorted(blk[pe], eb), np.searchsorted(blk[pe], eb, side="right")
    cI, cJ, cV = I[ce], J[ce], V[ce]; corder = np.argsort(blk[cI], kind="stable"); cI, cJ, cV = cI[corder], cJ[corder], cV[corder]
    cs = np.searchsorted(blk[cI], eb), np.searchsorted(blk[cI], eb, side="right")
    sol = {}
    for k, v in enumerate(eb):
        d0, dv = bo0[v], bs[v]
        C = np.zeros((dv, dv), LD)
        for a in range(cs[0][k], cs[1][k]):
            C[cI[a] - d0, cJ[a] - d0] += cV[a]
            if cI[a] != cJ[a]: C[cJ[a] - d0, cI[a] - d0] += cV[a]
        C[np.arange(dv), np.arange(dv)] += LD(lam)
        cols = np.unique(rpos[pr[starts[0][k]:starts[1][k]]])
        E = np.zeros((cols.size, dv), LD)                                 # rows: the block's reduced neighbours' dof
        ci = np.searchsorted(cols, rpos[pr[starts[0][k]:starts[1][k]]])
        np.add.at(E, (ci, pe[starts[0][k]:starts[1][k]] - d0), ve[starts[0][k]:starts[1][k]])
        W = _ld_ldlt_solve(C, np.concatenate([E.T, -g[d0:d0 + dv][:, None]], axis=1))     # C^-1 [E' | -g_v]
        S[np.ix_(cols, cols)] -= E @ W[:, :-1]
        s[cols] -= E @ W[:, -1]
        sol[v] = (cols, W)
    xr = _ld_ldlt_solve(S, s)[:, 0]
    x = np.zeros(ndof, LD); x[red] = xr
    for v, (cols, W) in sol.items():
        d0, dv = bo0[v], bs[v]
        x[d0:d0 + dv] = W[:, -1] - W[:, :-1] @ xr[cols]
    return x, S.astype(np.float64)


# ---- the same problem with its variables listed in another order (tests/test_variable_order.py, tests/test_gpu_variable_order.py) ---------------------
# Every generator lists the variables of the reduced system (cameras, poses, the adaptive kernel variable) before the eliminated ones (points).  The C ABI
# takes any order and the reference does not care (its LDL' orders itself); the device code does: a coupling block lies in the block row of whichever of its
# two variables comes LATER, so an eliminated variable listed before a reduced neighbour finds its block in the neighbour's row, stored transposed.
def permute_variables(problem, perm):
    """(new_problem, new_of_old): the variables of `problem` -- kind, size and stored values -- listed in the order `perm` (perm[new] = old, 0-based); every cost
    group with its block order, data and robust kernel, its varind re-indexed (the slot order inside a block is the residual kind's and stays).
    new_of_old[old] = new, 0-based."""
    from nllssolver_jl_amd import NLLSProblem
    perm = np.asarray(perm, np.int64); n = problem.nvariables
    assert perm.shape == (n,) and np.array_equal(np.sort(perm), np.arange(n)), "perm is not a permutation of the variables"
    new_of_old = np.empty(n, np.int64); new_of_old[perm] = np.arange(n)
    off = problem.var_offsets; v = problem.variables; kk, dd = problem.var_kind, problem.var_dim
    q = NLLSProblem()
    for old in perm:
        q.addvariable(v[off[old]:off[old + 1]], int(kk[old]))
    assert np.array_equal(q.var_kind, kk[perm]) and np.array_equal(q.var_dim, dd[perm])
    for g in problem.costs.values():
        vi, da = g.arrays()
        q.addcosts(g.res_kind, new_of_old[vi - 1] + 1, da.copy(), g.robust)
    assert list(q.costs.keys()) == list(problem.costs.keys())
    return q, new_of_old


def to_original_order(vec, sizes, new_of_old):
    """A packed vector of the PERMUTED problem (one segment per variable, in the new order) in the ORIGINAL order.  sizes[old] = length of the variable's
    segment: its storage for a variable vector, its unknowns (0 if fixed) for a step or a gradient."""
    sizes = np.asarray(sizes, np.int64); new_of_old = np.asarray(new_of_old, np.int64); n = sizes.size
    sizes_new = np.empty(n, np.int64); sizes_new[new_of_old] = sizes
    off_new = np.concatenate([[0], np.cumsum(sizes_new)])
    vec = np.asarray(vec); assert vec.size == off_new[-1], (vec.size, off_new[-1])
    start = off_new[new_of_old]                                              # per old variable: where its segment starts in the permuted vector
    idx = np.repeat(start, sizes) + (np.arange(sizes.sum()) - np.repeat(np.cumsum(sizes) - sizes, sizes))
    return vec[idx]


def variable_sizes(problem, unfixed=None):
    """(storage, unknowns) per variable of `problem`; unknowns 0 for the variables `unfixed` marks False."""
    from nllssolver_jl_amd import kinds as K
    st = np.diff(problem.var_offsets)
    dof = np.array([K.var_dof(int(k), int(d)) for k, d in zip(problem.var_kind, problem.var_dim)], np.int64)
    if unfixed is not None: dof = dof * np.asarray(unfixed, bool)
    return st, dof


def eliminated_mask(problem):
    """The variables of a bundle-adjustment problem of the generators that the elimination takes: the 3-dof Euclidean points."""
    from nllssolver_jl_amd import kinds as K
    return (problem.var_kind == K.VAR_EUCLIDEAN) & (problem.var_dim == 3)


# named orders (perm[new] = old).  `elim`: boolean per variable, the eliminated ones.
def order_identity(elim):
    return np.arange(len(elim))                                              # the control


def order_elim_first(elim):
    elim = np.asarray(elim, bool); return np.r_[np.nonzero(elim)[0], np.nonzero(~elim)[0]]     # all points, then the cameras: every neighbour block transposed


def order_reversed(elim):
    return np.arange(len(elim))[::-1].copy()


def order_interleaved(elim):
    """reduced variable k followed by the k-th share of the eliminated ones: a point's neighbours lie on both sides of it (lists that mix both `trans` values)"""
    elim = np.asarray(elim, bool); red = np.nonzero(~elim)[0]; shares = np.array_split(np.nonzero(elim)[0], max(red.size, 1))
    return np.concatenate([np.r_[r, s] for r, s in zip(red, shares)]).astype(np.int64)


def order_random(seed):
    return lambda elim: np.random.default_rng(seed).permutation(len(elim))


def order_var_last(var=0):
    """variable `var` (the adaptive kernel variable: index 0 in every generator) moved behind all others"""
    return lambda elim: np.r_[np.delete(np.arange(len(elim)), var), var]


def order_var_middle(var=0):
    def f(elim):
        rest = np.delete(np.arange(len(elim)), var); return np.r_[rest[:rest.size // 2], var, rest[rest.size // 2:]]
    return f


NAMED_ORDERS = dict(identity=order_identity, elim_first=order_elim_first, reversed=order_reversed, interleaved=order_interleaved, random=order_random(7))


# ---- two-slot problems of a chosen elimination structure (the matrix-free LM trial's kernel shapes: tests/test_gpu_mf_shapes.py) -------------------
def structured_problem(kind, runs, nred, ps=1, seed=0, noise=1e-3):
    """A problem of ONE cost group of a two-slot kind whose eliminated set and supernodes the caller chooses.  The `nred` reduced variables come first,
    the eliminated ones after them; runs = [(ncb, nmem), ...]: nmem eliminated variables in a row that share one window of ncb consecutive reduced
    variables (one cost block each), windows of neighbouring runs different -- so a run is a supernode (cut at 128 members).
      kind RES_BA_AFFINE: cameras (6 dof) reduced, points (3 dof) eliminated, slot 1 (ps must be 1); measurements at the truth, then the variables
        perturbed as perturb_ba_problem does.
      kind RES_ROSENBROCK_B: b (x^2 - y), every variable one dof; ps = 1: the eliminated variable is y, ps = 0: it is x.  All blocks are of one size,
        so the greedy independent set (lowest degree first) must find every reduced variable of higher degree than every eliminated one: runs of
        one-block members are appended to lift every reduced variable above the widest window.
    Returns (problem, meta): meta["elim_blocks"] (bool per block), meta["supernodes"] (the count the grouping gives), meta["windows"] (per eliminated
    variable: its reduced neighbours, 0-based)."""
    from nllssolver_jl_amd import NLLSProblem, kinds as K
    rng = np.random.default_rng(seed)
    windows, R = [], len(runs)
    for r, (ncb, nmem) in enumerate(runs):
        assert 1 <= ncb <= nred
        span = nred - ncb + 1; start = int(round(r * (span - 1) / max(R - 1, 1)))          # (the windows spread over the reduced variables)
        if windows and windows[-1][0] == start and len(windows[-1]) == ncb: start = (start + 1) % span
        windows += [tuple(range(start, start + ncb))] * nmem
    cover = np.zeros(nred, np.int64)
    for w in windows: cover[list(w)] += 1
    for j in range(nred):                   # a reduced variable no window reaches: one more member of the first run's width there
        if cover[j] == 0:
            ncb = runs[0][0]; start = min(j, nred - ncb); windows.append(tuple(range(start, start + ncb))); cover[start:start + ncb] += 1
    if kind == K.RES_ROSENBROCK_B:
        top = max(len(w) for w in windows)
        for j in np.nonzero(cover <= top)[0]:
            windows += [(int(j),)] * int(top + 1 - cover[j])
    else:
        assert kind == K.RES_BA_AFFINE and ps == 1
    nelim = len(windows)
    assert nelim * 2 >= nred + nelim, "the eliminated variables must be at least half of all blocks"
    p = NLLSProblem()
    if kind == K.RES_BA_AFFINE:
        cams = rng.standard_normal((nred, 6)) + np.array([1.0, 0, 0, 0, 1.0, 0])
        pts = rng.random((nelim, 3)) + np.array([-0.5, -0.5, 10.0])
        p.addvariables(cams); p.addvariables(pts)
        cam = np.concatenate([np.asarray(w) for w in windows]); pt = np.repeat(np.arange(nelim), [len(w) for w in windows])
        c, X = cams[cam], pts[pt]
        meas = np.stack([(c[:, 0:3] * X).sum(1), (c[:, 3:6] * X).sum(1)], axis=1)
        p.addcosts(K.RES_BA_AFFINE, np.stack([cam + 1, pt + nred + 1], axis=1), meas)
        from nllssolver_jl_amd import synthetic
        synthetic.perturb_ba_problem(p, noise, noise, seed=seed + 1)
    else:
        p.addvariables(rng.uniform(0.5, 1.5, (nred + nelim, 1)))
        red = np.concatenate([np.asarray(w) for w in windows]) + 1; el = np.repeat(np.arange(nelim), [len(w) for w in windows]) + nred + 1
        vi = np.stack([el, red] if ps == 0 else [red, el], axis=1)
        p.addcosts(K.RES_ROSENBROCK_B, vi, rng.uniform(0.5, 2.0, (len(vi), 1)))
    sn, prev, glen = 0, None, 0
    for w in windows:
        if w != prev or glen == 128: sn += 1; glen = 0
        prev = w; glen += 1
    return p, dict(elim_blocks=np.r_[np.zeros(nred, bool), np.ones(nelim, bool)], supernodes=sn, windows=windows, nred=nred)


def check_structure(ols, meta):
    """The generated structure as the oracle's linear system stores it (bsm_index, 1-based): every eliminated block row holds exactly its window and
    its diagonal block, no reduced block couples to another, and the eliminated set is what the greedy independent set (lowest degree first inside the
    most numerous block size) picks."""
    cp, rv, _, bo = (np.asarray(a, np.int64) for a in ols.bsm_index())
    nb = len(cp) - 1; nred = meta["nred"]; elim = meta["elim_blocks"]
    assert ols.info.is_sparse and nb == elim.size
    deg = np.zeros(nb, np.int64)
    for row in range(nb):
        cols = rv[cp[row] - 1:cp[row + 1] - 1] - 1
        if elim[row]: assert sorted(cols) == sorted(list(meta["windows"][row - nred]) + [row]), row
        else: assert list(cols) == [row], row
        off = cols[cols != row]; deg[row] += off.size; np.add.at(deg, off, 1)
    bs = np.diff(np.r_[bo - 1, ols.info.ndof])
    sizes, counts = np.unique(bs, return_counts=True); best = sizes[np.argmax(counts)]
    assert np.all(bs[elim] == best) and 2 * elim.sum() >= nb
    if np.all(bs == best): assert deg[~elim].min() > deg[elim].max(), "a reduced block would be eliminated first"
