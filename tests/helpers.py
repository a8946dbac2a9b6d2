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
def structured_problem(kind, runs, nred, ps=1, seed=0, noise=1e-3, border=0, windows=None):
    """A problem of ONE cost group of a two-slot kind whose eliminated set and supernodes the caller chooses.  The `nred` reduced variables come first,
    the eliminated ones after them; runs = [(ncb, nmem), ...]: nmem eliminated variables in a row that share one window of ncb consecutive reduced
    variables (one cost block each), windows of neighbouring runs different -- so a run is a supernode (cut at 128 members).
      kind RES_BA_AFFINE: cameras (6 dof) reduced, points (3 dof) eliminated, slot 1 (ps must be 1); measurements at the truth, then the variables
        perturbed as perturb_ba_problem does.
      kind RES_ROSENBROCK_B: b (x^2 - y), every variable one dof; ps = 1: the eliminated variable is y, ps = 0: it is x.  All blocks are of one size,
        so the greedy independent set (lowest degree first) must find every reduced variable of higher degree than every eliminated one: runs of
        one-block members are appended to lift every reduced variable above the widest window.  border (this kind only): the last `border` of the nred
        reduced variables are no part of the band -- the windows are laid over the first nred - border -- and EVERY eliminated variable has one more
        cost block on each of them: coupled to all eliminated blocks, they are what the upload orders behind the band as border rows (15 dof at most).
      windows (optional; `runs` is then not read): one tuple of 0-based reduced variables (of the first nred - border) per eliminated variable, in place of the
        windows laid out from runs -- any reduced graph (a tree, an expander, several components: tests/test_gpu_tsp_shapes.py); every reduced variable must lie
        in one.  What follows the layout -- the degree lifting, the border, meta, the perturbation -- is the same.
    Returns (problem, meta): meta["elim_blocks"] (bool per block), meta["supernodes"] (the count the grouping gives), meta["windows"] (per eliminated
    variable: its reduced neighbours, 0-based)."""
    from nllssolver_jl_amd import NLLSProblem, kinds as K
    rng = np.random.default_rng(seed)
    assert border == 0 or kind == K.RES_ROSENBROCK_B
    given, nred_all = windows, nred
    windows, R = [], (0 if given is not None else len(runs))
    nred = nred_all - border                # (the band's variables: what the windows are laid over)
    if given is not None:
        windows = [tuple(int(j) for j in w) for w in given]
        assert all(len(w) >= 1 and len(set(w)) == len(w) and 0 <= min(w) and max(w) < nred for w in windows), "a window outside the reduced variables, or one listed twice"
        assert np.unique(np.concatenate([np.asarray(w) for w in windows])).size == nred, "a reduced variable in no window"
    for r, (ncb, nmem) in enumerate(runs if given is None else []):
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
        top = max(len(w) for w in windows) + border
        for j in np.nonzero(cover <= top)[0]:
            windows += [(int(j),)] * int(top + 1 - cover[j])
        windows = [w + tuple(range(nred, nred_all)) for w in windows]
    else:
        assert kind == K.RES_BA_AFFINE and ps == 1
    nred = nred_all
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


# ---- graphs that are not bundle adjustment (tests/test_general_graphs.py, tests/test_gpu_general_graphs.py) ------------------------------------------
# Every sparse problem of the generators is bipartite with the eliminated variable in one fixed slot of one kind.  The symbolic phase takes any graph of cost
# blocks: the problems below have cost blocks between two REDUCED variables (copied into S, Schur updates on top), the eliminated variable in slot 0 of some
# blocks and slot 1 of others, four-slot kinds, unary groups beside the coupling group, several block sizes in the reduced system, eliminated classes other than
# the 3-dof points, and independent sets too small for a Schur complement.
def expected_elimination(ols):
    """The blocks select_elimination (csrc/nlls_structure.cpp) takes, from the oracle's block structure (ols.bsm_index()): the candidates are the blocks of the most
    numerous size (ties: the smaller size) whose neighbours fit the LDS-staged kernels; by ascending degree (stable: ties in block order) a candidate is taken unless
    a block it shares a stored block with was taken before; the set is kept only if it holds at least half of all blocks.  A boolean per block."""
    cp, rv, _, bo = (np.asarray(a, np.int64) for a in ols.bsm_index()); nb = len(cp) - 1
    elim = np.zeros(nb, bool)
    if not ols.info.is_sparse or nb <= 1: return elim
    bs = np.diff(np.r_[bo - 1, ols.info.ndof]); rows = np.repeat(np.arange(nb), np.diff(cp)); cols = rv - 1
    off = rows != cols
    deg = np.bincount(rows[off], minlength=nb) + np.bincount(cols[off], minlength=nb)
    nbrs = [[] for _ in range(nb)]
    for r, c in zip(rows[off], cols[off]): nbrs[r].append(c); nbrs[c].append(r)
    sizes, counts = np.unique(bs, return_counts=True); best = int(sizes[np.argmax(counts)])          # (np.unique sorts ascending, argmax takes the first: ties to the smaller)
    fits = lambda v: 8 * (best * best + best * (2 * sum(bs[u] for u in nbrs[v]) + 1)) + 28 * sum(bs[u] for u in nbrs[v]) + 16 <= 150 * 1024
    cand = [v for v in range(nb) if bs[v] == best and fits(v)]
    blocked = np.zeros(nb, bool)
    for v in sorted(cand, key=lambda v: deg[v]):                                                    # (sorted is stable)
        if blocked[v]: continue
        elim[v] = True; blocked[v] = True; blocked[nbrs[v]] = True
    if 2 * elim.sum() < nb: elim[:] = False
    return elim


def block_mask_to_variables(block_mask, bi):
    """a boolean per variable from a boolean per block (bi: blockindices, 0 = fixed -> False)"""
    bi = np.asarray(bi, np.int64); out = np.zeros(bi.size, bool); out[bi > 0] = np.asarray(block_mask, bool)[bi[bi > 0] - 1]; return out


def structure_counts(problem, ols, elim_blocks, bi=None):
    """What a case of the general-graph tests is written for, from the oracle's structure and the mirror's set: `independent` (no stored block joins two eliminated
    blocks), `reduced_reduced` (stored off-diagonal blocks between two reduced blocks), `mixed_slots` (eliminated variables seen in more than one slot of ONE cost
    group), `elim_slots` (the slots eliminated variables are seen in, over all groups of two or more slots), `elim_unary` (unary cost blocks on eliminated variables),
    `reduced_sizes` / `elim_sizes` (block sizes)."""
    cp, rv, _, bo = (np.asarray(a, np.int64) for a in ols.bsm_index()); nb = len(cp) - 1; elim = np.asarray(elim_blocks, bool)
    bs = np.diff(np.r_[bo - 1, ols.info.ndof]); rows = np.repeat(np.arange(nb), np.diff(cp)); cols = rv - 1; off = rows != cols
    bi = blockindices(problem) if bi is None else bi
    ev = block_mask_to_variables(elim, bi)
    mixed, slots, unary = 0, set(), 0
    for g in problem.costs.values():
        vi, _ = g.arrays()
        if vi.shape[1] == 1: unary += int(ev[vi[:, 0] - 1].sum()); continue
        seen = np.zeros((problem.nvariables, vi.shape[1]), bool)
        for s in range(vi.shape[1]): seen[vi[:, s] - 1, s] = True
        mixed += int((seen[ev].sum(axis=1) > 1).sum()); slots |= set(np.nonzero(seen[ev].any(axis=0))[0].tolist())
    return dict(independent=not np.any(off & elim[rows] & elim[cols]), reduced_reduced=int((off & ~elim[rows] & ~elim[cols]).sum()), mixed_slots=mixed,
                elim_slots=sorted(slots), elim_unary=unary, reduced_sizes=sorted(set(bs[~elim].tolist())), elim_sizes=sorted(set(bs[elim].tolist())),
                nelim=int(elim.sum()), nreduced_dof=int(bs[~elim].sum()))


def greedy_independent_set(n, edges):
    """expected_elimination on a graph of n one-dof variables given as an edge list (0-based pairs; repeated edges count once): what scalar_graph_problem needs to know
    BEFORE it builds the problem, to keep the eliminated variables in one slot when mix_slots is off."""
    e = np.unique(np.sort(np.asarray(edges, np.int64).reshape(-1, 2), axis=1), axis=0)
    deg = np.bincount(e.ravel(), minlength=n); nbrs = [[] for _ in range(n)]
    for a, b in e: nbrs[a].append(b); nbrs[b].append(a)
    elim = np.zeros(n, bool); blocked = np.zeros(n, bool)
    for v in sorted(range(n), key=lambda v: deg[v]):
        if blocked[v]: continue
        elim[v] = True; blocked[v] = True; blocked[nbrs[v]] = True
    if 2 * elim.sum() < n: elim[:] = False
    return elim


def scalar_graph_problem(edges, n, seed, mix_slots=True, unary=True, robust=None):
    """n one-dof variables in U(0.5, 1.5); one RES_ROSENBROCK_B block b (x^2 - y), b in U(0.5, 2), per entry of `edges` (0-based pairs, repeats allowed: several cost
    blocks on one stored block) under `robust`; unary: one RES_ROSENBROCK_A block on every variable (a second group, on eliminated and reduced variables alike).
    mix_slots: every edge's orientation -- which end is x -- is drawn with probability 1/2, so a variable is x in some of its blocks and y in others; off: an end the
    greedy independent set takes is always x (slot 0), edges between two reduced variables stay as listed."""
    from nllssolver_jl_amd import NLLSProblem, kinds as K
    rng = np.random.default_rng(seed); e = np.asarray(edges, np.int64).reshape(-1, 2).copy()
    assert e.min() >= 0 and e.max() < n and np.all(e[:, 0] != e[:, 1])
    p = NLLSProblem(); p.addvariables(rng.uniform(0.5, 1.5, (n, 1)))
    flip = rng.random(len(e)) < 0.5                                                                 # (drawn either way: the other numbers do not depend on mix_slots)
    if not mix_slots: flip = greedy_independent_set(n, e)[e[:, 1]]
    e[flip] = e[flip][:, ::-1]
    p.addcosts(K.RES_ROSENBROCK_B, e + 1, rng.uniform(0.5, 2.0, (len(e), 1)), robust)
    if unary: p.addcosts(K.RES_ROSENBROCK_A, np.arange(1, n + 1)[:, None], rng.uniform(0.5, 1.5, (n, 1)))
    return p


# edge-list builders: (edges, n).  The size parameter puts the reduced system under the 64 dof of the one-wavefront solve or over the 128 of the band solvers.
def chain_edges(n):
    """a path: the ends (degree 1), then every other variable: n / 2 eliminated, each with two reduced neighbours; one reduced-reduced block for even n"""
    return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1), n


def lattice_edges(w, h, diagonal=False):
    """a w x h grid, row-major; diagonal: with one diagonal per cell (a triangular lattice).  Its greedy independent set stays under half of the variables."""
    idx = np.arange(w * h).reshape(h, w)
    e = [np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], axis=1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], axis=1)]
    if diagonal: e.append(np.stack([idx[:-1, :-1].ravel(), idx[1:, 1:].ravel()], axis=1))
    return np.concatenate(e), w * h


def caterpillar_edges(nhubs, nleaves=4):
    """hubs 0 .. nhubs-1, hub k coupled to k+1 and k+2 (2 nhubs - 3 reduced-reduced blocks, a band of two); nleaves leaves (degree 1: eliminated) on every hub, listed
    after the hubs"""
    hubs = np.arange(nhubs)
    e = [np.stack([hubs[:-1], hubs[1:]], axis=1), np.stack([hubs[:-2], hubs[2:]], axis=1)]
    e.append(np.stack([np.repeat(hubs, nleaves), nhubs + np.arange(nhubs * nleaves)], axis=1))
    return np.concatenate(e), nhubs * (1 + nleaves)


def shared_leaves_edges(nhubs, nleaves, heavy=0):
    """hubs in a chain (nhubs - 1 reduced-reduced blocks); every leaf on three consecutive hubs (degree 3, eliminated: the Schur update of a leaf lands on the two
    chain blocks inside its window and fills the block between its outer hubs).  heavy: leaf 0's three edges are listed that many times more (one variable with
    3 (heavy + 1) coupling blocks on three stored blocks)."""
    hubs = np.arange(nhubs); start = (np.arange(nleaves) * (nhubs - 2)) // nleaves
    leaf = nhubs + np.arange(nleaves)
    e = [np.stack([hubs[:-1], hubs[1:]], axis=1)] + [np.stack([start + k, leaf], axis=1) for k in range(3)]
    e += [np.stack([start[:1] + k, leaf[:1]], axis=1) for _ in range(heavy) for k in range(3)]
    return np.concatenate(e), nhubs + nleaves


def hub_edges(n, pendants=0):
    """a chain of n (odd) variables, `pendants` more variables hung on its odd members (which the chain's elimination leaves in the reduced system), and one last variable
    coupled to every other: with 64 or more eliminated variables it couples to more than a quarter of them and becomes a border block of the reduced system."""
    assert n % 2 == 1
    e = [chain_edges(n)[0]]
    odd = np.arange(1, n, 2)
    if pendants: e.append(np.stack([odd[np.arange(pendants) % odd.size], n + np.arange(pendants)], axis=1))
    hub = n + pendants
    e.append(np.stack([np.arange(hub), np.full(hub, hub)], axis=1))
    return np.concatenate(e), hub + 1


def curve_family_problem(ncurves, npoints, own, seed=0, noise=1e-3):
    """a exp(b t) + c t + d - y (RES_CURVE_EXP4, four one-dof slots) over ncurves curves of npoints samples each.  own: the slots (0 .. 3) whose parameter every curve
    has for itself; the others are shared by all curves.  own = (0,) or (3,): the curves' own parameters (degree 3) are eliminated, each coupled to the three shared
    scalars by npoints cost blocks, the same blocks that couple the three reduced scalars to one another.  own = (0, 1): a curve's two parameters share a stored
    block, the independent set holds one of them -- under half of all blocks, no Schur complement."""
    from nllssolver_jl_amd import NLLSProblem, kinds as K
    rng = np.random.default_rng(seed); own = tuple(own); truth = np.array([2.0, -1.5, 0.7, 0.3]); start = np.array([1.5, -1.0, 0.0, 0.0])
    p = NLLSProblem(); par = np.tile(truth, (ncurves, 1)); slotvar = np.zeros((ncurves, 4), np.int64)
    for s in range(4):
        if s in own:
            par[:, s] = truth[s] * rng.uniform(0.8, 1.2, ncurves)
            slotvar[:, s] = p.addvariables((start[s] + rng.uniform(-0.1, 0.1, ncurves))[:, None]) + np.arange(ncurves)
        else:
            slotvar[:, s] = p.addvariable(start[s])
    t = rng.random((ncurves, npoints)) * 2.0
    y = par[:, 0:1] * np.exp(par[:, 1:2] * t) + par[:, 2:3] * t + par[:, 3:4] + rng.standard_normal(t.shape) * noise
    p.addcosts(K.RES_CURVE_EXP4, np.repeat(slotvar, npoints, axis=0), np.stack([t.ravel(), y.ravel()], axis=1))
    return p


def mixed_sizes_problem(extra="linear3", seed=3):
    """Affine bundle adjustment 12 x 150 at 0.3 under a Huber kernel (6-dof cameras, 3-dof points: the eliminated class) with, beside it,
      extra = "linear3": X w - y (RES_LINEAR3, unary) on every third point, and a chain of 40 scalars (RES_ROSENBROCK_B with both orientations, RES_ROSENBROCK_A on each):
        a second component of one-dof blocks that all stay in the reduced system, next to the 6-dof cameras;
      extra = "cost3": the same with the non-squared cost y'w (COST_LINEAR3) on those points;
      extra = "adaptive_mean": instead an RES_ADAPTIVE_MEAN component -- one ContaminatedGaussian variable (3 dof: the points' size class, not Euclidean, of degree 2: a
        candidate the greedy set reaches early) and two means, 60 blocks."""
    import nllssolver_jl_amd as N
    from nllssolver_jl_amd import synthetic, kinds as K
    from nllssolver_jl_amd.variables import contaminated_gaussian
    ncam, npts = 12, 150; rng = np.random.default_rng(seed)
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(ncam, npts, 0.3, seed=seed, robust=N.HuberKernel(0.05), outlier_frac=0.1, outlier_sigma=0.05), 1e-3, 1e-3)
    if extra in ("linear3", "cost3"):
        pts = np.arange(0, npts, 3); w = p.variables.reshape(-1)[6 * ncam:].reshape(npts, 3)[pts]
        if extra == "linear3":
            X = rng.standard_normal((pts.size, 3, 3)) + 2.0 * np.eye(3); y = np.einsum("nij,nj->ni", X, w) + 0.01 * rng.standard_normal((pts.size, 3))
            p.addcosts(K.RES_LINEAR3, (ncam + pts + 1)[:, None], np.concatenate([y, X.transpose(0, 2, 1).reshape(pts.size, 9)], axis=1))      # (y, X column-major)
        else:
            p.addcosts(K.COST_LINEAR3, (ncam + pts + 1)[:, None], 0.01 * rng.standard_normal((pts.size, 3)))
        n0 = p.nvariables; e, n = chain_edges(40)
        p.addvariables(rng.uniform(0.5, 1.5, (n, 1)))
        e = e.copy(); flip = rng.random(len(e)) < 0.5; e[flip] = e[flip][:, ::-1]
        p.addcosts(K.RES_ROSENBROCK_B, e + n0 + 1, rng.uniform(0.5, 2.0, (len(e), 1)))
        p.addcosts(K.RES_ROSENBROCK_A, (np.arange(n) + n0 + 1)[:, None], rng.uniform(0.5, 1.5, (n, 1)))
    else:
        assert extra == "adaptive_mean"
        k = p.addvariable(contaminated_gaussian(0.5, 5.0, 0.6), K.VAR_CONTAMINATED_GAUSSIAN); m1 = p.addvariable(-0.7); m2 = p.addvariable(0.6)
        draws = np.concatenate([rng.standard_normal(24), rng.standard_normal(6) * 10.0])
        vi = np.empty((60, 2), np.int64); vi[:, 0] = k; vi[0::2, 1] = m1; vi[1::2, 1] = m2
        da = np.empty((60, 1)); da[0::2, 0] = draws - 1; da[1::2, 0] = draws + 1
        p.addcosts(K.RES_ADAPTIVE_MEAN, vi, da)
    return p


def many_cameras_problem(so3, seed=4):
    """120 cameras over 30 points at 0.15: the 6-dof class is the most numerous and independent -- the CAMERAS (affine, or SO(3) poses: storage 12, a retraction that is
    not an addition) are eliminated, the points form the reduced system."""
    import nllssolver_jl_amd as N
    from nllssolver_jl_amd import synthetic
    if so3: p = synthetic.create_so3_ba_problem(120, 30, 0.15, seed=seed, adaptive=False, robust=N.HuberKernel(0.05))
    else: p = synthetic.create_ba_problem(120, 30, 0.15, seed=seed, robust=N.HuberKernel(0.05), outlier_frac=0.1, outlier_sigma=0.05)
    return synthetic.perturb_ba_problem(p, 1e-3, 1e-3)
