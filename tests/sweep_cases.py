"""The accumulate and cost sweeps (csrc/nlls_sweep.hip, csrc/nlls_cost.hip) at the edges where their launches switch form -- problems, an INTEGER reference and the
tile builder restated.  A plain module: tests/test_sweep_cases.py (CPU) and tests/test_gpu_sweep_exact.py (GPU) run the cases below.

The problems are affine bundle adjustment (RES_BA_AFFINE, no robust kernel) on a dyadic grid, as tests/test_gpu_mfb_pack.dyadic_ba_problem (notes/r16.md): truth on
multiples of 1/16, perturbations on multiples of 1/256, measurements from the unperturbed truth.  The residual is bilinear, r = (c[0:3].X - m0, c[3:6].X - m1), so with
the variables scaled by 2^8 everything the sweep forms is an integer: r 2^16, J'J 2^16, J'r 2^24, the cost r'r / 2 2^33.  exact_system() forms them in int64 and asserts,
entry by entry, that the sum of the ABSOLUTE terms stays below 2^53: every partial sum in any order is then exact in float64, and A.data, b and the cost are the same BITS
whatever the order of the atomics, the accumulator copies or the reduction trees.  The comparison needs no tolerance and sees one dropped, doubled or misplaced term.

expected_tiles() / expected_fold() restate build_structure's tile loop and build_fold (csrc/nlls_structure.cpp) and what launch_gh (csrc/nlls_sweep.hip) decides from
them.  Every case states the edge it exists for as a predicate on that restatement; the GPU test holds the six counters of nlls_get_solve_stats()[37..42] against it."""
import functools

import numpy as np

from nllssolver_jl_amd import kinds as K
from tests.helpers import blockindices, permute_variables, NAMED_ORDERS

BA = K.RES_BA_AFFINE
# csrc/nlls_structure.cpp, csrc/nlls_ctx.hpp, csrc/nlls_sweep.hip
LIGHT_MAX_ENTRIES, LIGHT_IMG_MAX, HEAVY_ROW_ENTRIES, ACC_COPIES = 256, 6144, 128, 4
TILE_PARTIAL, TILE_DIRECT, TILE_NOZERO = 1, 2, 4
DEST_NONE, OWN_COST_OWNER = 0xFFFFFFFF, 1 << 16
FOLD_SLOT_NONE, FOLD_MAX_CW, FOLD_ROW_COPIES, GCONS = 0x3F, 128, 2, 4096
TPB, HTPB, HROWS, HCHUNK, TINY_DENSE_MAX_WGS = 256, 128, 2, 14, 256
FLAG_FORCE_ATOMIC = 1
DOF = (6, 3)                                   # slot 0: the camera, slot 1: the point
COUNTERS = ("sweep_light_tiles", "sweep_image_tiles", "sweep_direct_tiles", "sweep_partial_tiles", "sweep_fold_groups", "sweep_fused_groups")


# ---- the problems ---------------------------------------------------------------------------------------------------------------------------------
class SweepProblem:
    """What crosses the C ABI (var_kind, var_dim, bi, groups) with two variable sets on the grid; cameras and points in the caller's numbering map to the variables
    cam_var[c], pt_var[p] (0-based, in the uploaded order)."""

    def oracle(self):
        if getattr(self, "_oracle", None) is None:
            from oracle import oracle as O
            op = O.OracleProblem(self.var_kind, self.var_dim, self.groups); op.set_variables(self.variables)
            self._oracle = (op, op.linear_system(self.bi))
        return self._oracle


def dyadic_ba(incidences, order="identity", fixed=None, ngroups=1, seed=5, group_of=None):
    """incidences: (camera, point) pairs, 0-based; a repeated pair is a second observation.  order: a name of tests.helpers.NAMED_ORDERS or a permutation (perm[new] =
    old) of the variables [cameras, points].  fixed: boolean per variable in THAT numbering (cameras, then points).  ngroups: the costs are dealt over that many
    RES_BA_AFFINE groups on the same variables (cost k to group k % ngroups, or group_of[k])."""
    from nllssolver_jl_amd import NLLSProblem
    inc = np.asarray(incidences, np.int64).reshape(-1, 2); cam, pt = inc[:, 0], inc[:, 1]
    ncam, npts = int(cam.max()) + 1, int(pt.max()) + 1; n = ncam + npts
    rng = np.random.default_rng(seed)
    cams = np.round(16 * (rng.standard_normal((ncam, 6)).clip(-3, 3) + np.array([1.0, 0, 0, 0, 1.0, 0]))) / 16
    pts = np.round(16 * (rng.random((npts, 3)) + np.array([-0.5, -0.5, 10.0]))) / 16
    c, X = cams[cam], pts[pt]
    meas = np.stack([(c[:, 0:3] * X).sum(1), (c[:, 3:6] * X).sum(1)], axis=1)                   # exact: multiples of 2^-8 below 2^7
    truth = np.concatenate([cams.ravel(), pts.ravel()])
    v1 = truth + rng.integers(-3, 4, truth.shape) / 256
    v1[v1 == 0.0] = 1 / 256                                                                       # (no exact zero: a product with it would carry a sign the sums do not)
    rng2 = np.random.default_rng(seed + 1000)
    v2 = truth + rng2.integers(1, 4, truth.shape) * rng2.choice([-1, 1], truth.shape) / 256       # every value moved: truth is a multiple of 16/256, so none is zero
    assert np.all(v2 != truth) and np.all(v2 != 0.0) and np.all(v1 != 0.0)
    p = NLLSProblem(); p.addvariables(v1[:6 * ncam].reshape(ncam, 6)); p.addvariables(v1[6 * ncam:].reshape(npts, 3))
    p.addcosts(BA, np.stack([cam + 1, pt + ncam + 1], axis=1), meas)
    elim = np.r_[np.zeros(ncam, bool), np.ones(npts, bool)]
    perm = NAMED_ORDERS[order](elim) if isinstance(order, str) else np.asarray(order, np.int64)
    q, new_of_old = permute_variables(p, perm)
    off_old = p.var_offsets
    sp = SweepProblem()
    sp.problem = q; sp.var_kind, sp.var_dim, sp.off = q.var_kind, q.var_dim, q.var_offsets
    sp.variables = q.variables.copy()
    sp.variables2 = np.concatenate([v2[off_old[o]:off_old[o + 1]] for o in perm])
    assert np.array_equal(sp.variables, np.concatenate([v1[off_old[o]:off_old[o + 1]] for o in perm]))
    fixed = np.zeros(n, bool) if fixed is None else np.asarray(fixed, bool); assert fixed.shape == (n,)
    sp.bi = blockindices(q, ~fixed[perm])
    vi, da = next(iter(q.costs.values())).arrays()
    group_of = np.arange(len(vi)) % ngroups if group_of is None else np.asarray(group_of, np.int64)
    assert group_of.shape == (len(vi),) and set(np.unique(group_of)) == set(range(ngroups))
    sp.groups = [dict(res_kind=BA, robust_kind=0, robust_params=(0.0, 0.0, 0.0, 0.0), varind=np.ascontiguousarray(vi[group_of == g]), data=np.ascontiguousarray(da[group_of == g]))
                 for g in range(ngroups)]
    sp.ncam, sp.npts, sp.cam_var, sp.pt_var = ncam, npts, new_of_old[:ncam], new_of_old[ncam:]
    return sp


# ---- the integer reference --------------------------------------------------------------------------------------------------------------------------
def _structure(sp, bi):
    """block sizes, offsets and the stored blocks' offsets (0-based) of the linear system: the oracle's bsm_index() where it is block-sparse, the full column-major
    ndof x ndof matrix where it is dense"""
    bi = np.asarray(bi, np.int64); nb = int(bi.max()) if bi.size else 0
    bs = np.zeros(nb, np.int64); bs[bi[bi > 0] - 1] = sp.var_dim[bi > 0]
    boff = np.concatenate([[0], np.cumsum(bs)]); ndof = int(boff[-1])
    _, ols = sp.oracle() if np.array_equal(bi, np.asarray(sp.bi, np.int64)) else (None, oracle_problem_of(sp).linear_system(bi.astype(np.uint64)))
    assert ols.info.ndof == ndof
    st = dict(nb=nb, bs=bs, boff=boff, ndof=ndof, sparse=bool(ols.info.is_sparse), nnz=int(ols.info.nnz_data), ols=ols)
    if st["sparse"]:
        cp, rv, nz, bo = (np.asarray(a, np.int64) for a in ols.bsm_index())
        assert np.array_equal(bo - 1, boff[:-1])
        rows = np.repeat(np.arange(nb), np.diff(cp)); key = rows * nb + (rv - 1)
        assert np.all(np.diff(key) > 0), "the stored blocks are not sorted by (row, column)"
        st.update(cp=cp - 1, rv=rv - 1, nz=nz - 1, key=key, rows=rows, segs=np.r_[(nz - 1)[cp[:-1] - 1], st["nnz"]])
    return st


def oracle_problem_of(sp):
    from oracle import oracle as O
    op = O.OracleProblem(sp.var_kind, sp.var_dim, sp.groups); op.set_variables(sp.variables); return op


def _block_off(st, row, col):
    """offset of block (row, col), row >= col (0-based arrays), and its leading dimension"""
    if not st["sparse"]: return st["boff"][row] + st["ndof"] * st["boff"][col], np.full(len(row), st["ndof"], np.int64)
    k = row * st["nb"] + col; i = np.searchsorted(st["key"], k)
    assert np.all(i < len(st["key"])) and np.all(st["key"][np.minimum(i, len(st["key"]) - 1)] == k), "a block is missing from the pattern"
    return st["nz"][i], st["bs"][row]


def mirror_dense(data, n):
    """the full symmetric matrix from a dense system's lower triangle (column-major A.data), as the device's sweep leaves it (gethessian: symmetrifyfull)"""
    M = np.asarray(data).reshape(n, n).T; M = np.tril(M) + np.tril(M, -1).T; return np.ascontiguousarray(M.T).ravel()


def exact_system(sp, bi=None, variables=None):
    """(A.data, b, cost) of costgradhess! at `variables` in integers: J written out by hand (row 0: [X, 0 | c[0:3]], row 1: [0, X | c[3:6]]), the blocks scattered as
    updatesymlinearsystem! does (src/linearsystem.jl:132-175) through the oracle's bsm_index(); a dense system as the full mirrored matrix.  Asserts the exactness
    condition: per entry the sum of the absolute scaled terms is below 2^53."""
    bi = sp.bi if bi is None else bi; v = sp.variables if variables is None else np.asarray(variables, np.float64)
    st = _structure(sp, bi); bi = np.asarray(bi, np.int64)
    V = np.rint(v * 256).astype(np.int64); assert np.array_equal(V / 256.0, v), "a variable off the 2^-8 grid"
    nA = st["nnz"] if st["sparse"] else st["ndof"] ** 2
    A, Aabs, b, babs = (np.zeros(n, np.int64) for n in (nA, nA, st["ndof"], st["ndof"]))
    cost = 0
    i6, i3 = np.arange(6), np.arange(3)

    def add(row, col, sub, subabs):
        if len(row) == 0: return
        base, ld = _block_off(st, row, col)
        idx = base[:, None, None] + np.arange(sub.shape[1])[None, :, None] + (ld[:, None, None] if np.ndim(ld) else ld) * np.arange(sub.shape[2])[None, None, :]
        np.add.at(A, idx.ravel(), sub.ravel()); np.add.at(Aabs, idx.ravel(), subabs.ravel())

    for g in sp.groups:
        vi = np.asarray(g["varind"], np.int64); n = len(vi)
        if n == 0: continue
        m = np.rint(np.asarray(g["data"]) * 65536).astype(np.int64); assert np.array_equal(m / 65536.0, g["data"]), "a measurement off the 2^-16 grid"
        cv, pv = vi[:, 0] - 1, vi[:, 1] - 1
        c = V[sp.off[cv][:, None] + i6]; X = V[sp.off[pv][:, None] + i3]
        r = np.stack([(c[:, 0:3] * X).sum(1) - m[:, 0], (c[:, 3:6] * X).sum(1) - m[:, 1]], axis=1)                  # x 2^16
        J = np.zeros((n, 2, 9), np.int64); J[:, 0, 0:3] = X; J[:, 1, 3:6] = X; J[:, 0, 6:9] = c[:, 0:3]; J[:, 1, 6:9] = c[:, 3:6]      # x 2^8
        H = np.einsum("nri,nrj->nij", J, J); Habs = np.einsum("nri,nrj->nij", np.abs(J), np.abs(J))                 # x 2^16
        gv = np.einsum("nri,nr->ni", J, r); gabs = np.einsum("nri,nr->ni", np.abs(J), np.abs(r))                    # x 2^24
        cost += int((r * r).sum())                                                                                  # r'r x 2^32 = cost x 2^33
        bc, bp = bi[cv] - 1, bi[pv] - 1; fc, fp = bc >= 0, bp >= 0
        np.add.at(b, st["boff"][bc[fc]][:, None] + i6, gv[fc, 0:6]); np.add.at(babs, st["boff"][bc[fc]][:, None] + i6, gabs[fc, 0:6])
        np.add.at(b, st["boff"][bp[fp]][:, None] + i3, gv[fp, 6:9]); np.add.at(babs, st["boff"][bp[fp]][:, None] + i3, gabs[fp, 6:9])
        add(bc[fc], bc[fc], H[fc, 0:6, 0:6], Habs[fc, 0:6, 0:6]); add(bp[fp], bp[fp], H[fp, 6:9, 6:9], Habs[fp, 6:9, 6:9])
        lo = fc & fp & (bp > bc); hi = fc & fp & (bp < bc)                                                          # the block lies in the row of the LATER variable
        add(bp[lo], bc[lo], H[lo, 6:9, 0:6], Habs[lo, 6:9, 0:6]); add(bc[hi], bp[hi], H[hi, 0:6, 6:9], Habs[hi, 0:6, 6:9])
    lim = 2 ** 53
    assert (Aabs.max() if nA else 0) < lim and (babs.max() if babs.size else 0) < lim and cost < lim, "the sums are not exact in float64: not a case"
    data = A.astype(np.float64) / 65536.0
    if not st["sparse"]: data = mirror_dense(data, st["ndof"])
    return data, b.astype(np.float64) / 2.0 ** 24, cost / 2.0 ** 33


# ---- the tile loop, restated ----------------------------------------------------------------------------------------------------------------------------
def _lists(sp, bi, st):
    """per (group, slot): the incidences sorted by block row (stable in cost order): rows, rowptr, cost"""
    out = {}
    for g, G in enumerate(sp.groups):
        vi = np.asarray(G["varind"], np.int64)
        for s in range(2):
            r = bi[vi[:, s] - 1] - 1; k = np.nonzero(r >= 0)[0]; o = np.argsort(r[k], kind="stable"); cost = k[o]; rr = r[cost]
            rows, cnt = np.unique(rr, return_counts=True)
            out[(g, s)] = dict(rows=rows, rowptr=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), cost=cost, n=len(cost))
    return out


def expected_tiles(sp, bi=None, flags=0, heavy_max=1024, fold_mode=-1):
    """build_structure's `// ---- tiles` section for every group and slot, and what follows from it: lists[(g, s)] = dict(light, heavy: tiles as dicts e0, e1, row0, nrows,
    data_off, data_len, b_off, b_len, flags; unique_dest, compact, own_flags, light_lds, heavy_lds, xdest, owner, rows, rowptr, cost), groups[g] = dict(cost_list, fold,
    fused), counters = the six of nlls_get_solve_stats()[37..42], zero_rows = the block rows zero_ranges_kernel clears.  fold_mode: NLLS_SWEEP_FOLD (-1: the default)."""
    bi = np.asarray(sp.bi if bi is None else bi, np.int64); st = _structure(sp, bi)
    res = dict(lists={}, groups=[], counters=dict.fromkeys(COUNTERS, 0), zero_rows=[], sparse=st["sparse"], st=st)
    if not st["sparse"]: return res
    nb, bs, boff, segs = st["nb"], st["bs"], st["boff"], st["segs"]
    diag_off, _ = _block_off(st, np.arange(nb), np.arange(nb))
    L = _lists(sp, bi, st)
    row_nlists = np.zeros(nb, np.int64)
    for l in L.values(): row_nlists[l["rows"]] += 1
    row_zero = np.zeros(nb, bool); force_atomic = bool(flags & FLAG_FORCE_ATOMIC)
    cnt = res["counters"]
    for g, G in enumerate(sp.groups):
        vi = np.asarray(G["varind"], np.int64)
        for s in range(2):
            l = L[(g, s)]; rows, rowptr, n = l["rows"], l["rowptr"], l["n"]; nrows = len(rows)
            l.update(light=[], heavy=[], unique_dest=True, compact=False, own_flags=0, light_lds=0, heavy_lds=0)
            res["lists"][(g, s)] = l
            if n == 0: continue
            entry_base = np.zeros(n, np.int64); own_row = np.zeros(n, np.int64); tile_of = np.zeros(n, np.int64)

            def close_light(r0, r1, partial):
                br0, br1 = rows[r0], rows[r1 - 1]
                t = dict(e0=int(rowptr[r0]), e1=int(rowptr[r1]), row0=r0, nrows=r1 - r0, data_off=int(segs[br0]), data_len=int(segs[br1 + 1] - segs[br0]),
                         b_off=int(boff[br0]), b_len=int(boff[br1 + 1] - boff[br0]), flags=TILE_PARTIAL if partial else 0)
                for r in range(r0, r1):
                    if partial: row_zero[rows[r]] = True
                    entry_base[rowptr[r]:rowptr[r + 1]] = t["data_off"]; own_row[rowptr[r]:rowptr[r + 1]] = r - r0
                tile_of[t["e0"]:t["e1"]] = len(l["light"])
                dsz = int(bs[br0]); l["light_lds"] = max(l["light_lds"], t["data_len"] + t["b_len"] + t["nrows"] * ACC_COPIES * (dsz * (dsz + 1) // 2 + dsz))
                l["light"].append(t)

            r = 0
            while r < nrows:
                br = rows[r]; ne = int(rowptr[r + 1] - rowptr[r]); seglen = int(segs[br + 1] - segs[br])
                if ne > HEAVY_ROW_ENTRIES or seglen + bs[br] > LIGHT_IMG_MAX:
                    direct = seglen + bs[br] > LIGHT_IMG_MAX; split = ne > heavy_max; shared = row_nlists[br] > 1 or force_atomic
                    for e0 in range(int(rowptr[r]), int(rowptr[r + 1]), heavy_max):
                        t = dict(e0=e0, e1=min(e0 + heavy_max, int(rowptr[r + 1])), row0=r, nrows=1, data_off=int(segs[br]), data_len=0 if direct else seglen, b_off=int(boff[br]),
                                 b_len=int(bs[br]), flags=(TILE_DIRECT if direct else 0) | (TILE_PARTIAL if (split or shared or direct) else 0))
                        tile_of[t["e0"]:t["e1"]] = -1 - len(l["heavy"])
                        l["heavy"].append(t); l["heavy_lds"] = max(l["heavy_lds"], t["data_len"])
                        entry_base[t["e0"]:t["e1"]] = 0 if direct else t["data_off"]
                        if t["flags"] & TILE_PARTIAL: row_zero[br] = True
                    r += 1; continue
                r1, ents, img, partial = r, 0, 0, force_atomic
                while r1 < nrows:
                    brr = rows[r1]; nee = int(rowptr[r1 + 1] - rowptr[r1]); dsz = int(bs[brr])
                    sl = int(segs[brr + 1] - segs[brr]) + dsz + ACC_COPIES * (dsz * (dsz + 1) // 2 + dsz)
                    if r1 > r and brr != rows[r1 - 1] + 1: break
                    if nee > HEAVY_ROW_ENTRIES or sl > LIGHT_IMG_MAX: break
                    if r1 > r and (ents + nee > LIGHT_MAX_ENTRIES or img + sl > LIGHT_IMG_MAX or r1 - r >= 0xFFFF): break
                    sh = row_nlists[brr] > 1
                    if r1 > r and sh != partial and not force_atomic: break
                    partial = sh or force_atomic; ents += nee; img += sl; r1 += 1
                close_light(r, r1, partial); r = r1
            # the other slot's destination and the cost owner, per entry
            k = l["cost"]; t_ = 1 - s; br_e = np.repeat(rows, np.diff(rowptr)); bt = bi[vi[k, t_] - 1] - 1
            has = (bt >= 0) & (bt <= br_e); xdest = np.full(n, DEST_NONE, np.int64)
            if has.any(): xdest[has] = _block_off(st, br_e[has], bt[has])[0] - entry_base[has]
            owner = np.ones(n, bool) if s == 0 else (bi[vi[k, 0] - 1] == 0)                  # first_free: no free variable in an earlier slot
            l.update(xdest=xdest, owner=owner, tile_of=tile_of, own_row=own_row, entry_base=entry_base)
            pairs = np.stack([br_e[xdest != DEST_NONE], xdest[xdest != DEST_NONE]], axis=1)
            l["unique_dest"] = len(np.unique(pairs, axis=0)) == len(pairs)
            if l["unique_dest"]:
                for t in l["light"]:
                    if not t["flags"] & TILE_PARTIAL: t["flags"] |= TILE_NOZERO
            if not l["light"] and l["heavy"] and np.all(owner == owner[0]) and np.all(xdest == DEST_NONE):
                l["compact"] = True; l["own_flags"] = OWN_COST_OWNER if owner[0] else 0
            cnt["sweep_light_tiles"] += len(l["light"]); cnt["sweep_partial_tiles"] += sum(1 for t in l["light"] + l["heavy"] if t["flags"] & TILE_PARTIAL)
            cnt["sweep_direct_tiles"] += sum(1 for t in l["heavy"] if t["flags"] & TILE_DIRECT); cnt["sweep_image_tiles"] += sum(1 for t in l["heavy"] if not t["flags"] & TILE_DIRECT)
        l0, l1 = res["lists"][(g, 0)], res["lists"][(g, 1)]
        fold = expected_fold(sp, bi, res, g, row_nlists, flags, fold_mode)
        if fold["folded"]:
            for br in res["lists"][(g, fold["hs"])]["rows"]: row_zero[br] = False
        # launch_gh_fused: the lists split into {light only, heavy only} and the heavy role costs the light one no LDS
        ls = 0 if (l0["light"] and not l0["heavy"] and l1["heavy"] and not l1["light"]) else 1 if (l1["light"] and not l1["heavy"] and l0["heavy"] and not l0["light"]) else -1
        fused = False
        if ls >= 0 and not fold["folded"]:
            ll, hl = res["lists"][(g, ls)]["light_lds"], res["lists"][(g, 1 - ls)]["heavy_lds"]
            fused = not (max(ll + 2, HROWS * hl + HCHUNK * (TPB + 1)) * 8 > (ll + 2) * 8 + 4096)
        ncost = len(vi); cost_list = -1
        for s in range(2):
            l = res["lists"][(g, s)]
            if l["n"] == ncost and ncost > 0 and l["light"] and not l["heavy"]: cost_list = s; break
        res["groups"].append(dict(cost_list=cost_list, fold=fold, fused=fused))
        cnt["sweep_fold_groups"] += int(fold["folded"]); cnt["sweep_fused_groups"] += int(fused)
    res["zero_rows"] = np.nonzero(row_zero)[0]
    return res


def expected_fold(sp, bi, res, g, row_nlists, flags=0, fold_mode=-1):
    """build_fold for the two-slot group g: dict(folded, why, ls, hs, unique, shared (masks over the slots), ns (per light tile: heavy rows it touches), maxns, copies, cw,
    records (per heavy row: the light tiles that leave a record for it), lds (doubles))."""
    out = dict(folded=False, why="", ls=-1, hs=-1, unique=0, shared=0, ns=[], maxns=0, copies=1, cw=0, records=[], lds=0)
    def no(why): out["why"] = why; return out
    if fold_mode == 0 or fold_mode < 0: return no("NLLS_SWEEP_FOLD: off for a two-slot kind")
    if flags & FLAG_FORCE_ATOMIC: return no("FLAG_FORCE_ATOMIC")
    bi = np.asarray(bi, np.int64); st = res["st"]; vi = np.asarray(sp.groups[g]["varind"], np.int64); ls = -1
    for s in range(2):
        l = res["lists"][(g, s)]
        if l["n"] == 0: continue
        if l["light"] and not l["heavy"]:
            if ls >= 0: return no("two light lists")
            ls = s
        elif not (l["heavy"] and not l["light"]): return no("a list with light and heavy rows")
    if ls < 0 or res["lists"][(g, ls)]["n"] != len(vi): return no("the light list does not hold every cost block")
    T = 1 - ls; H = res["lists"][(g, T)]; Ll = res["lists"][(g, ls)]
    if H["n"] == 0: return no("no heavy list")
    if any(t["flags"] & TILE_DIRECT for t in H["heavy"]): return no("a direct heavy row")
    if np.any(row_nlists[H["rows"]] != 1): return no("a heavy row other lists add to")
    xmask = None
    for r in range(len(H["rows"])):
        x = H["xdest"][H["rowptr"][r]:H["rowptr"][r + 1]]
        if np.any(x != x[0]): return no("a heavy row whose blocks have one writer each")
        xm = int(x[0] != DEST_NONE) << ls
        if xmask is None: xmask = xm
        elif xmask != xm: return no("heavy rows of different shape")
    ds = DOF[T]; cw = ds * (ds + 1) // 2 + ds + (ds * DOF[ls] if xmask else 0)
    if cw > FOLD_MAX_CW: return no("record too wide")
    rowidx = -np.ones(st["nb"], np.int64); rowidx[H["rows"]] = np.arange(len(H["rows"]))
    records = [[] for _ in H["rows"]]; ns = []
    for ti, t in enumerate(Ll["light"]):
        here = []
        for e in range(t["e0"], t["e1"]):
            bv = bi[vi[Ll["cost"][e], T] - 1]
            if not bv: continue
            r = int(rowidx[bv - 1]); assert r >= 0
            if r not in here:
                if len(here) >= FOLD_SLOT_NONE - 1: return no("a tile that touches more than 62 heavy rows")
                here.append(r)
        ns.append(len(here))
        for r in here: records[r].append(ti)
    maxns = max(ns) if ns else 0; cp = 1
    if maxns:
        while cp < 16 and 2 * cp * maxns * cw <= 1024: cp *= 2
    if any(t["flags"] & TILE_PARTIAL for t in Ll["light"]): return no("light rows other lists add to")
    uniq = shared = 0; x = Ll["xdest"]
    if np.any(x != DEST_NONE):
        u, sh = True, True
        for r in range(len(Ll["rows"])):
            xr = x[Ll["rowptr"][r]:Ll["rowptr"][r + 1]]; tmp = xr[xr != DEST_NONE]
            if tmp.size == 0: continue
            if tmp.size != xr.size or np.any(tmp != tmp[0]): sh = False
            if np.unique(tmp).size != tmp.size: u = False
        if u: uniq |= 1 << T
        elif sh: shared |= 1 << T
        else: return no("light rows whose blocks are neither unique nor shared")
    dsl = DOF[ls]; nw = dsl * (dsl + 1) // 2 + dsl + (dsl * DOF[T] if shared else 0)
    lds = max(t["nrows"] * FOLD_ROW_COPIES * nw + n_ * cp * cw for t, n_ in zip(Ll["light"], ns))
    if (lds + 2) * 8 > 64 * 1024: return no("LDS")
    out.update(folded=True, ls=ls, hs=T, unique=uniq, shared=shared, ns=ns, maxns=maxns, copies=cp, cw=cw, records=records, lds=lds)
    return out


def owner_of_entry(res, off):
    """(block row, block column, "g.s light/heavy tile k" of every list that writes the row) of A.data[off] -- for a failing comparison's message"""
    st = res["st"]
    if not st["sparse"]: return (int(off % st["ndof"]), int(off // st["ndof"]), "dense")
    q = int(np.searchsorted(st["nz"], off, side="right") - 1); row, col = int(st["rows"][q]), int(st["rv"][q]); who = []
    for (g, s), l in res["lists"].items():
        for kind in ("light", "heavy"):
            for k, t in enumerate(l[kind]):
                if l["rows"][t["row0"]] <= row <= l["rows"][t["row0"] + t["nrows"] - 1]: who.append(f"{g}.{s} {kind} {k} (flags {t['flags']}, entries {t['e0']}..{t['e1']})")
    return row, col, "; ".join(who)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------
def rows_of(lengths):
    """camera k sees the points 0 .. lengths[k] - 1: one row length per camera; a point is seen by at most len(lengths) cameras"""
    return np.concatenate([np.stack([np.full(n, k), np.arange(n)], axis=1) for k, n in enumerate(lengths)])


def degrees_of(deg):
    """point j is seen by the cameras 0 .. deg[j] - 1"""
    return np.concatenate([np.stack([np.arange(d), np.full(d, j)], axis=1) for j, d in enumerate(deg)])


class Case:
    def __init__(self, sp, check, flags=0, env=None):
        self.sp, self.check, self.flags, self.env = sp, check, flags, dict(env or {})

    def tiles(self):
        if getattr(self, "_tiles", None) is None:
            self._tiles = expected_tiles(self.sp, flags=self.flags, heavy_max=int(self.env.get("NLLS_HEAVY_MAX_ENTRIES", 1024)), fold_mode=int(self.env.get("NLLS_SWEEP_FOLD", -1)))
        return self._tiles

    def reference(self, which):
        """(A.data, b, cost) in integers at variable set 0 (variables) or 1 (variables2), computed once"""
        if getattr(self, "_ref", None) is None: self._ref = {}
        if which not in self._ref: self._ref[which] = exact_system(self.sp, variables=self.sp.variables2 if which else self.sp.variables)
        return self._ref[which]

    def assert_edge(self):
        """the predicate the case exists for, on the restatement alone"""
        t = self.tiles(); self.check(t); return t


def lens(l, kind): return [t["e1"] - t["e0"] for t in l[kind]]
def has_flag(t, f): return bool(t["flags"] & f)
ALL13 = (129, 255, 256, 257, 383, 384, 385, 512, 513, 640, 769, 1024, 1025)
FOLD = {"NLLS_SWEEP_FOLD": "1"}
CASES = {}


def case(f):
    CASES[f.__name__] = functools.lru_cache(maxsize=None)(f); return f


def _heavy_cams_first(t, lengths, fused, nheavy):
    l0, l1 = t["lists"][(0, 0)], t["lists"][(0, 1)]
    assert t["sparse"] and l1["light"] and not l1["heavy"]
    assert sorted(lens(l0, "heavy")) == sorted(sum(([n] if n <= 1024 else [1024, n - 1024] for n in lengths if n > 128), [])) and len(l0["heavy"]) == nheavy
    assert t["groups"][0]["fused"] == fused and t["groups"][0]["cost_list"] == 1
    if not l0["light"]: assert l0["compact"] and l0["own_flags"] == OWN_COST_OWNER


# -- heavy rows, cameras first (compact lists)
@case
def heavy_fused_odd():
    """three heavy camera rows (129, 255, 256): an odd number of heavy tiles -- the second workgroup's spare half walks an empty tile -- and nhw = 2 of nhw_pad = 8"""
    def check(t):
        _heavy_cams_first(t, (129, 255, 256), True, 3)
        assert len(t["lists"][(0, 0)]["heavy"]) % 2 == 1
    return Case(dyadic_ba(rows_of((129, 255, 256))), check)


@case
def heavy_fused_all13():
    """every row length around the multiples of 128, 256 and 384 (the two-set pipeline's rotations and last partial slice); 1025 gives two TILE_PARTIAL pieces; 14 heavy
    tiles, nhw = 7: one workgroup of nhw_pad = 8 idle"""
    def check(t):
        _heavy_cams_first(t, ALL13, True, 14); h = t["lists"][(0, 0)]["heavy"]
        assert [has_flag(x, TILE_PARTIAL) for x in h] == [False] * 12 + [True] * 2 and (len(h) + 1) // 2 % 8 != 0
        assert t["counters"]["sweep_partial_tiles"] == 2 and list(t["zero_rows"]) == [12]
    return Case(dyadic_ba(rows_of(ALL13)), check)


@case
def heavy_fused_xcd():
    """16 cameras, 17 heavy tiles: nhw = 9 > 8, nhw_pad = 16 -- the XCD remap (w & 7) * 2 + (w >> 3) is no identity -- an odd tile count and idle workgroups at once"""
    L = ALL13 + (130, 200, 300)
    def check(t):
        _heavy_cams_first(t, L, True, 17); nhw = (17 + 1) // 2
        assert nhw == 9 and 8 * ((nhw + 7) // 8) >> 3 == 2
    return Case(dyadic_ba(rows_of(L)), check)


@case
def heavy_alone_128():
    """the same 13 rows and one camera of exactly 128 entries: its row is a light tile, list 0 holds light and heavy rows, so the launch is not fused: gh_heavy_kernel,
    three register sets"""
    L = ALL13 + (128,)
    def check(t):
        _heavy_cams_first(t, L, False, 14); l0 = t["lists"][(0, 0)]
        assert lens(l0, "light") == [128] and not l0["compact"]
    return Case(dyadic_ba(rows_of(L)), check)


@case
def heavy_split_128():
    """NLLS_HEAVY_MAX_ENTRIES=128 on rows of 129, 256, 257: 2, 2 and 3 TILE_PARTIAL pieces on rows zero_ranges_kernel clears"""
    def check(t):
        l0 = t["lists"][(0, 0)]
        assert lens(l0, "heavy") == [128, 1, 128, 128, 128, 128, 1] and all(has_flag(x, TILE_PARTIAL) for x in l0["heavy"]) and list(t["zero_rows"]) == [0, 1, 2]
        assert t["groups"][0]["fused"]
    return Case(dyadic_ba(rows_of((129, 256, 257))), check, env={"NLLS_HEAVY_MAX_ENTRIES": "128"})


# -- heavy rows, points first: a camera row owns 18 n + 36 doubles
def _points_first(lengths, **kw): return dyadic_ba(rows_of(lengths), order="elim_first", **kw)


@case
def pf_128_129():
    """points first, camera rows of 128 | 129 entries: a light tile | a heavy row with an LDS image (full list: every entry has its own off-diagonal block)"""
    def check(t):
        l0 = t["lists"][(0, 0)]
        assert lens(l0, "light") == [128] and lens(l0, "heavy") == [129] and l0["heavy"][0]["flags"] == 0 and l0["heavy"][0]["data_len"] == 18 * 129 + 36 and not l0["compact"]
        assert t["counters"]["sweep_image_tiles"] == 1 and t["counters"]["sweep_direct_tiles"] == 0
    return Case(_points_first((128, 129)), check)


@case
def pf_339_340():
    """camera rows of 339 | 340 entries: 18 n + 36 + 6 = 6144 | 6162 doubles: the last LDS image | the first TILE_DIRECT row"""
    def check(t):
        h = t["lists"][(0, 0)]["heavy"]
        assert [x["flags"] for x in h] == [0, TILE_DIRECT | TILE_PARTIAL] and h[0]["data_len"] + 6 == LIGHT_IMG_MAX and h[1]["data_len"] == 0
        assert t["counters"]["sweep_image_tiles"] == 1 and t["counters"]["sweep_direct_tiles"] == 1
    return Case(_points_first((339, 340)), check)


@case
def pf_direct_1100():
    """a direct row of more than 1024 entries (two pieces, HBM atomics) beside an image row"""
    def check(t):
        h = t["lists"][(0, 0)]["heavy"]
        assert lens(t["lists"][(0, 0)], "heavy") == [1024, 76, 200] and [x["flags"] for x in h] == [3, 3, 0]
    return Case(_points_first((1100, 200)), check)


def _hub(fixed_cams):
    ncam = 200; inc = np.concatenate([np.stack([np.arange(ncam), np.full(ncam, j)], axis=1) for j in range(2)])
    fixed = np.zeros(ncam + 2, bool); fixed[list(fixed_cams)] = True
    return dyadic_ba(inc, order="elim_first", fixed=fixed)


@case
def pf_hub_fixed_cameras():
    """two hub POINTS seen by 200 cameras of which three are fixed, points first: the point rows are heavy and own no off-diagonal block, but OWN_COST_OWNER differs from
    entry to entry (a fixed camera's block is counted by the point's entry): the list is not compact.  No list holds every block: the cost sweep reads the cost order"""
    def check(t):
        l1 = t["lists"][(0, 1)]
        assert lens(l1, "heavy") == [200, 200] and not l1["light"] and np.all(l1["xdest"] == DEST_NONE) and 0 < l1["owner"].sum() == 6 and not l1["compact"]
        assert t["groups"][0]["cost_list"] == -1
    return Case(_hub((3, 77, 199)), check)


@case
def pf_hub_compact():
    """the same hubs with no camera fixed: compact, own_flags 0 (the cameras' entries own the cost); the cameras' light list serves the cost sweep"""
    def check(t):
        l1 = t["lists"][(0, 1)]
        assert lens(l1, "heavy") == [200, 200] and l1["compact"] and l1["own_flags"] == 0 and t["groups"][0]["cost_list"] == 0
    return Case(_hub(()), check)


# -- light tiles
@case
def light_256_entries():
    """16 cameras, 48 points seen by all: point tiles of exactly 16 rows = 256 entries (5376 doubles of image: the entries close the tile)"""
    def check(t):
        l1 = t["lists"][(0, 1)]
        assert lens(l1, "light") == [256] * 3 and all(x["nrows"] == 16 for x in l1["light"]) and l1["light_lds"] < LIGHT_IMG_MAX and l1["unique_dest"]
        assert all(x["flags"] == TILE_NOZERO for x in l1["light"])
    return Case(dyadic_ba(degrees_of([16] * 48)), check)


@case
def light_257_entries():
    """the same with one point of 17 entries behind 15 of 16: 240 + 17 = 257 opens a tile"""
    deg = [16] * 15 + [17] + [16] * 32
    def check(t):
        l1 = t["lists"][(0, 1)]; n = lens(l1, "light")
        assert n[0] == 240 and l1["light"][0]["nrows"] == 15 and l1["rowptr"][16] - l1["rowptr"][15] == 17 and max(n) <= 256
    return Case(dyadic_ba(degrees_of(deg)), check)


@case
def light_32x8():
    """64 points seen by 8 cameras: tiles of 32 rows = 256 entries = exactly 6144 doubles; nfold = 32 * 9 = 288 > 256: the fold loop reloads rows[]"""
    def check(t):
        l1 = t["lists"][(0, 1)]
        assert lens(l1, "light") == [256, 256] and l1["light"][0]["nrows"] * 9 > TPB and l1["light_lds"] == LIGHT_IMG_MAX
    return Case(dyadic_ba(degrees_of([8] * 64)), check)


@case
def light_2x128():
    """4 points seen by 128 cameras: tiles of 2 rows of 128 entries, nfold = 18"""
    def check(t):
        l1 = t["lists"][(0, 1)]
        assert lens(l1, "light") == [256, 256] and all(x["nrows"] == 2 for x in l1["light"]) and not l1["heavy"]
    return Case(dyadic_ba(degrees_of([128] * 4)), check)


@case
def light_image_6144():
    """points first, thirteen camera rows with 233 entries between them: sl = 18 n + 150 per row, 6144 doubles: one tile"""
    L = [18] * 12 + [17] + [18]
    def check(t):
        l0 = t["lists"][(0, 0)]
        assert [x["nrows"] for x in l0["light"]] == [13, 1] and lens(l0, "light")[0] == 233 and 18 * 233 + 13 * 150 == LIGHT_IMG_MAX and l0["light_lds"] == LIGHT_IMG_MAX
    return Case(_points_first(L), check)


@case
def light_image_6162():
    """with 234 entries the thirteenth row opens a tile"""
    L = [18] * 13 + [18]
    def check(t):
        l0 = t["lists"][(0, 0)]
        assert [x["nrows"] for x in l0["light"]] == [12, 2] and 18 * 234 + 13 * 150 == LIGHT_IMG_MAX + 18
    return Case(_points_first(L), check)


def _breakers(npts_runs, ncam, cams_of):
    """cameras first, then the points in runs of the given lengths with one BREAKER point between two runs: a free point whose one observation (of a fixed camera behind
    the ncam others) lies in a second group, so it has a block row that group 0's point list does not hold -- the run of consecutive rows ends there.  (A FIXED point
    has no block row and breaks nothing.)  cams_of(k): the cameras of the k-th point of the runs.  Returns (incidences, group_of, fixed)."""
    inc, grp, p, k = [], [], 0, 0
    for i, n in enumerate(npts_runs):
        for _ in range(n):
            cs = list(cams_of(k)); inc += [(c, p) for c in cs]; grp += [0] * len(cs); p += 1; k += 1
        if i + 1 < len(npts_runs): inc.append((ncam, p)); grp.append(1); p += 1
    fixed = np.zeros(ncam + 1 + p, bool); fixed[ncam] = True
    return np.array(inc), np.array(grp), fixed


@case
def light_alignment():
    """point rows are 18 k + 9 doubles, so a tile of an odd number of rows ends on the other parity: one-row and two-row tiles (runs 1, 1, 2, 1, 2 between breaker rows)
    give all four flushes: (data_off odd or even) x (a single trailing double or none)"""
    inc, grp, fixed = _breakers((1, 1, 2, 1, 2, 30), 4, lambda k: range(4))       # (the run of 30: enough rows for a block-sparse system)
    def check(t):
        l1 = t["lists"][(0, 1)]; seen = set()
        for x in l1["light"]:
            assert x["flags"] == TILE_NOZERO
            odd = x["data_off"] & 1; seen.add((odd, odd + 2 * ((x["data_len"] - odd) >> 1) < x["data_len"]))
        assert seen == {(0, False), (0, True), (1, False), (1, True)}, seen
        assert t["sparse"] and [x["nrows"] for x in l1["light"]] == [1, 1, 2, 1, 2, 30]
    return Case(dyadic_ba(inc, fixed=fixed, ngroups=2, group_of=grp), check)


@case
def light_repeat_not_unique():
    """one repeated (camera, point) pair: the whole list is non-unique: LDS atomics for the off-diagonal blocks, images zero-filled"""
    inc = np.concatenate([degrees_of([5] * 40), [[2, 7]]])
    def check(t):
        l1 = t["lists"][(0, 1)]
        assert not l1["unique_dest"] and all(x["flags"] == 0 for x in l1["light"]) and len(l1["light"]) >= 1
    return Case(dyadic_ba(inc), check)


@case
def light_no_repeat_unique():
    """the same without the repeat: TILE_NOZERO"""
    def check(t):
        l1 = t["lists"][(0, 1)]
        assert l1["unique_dest"] and all(x["flags"] == TILE_NOZERO for x in l1["light"])
    return Case(dyadic_ba(degrees_of([5] * 40)), check)


@case
def light_fixed_mix():
    """fixed variables: a fixed point between free ones (no block row: the run goes on), a point seen only by fixed cameras (a row without an off-diagonal block, its
    entries own the cost), a cost whose camera AND point are fixed (the fixed-cost pass counts it once; it appears nowhere in A)"""
    ncam, npts = 6, 40; inc = [(c, p) for p in range(npts) for c in range(ncam) if (c + p) % 2 == 0 or c < 2]
    inc = [(c, p) for (c, p) in inc if not (p == 9 and c >= 2)]                      # point 9: cameras 0 and 1 only, both fixed
    fixed = np.zeros(ncam + npts, bool); fixed[[0, 1]] = True; fixed[ncam + 20] = True
    def check(t):
        sp = SP; l1 = t["lists"][(0, 1)]; bi = np.asarray(sp.bi, np.int64); vi = sp.groups[0]["varind"]
        both = (bi[vi[:, 0] - 1] == 0) & (bi[vi[:, 1] - 1] == 0); assert both.sum() == 2
        r9 = int(bi[sp.pt_var[9]] - 1); k = int(np.nonzero(l1["rows"] == r9)[0][0]); e = slice(l1["rowptr"][k], l1["rowptr"][k + 1])
        assert np.all(l1["xdest"][e] == DEST_NONE) and np.all(l1["owner"][e]) and e.stop - e.start == 2
        assert np.all(np.diff(l1["rows"]) == 1) and t["groups"][0]["cost_list"] == -1 and len(l1["rows"]) == npts - 1
    SP = dyadic_ba(np.array(inc), fixed=fixed)
    return Case(SP, check)


@case
def light_two_groups():
    """ngroups = 2: every row is shared by two lists: TILE_PARTIAL everywhere, HBM atomics, every row in the zero ranges"""
    def check(t):
        tiles = [x for l in t["lists"].values() for x in l["light"] + l["heavy"]]
        assert all(has_flag(x, TILE_PARTIAL) and not has_flag(x, TILE_NOZERO) for x in tiles) and len(t["zero_rows"]) == t["st"]["nb"]
        assert t["counters"]["sweep_partial_tiles"] == len(tiles) and t["counters"]["sweep_image_tiles"] == 4 and all(G["cost_list"] == 1 for G in t["groups"])
    inc = rows_of((300, 300, 60))
    return Case(dyadic_ba(inc, ngroups=2, group_of=(inc[:, 0] + inc[:, 1]) % 2), check)


@case
def light_two_groups_exclusive():
    """two groups where the points 20 .. 59 appear in group 0 only: exclusive and shared rows fall in separate tiles"""
    inc = degrees_of([4] * 80); grp = np.where((inc[:, 1] >= 20) & (inc[:, 1] < 60), 0, np.arange(len(inc)) % 2)
    def check(t):
        l1 = t["lists"][(0, 1)]; fl = [x["flags"] for x in l1["light"]]
        assert TILE_PARTIAL in fl and TILE_NOZERO in fl
        for x in l1["light"]:
            pts = l1["rows"][x["row0"]:x["row0"] + x["nrows"]] - 4
            assert np.all((pts >= 20) & (pts < 60)) == (x["flags"] == TILE_NOZERO)
    return Case(dyadic_ba(inc, ngroups=2, group_of=grp), check)


@case
def light_force_atomic():
    """FLAG_FORCE_ATOMIC: every tile partial although every row has one list"""
    def check(t):
        tiles = [x for l in t["lists"].values() for x in l["light"] + l["heavy"]]
        assert all(has_flag(x, TILE_PARTIAL) for x in tiles) and any(l["heavy"] for l in t["lists"].values())
    return Case(dyadic_ba(rows_of((140, 100, 60))), check, flags=FLAG_FORCE_ATOMIC)


# -- the folded sweep (NLLS_SWEEP_FOLD=1, cameras first): record width cw = 21 + 6 = 27
def _fold_case(inc, check, folded=True, **kw):
    def chk(t):
        assert t["sparse"]; f = t["groups"][0]["fold"]
        assert f["folded"] == folded, f["why"]
        if folded: assert f["cw"] == 27 and f["ls"] == 1 and t["counters"]["sweep_fold_groups"] == 1 and t["counters"]["sweep_fused_groups"] == 0
        check(t, f)
    return Case(dyadic_ba(inc, **kw), chk, env=FOLD)


def _fold_maxns(m):
    """m cameras of 129 .. rows: every point tile touches exactly m cameras"""
    inc = degrees_of([m] * max(130, 2 * (256 // m)))
    def check(t, f):
        assert f["maxns"] == m and set(f["ns"]) == {m} and f["copies"] == {1: 16, 2: 16, 3: 8, 4: 8, 5: 4, 9: 4, 10: 2, 18: 2, 19: 1}[m] and f["unique"] == 1 and f["shared"] == 0
    return _fold_case(inc, check)


for _m in (1, 2, 3, 4, 5, 9, 10, 18, 19):
    CASES[f"fold_maxns_{_m}"] = functools.lru_cache(maxsize=None)(functools.partial(_fold_maxns, _m))


def _fold_tile_cams(ncam):
    """1040 points, point j seen by the eight cameras 8 j .. 8 j + 7 (mod ncam): every tile of 32 rows touches every camera, every camera has more than 128 entries"""
    return np.array([((8 * j + i) % ncam, j) for j in range(1040) for i in range(8)])


@case
def fold_62_cameras():
    """a tile that touches 62 distinct cameras: the last that folds"""
    def check(t, f): assert f["maxns"] == 62 and f["copies"] == 1
    return _fold_case(_fold_tile_cams(62), check)


@case
def fold_63_cameras():
    """63: build_fold declines, the group is fused instead"""
    def check(t, f): assert "62" in f["why"] and t["counters"]["sweep_fold_groups"] == 0 and t["groups"][0]["fused"]
    return _fold_case(_fold_tile_cams(63), check, folded=False)


@case
def fold_row_three_wavefronts():
    """point 0: one observation by camera 0; point 1: 128 by camera 1 -- the row starts at lane 1 and spans three wavefronts, the first and the third add to the same
    accumulator copy of the row; points 2 and 3 the same with the cameras swapped (both cameras 129 entries: heavy).  Tiles of 129 entries: the lanes without an entry
    evaluate and add nothing"""
    inc = [(0, 0)] + [(1, 1)] * 128 + [(0, 2)] * 128 + [(1, 3)] + [(p % 2, p) for p in range(4, 44) for _ in range(2)]      # (40 more points: a block-sparse system)
    def check(t, f):
        l1 = t["lists"][(0, 1)]; x = l1["light"][0]
        assert list(np.diff(l1["rowptr"])[:4]) == [1, 128, 128, 1] and (x["e0"], x["e1"], x["nrows"]) == (0, 129, 2) and l1["light"][1]["e1"] - 129 < 256 and f["shared"] == 1
    return _fold_case(np.array(inc), check)


@case
def fold_shared_block():
    """every point observed three times by ONE camera: the light rows' block is shared by the row's entries (shared_mask)"""
    inc = [(p % 2, p) for p in range(300) for _ in range(3)]
    def check(t, f): assert f["shared"] == 1 and f["unique"] == 0 and not t["lists"][(0, 1)]["unique_dest"]
    return _fold_case(np.array(inc), check)


@case
def fold_neither_unique_nor_shared():
    """the same and one point with two cameras: neither unique nor shared: not folded"""
    inc = [(p % 2, p) for p in range(300) for _ in range(3)] + [(1, 0)]
    def check(t, f): assert "neither" in f["why"]
    return _fold_case(np.array(inc), check, folded=False)


@case
def fold_records_1():
    """camera 0's 130 entries (65 points observed twice) lie in one tile: its heavy row is gathered from ONE record"""
    inc = [(0, p) for p in range(65) for _ in range(2)] + [(1, 65 + p) for p in range(100) for _ in range(2)]
    def check(t, f): assert [len(r) for r in f["records"]][0] == 1 and f["shared"] == 1
    return _fold_case(np.array(inc), check)


def _fold_records_case(nrec):
    """camera 0 is seen by nrec points, each a tile of its own (one-row tiles: breaker rows between them): nrec records; camera 1 by 140 more points"""
    inc, grp, fixed = _breakers((1,) * nrec + (140,), 2, lambda k: (0,) if k < nrec else (1,))
    def chk(t):
        f = t["groups"][0]["fold"]; assert f["folded"], f["why"]
        assert t["counters"]["sweep_fold_groups"] == 1 and not t["groups"][1]["fold"]["folded"] and f["unique"] == 1
        assert [len(r) for r in f["records"]][0] == nrec and len(t["lists"][(0, 0)]["heavy"]) == (nrec + 1023) // 1024 + 1
    return Case(dyadic_ba(inc, fixed=fixed, ngroups=2, group_of=grp), chk, env=FOLD)


for _n in (256, 257, 4096, 4097):
    CASES[f"fold_records_{_n}"] = functools.lru_cache(maxsize=None)(functools.partial(_fold_records_case, _n))


# -- dense systems (gh_dense_kernel)
def _dense_check(t): assert not t["sparse"] and not any(t["counters"].values())


def _dense(inc, env=None, **kw): return Case(dyadic_ba(np.array(inc), **kw), _dense_check, env=env)


for _td in ("1", "0"):
    CASES[f"dense_small_tiny{_td}"] = functools.lru_cache(maxsize=None)(functools.partial(lambda td: _dense(degrees_of([3] * 5), env={"NLLS_TINY_DENSE": td}), _td))
    CASES[f"dense_small_fixed_tiny{_td}"] = functools.lru_cache(maxsize=None)(functools.partial(
        lambda td: _dense(degrees_of([3] * 5), env={"NLLS_TINY_DENSE": td}, fixed=np.array([0, 1, 0, 0, 0, 1, 0, 0], bool)), _td))


@case
def dense_63_unknowns():
    """9 cameras and 3 points: 63 unknowns, the image of [A | b] in LDS (use_lds), the general kernels"""
    def check(t): _dense_check(t); assert t["st"]["ndof"] == 63
    return Case(dyadic_ba(degrees_of([9] * 3)), check, env={"NLLS_TINY_DENSE": "0"})


@case
def dense_66_unknowns():
    """10 cameras and 2 points: 66 unknowns, atomics straight into A and b"""
    def check(t): _dense_check(t); assert t["st"]["ndof"] == 66
    return Case(dyadic_ba(degrees_of([10] * 2)), check, env={"NLLS_TINY_DENSE": "0"})


@case
def dense_uniform_wavefront():
    """70 observations of one (camera, point) pair, then mixed ones: the first wavefront is uniform (summed on the VALU, one add), the second is not; 70 + 150 = 220 costs:
    the last wavefront is partly valid"""
    inc = [(1, 2)] * 70 + [(k % 4, k % 3) for k in range(150)]
    def check(t): _dense_check(t); assert t["st"]["ndof"] <= 64 and len(inc) % 64 != 0
    return Case(dyadic_ba(np.array(inc)), check, env={"NLLS_TINY_DENSE": "0"})


def _dense_stride(n):
    inc = np.stack([np.arange(n) % 6, (np.arange(n) // 6) % 64], axis=1); fixed = np.r_[np.zeros(6, bool), np.ones(64, bool)]
    def check(t): _dense_check(t); assert t["st"]["ndof"] == 36 and n - TPB * TINY_DENSE_MAX_WGS in (0, 1)
    return Case(dyadic_ba(inc, fixed=fixed), check)


CASES["dense_65536_costs"] = functools.lru_cache(maxsize=None)(functools.partial(_dense_stride, 65536))
CASES["dense_65537_costs"] = functools.lru_cache(maxsize=None)(functools.partial(_dense_stride, 65537))


# -- the cost sweep
@case
def cost_heavy_point_and_camera():
    """camera 0 sees all 129 points and point 0 is seen by all 129 cameras: both lists hold a heavy row beside light ones, so no list serves the cost sweep (cost_list
    -1: it reads the cost order) and the accumulate sweep takes one launch per slot and role"""
    inc = [(0, p) for p in range(129)] + [(c, 0) for c in range(1, 129)] + [(c, 1 + c % 128) for c in range(1, 129)]
    def check(t):
        l0, l1 = t["lists"][(0, 0)], t["lists"][(0, 1)]
        assert lens(l0, "heavy") == [129] and lens(l1, "heavy") == [129] and l0["light"] and l1["light"] and t["groups"][0]["cost_list"] == -1 and not t["groups"][0]["fused"]
    return Case(dyadic_ba(np.array(inc)), check)


# -- the cost sweep's grid
def _cost_grid(grid, extra):
    n = TPB * grid + extra; inc = degrees_of([4] * (n // 4)) if n % 4 == 0 else np.concatenate([degrees_of([4] * (n // 4)), [[0, 0]] * (n % 4)])
    def check(t): assert t["sparse"] and sum(len(G["varind"]) for G in SP.groups) == n and t["groups"][0]["cost_list"] >= 0
    SP = dyadic_ba(inc)
    return Case(SP, check, env={"NLLS_COST_GRID_MAX": str(grid)})


for _g in (1, 3):
    for _x in (0, 1):
        CASES[f"cost_grid{_g}_plus{_x}"] = functools.lru_cache(maxsize=None)(functools.partial(_cost_grid, _g, _x))
