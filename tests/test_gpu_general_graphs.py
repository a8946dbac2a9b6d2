"""The sparse Schur path on problems that are not bundle adjustment.

Every sparse problem of the other GPU tests is bipartite: no cost block couples two reduced variables (but for the adaptive kernel's variable), the eliminated variable
sits in one fixed slot of a two- or three-slot kind, the eliminated class is the 3-dof points and the reduced system has one block size.  The symbolic phase
(csrc/nlls_structure.cpp: select_elimination, build_schur) is written for any graph.  The problems of tests/test_general_graphs.py -- pinned there on the CPU: structure,
the mirror of select_elimination, the oracle's step against a long-double Schur step, indifference to the variable order -- go through tests/test_gpu_parity.check_problem
at that file's tolerances, unchanged, under the flags that select the reduced solver and under variable orders other than the generator's; every case asserts the branch
it exists for through nlls_get_solve_stats (tests/test_gpu_variable_order.branch_stats, which prints the COUNTERS line).  The LM loop, nlls_optimize_singles,
nlls_eval_blocks and nlls_set_cost_data follow on the shared-leaves graph and the mixed-size problem."""
import time

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import _capi
from tests.helpers import (oracle_problem, blockindices, permute_variables, expected_elimination, structure_counts,
                           scalar_graph_problem, shared_leaves_edges)
from tests.test_general_graphs import CASES, SCALAR_SCHUR, NO_SCHUR, ORDERS, case_problem, case_order, fixed_pair
from tests.test_gpu_parity import check_problem
from tests.test_gpu_variable_order import branch_stats

pytestmark = pytest.mark.gpu

F = _capi
FLAGS = {"default": 0, "no_bcr": F.FLAG_NO_BCR, "no_bcr_no_twist": F.FLAG_NO_BCR | F.FLAG_NO_TWIST, "no_band": F.FLAG_NO_BAND, "force_atomic": F.FLAG_FORCE_ATOMIC,
         "deterministic": F.FLAG_DETERMINISTIC}
ELIM_COUNTERS = ("elim_fast60", "elim_fast_narrow", "elim_fast_wide", "elim_slow_acc", "elim_slow_noacc", "elim_nbrs", "elim_nbrs_transposed", "elim_supernodes")
seen = dict(fast_one_dof=0, slow_one_dof=0)          # over the scalar-graph cases of one run: test_scalar_graphs_reach_both_supernode_classes


def run_case(name, order="identity", flags="default", unfixed=None):
    """check_problem on the case's problem in the named order; the structure the device chose against the mirror of select_elimination on the SAME (permuted) problem --
    the greedy set breaks ties of degree in block order, so another order may give another set, or one under half of the blocks and no Schur complement at all.
    Returns (info, counters, mirror's counts)."""
    p, want, elim = case_problem(name)
    perm = case_order(order, elim); q, _ = permute_variables(p, perm)
    uf = None if unfixed is None else unfixed[perm]
    bi = blockindices(q, uf); ols = oracle_problem(q).linear_system(bi); mirror = expected_elimination(ols); cnt = structure_counts(q, ols, mirror, bi)
    assert cnt["independent"]
    info = check_problem(q, unfixed=uf, flags=FLAGS[flags], expect_sparse=1, expect_schur=int(mirror.any()), lam_scale=want.get("lam", 1e-6))
    assert info.nschur_blocks == cnt["nelim"] and info.nreduced_dof == cnt["nreduced_dof"], (info.nschur_blocks, info.nreduced_dof, cnt)
    _, st = branch_stats(q, f"{name}-{order}-{flags}" + ("-fixed" if unfixed is not None else ""), unfixed=uf, flags=FLAGS[flags], lam_scale=want.get("lam", 1e-6))
    if mirror.any():
        assert st["elim_nbrs"] > 0 and st["fast"] + st["slow"] == st["elim_supernodes"] > 0, st
    else:
        assert all(st[k] == 0 for k in ELIM_COUNTERS), st               # (the whole block-sparse system is the "reduced" one: whichever solver its size and band select)
    if order == "identity" and unfixed is None:                        # the generator's own order: what CASES states
        assert cnt["nelim"] == want["nelim"] and cnt["nreduced_dof"] == want["nred"], cnt
    return info, st, cnt


# ---- one-dof graphs -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", SCALAR_SCHUR)
def test_scalar_graphs(name, order, flags):
    info, st, cnt = run_case(name, order, flags)
    want = CASES[name][1]
    assert st["mf_trials"] == 0, st                                     # two groups / both orientations: never the matrix-free trial
    if order in ("identity", "elim_first", "reversed") or not name.startswith(("chain", "hub")):
        assert info.has_schur == 1                                      # (a chain's greedy set under a random order may stay under half: run_case asserts what the mirror gives)
    if order == "identity":
        assert (cnt["mixed_slots"] > 0) == want["mixed"] and cnt["reduced_reduced"] == want["rr"], cnt
        if want["mixed"]: assert cnt["mixed_slots"] >= want["nelim"] // 4, cnt          # (half of the two-edge variables draw both orientations)
        if want["nred"] < 64: assert info.solve_mode == 0, info.solve_mode
        else:
            assert want["nred"] >= 128 and info.solve_mode == (1 if flags == "no_band" else 2), (info.solve_mode, info.bandwidth)
        if want.get("border"): assert info.nborder_dof >= 1, info.nborder_dof
    if info.has_schur:
        seen["fast_one_dof"] += st["fast"] > 0; seen["slow_one_dof"] += st["slow"] > 0


def test_scalar_graphs_reach_both_supernode_classes():
    """over the cases above (this test runs behind them): one-dof eliminated variables on the fast supernodes in at least one case, on the generic ones in at least one"""
    if not (seen["fast_one_dof"] or seen["slow_one_dof"]):             # run on its own: two cases that settle it
        for order in ("identity", "elim_first"):
            _, st, _ = run_case("caterpillar-30", order); seen["fast_one_dof"] += st["fast"] > 0; seen["slow_one_dof"] += st["slow"] > 0
    assert seen["fast_one_dof"] > 0 and seen["slow_one_dof"] > 0, seen


@pytest.mark.parametrize("order", ["identity", "reversed", "random"])          # (nothing eliminated: elim_first is the identity)
@pytest.mark.parametrize("name", NO_SCHUR)
def test_independent_sets_under_half_take_no_schur_complement(name, order):
    info, st, cnt = run_case(name, order)
    assert info.has_schur == 0 and info.is_sparse == 1 and info.nschur_blocks == 0 and info.nreduced_dof == info.ndof
    assert all(st[k] == 0 for k in ELIM_COUNTERS), st


# ---- four slots ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["curves_a-60x5", "curves_d-60x5", "curves_a-70x5"])
def test_curve_families(name, order):
    """60 eliminated scalars in slot 0 / slot 3 of a four-slot kind, five cost blocks per (eliminated, neighbour) pair; the three reduced scalars coupled to one another by
    those same blocks: S is 3 x 3, every entry a copied block with 60 Schur updates on top.  With 70 curves the three shared scalars are border blocks, the band part of
    the reduced system is empty."""
    info, st, cnt = run_case(name, order); want = CASES[name][1]; n = want["nelim"]
    assert info.has_schur == 1 and info.nschur_blocks == n and info.nreduced_dof == 3 and st["elim_nbrs"] == 3 * n > 0, (st, info.nreduced_dof)
    assert cnt["reduced_reduced"] == 3 and cnt["elim_slots"] == want["elim_slots"] and info.solve_mode == 0
    assert info.nborder_dof == (3 if want.get("border") else 0), info.nborder_dof


# ---- several block sizes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["mixed-linear3", "mixed-cost3", "mixed-adaptive_mean"])
def test_mixed_block_sizes(name, order):
    info, st, cnt = run_case(name, order)
    assert info.has_schur == 1 and cnt["reduced_sizes"] == [1, 6] and cnt["elim_sizes"] == [3], cnt
    if name == "mixed-adaptive_mean":
        p, _, elim = case_problem(name)
        print(f"ADAPTIVE_MEAN {order}: the mirror eliminates the kernel variable in the identity order: {bool(elim[162])}; eliminated here {cnt['nelim']} (150 points + the kernel variable = 151)")
        assert info.nschur_blocks in (150, 151)
    else:
        assert info.nschur_blocks == 150 and info.nreduced_dof == 112 and cnt["reduced_reduced"] == 39, cnt
        if order == "identity": assert st["fast"] > 0 and st["mf_trials"] == 0, st     # (a unary group on eliminated points beside the coupling group)


# ---- the 6-dof class eliminated -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["identity", "elim_first", "random"])
@pytest.mark.parametrize("name", ["many_cameras-affine", "many_cameras-so3"])
def test_cameras_outnumber_points(name, order):
    """120 cameras / SO(3) poses eliminated, 30 points reduced: supernodes of 6-dof members (nothing fast: fast_dv <= 3), and for SO(3) the retraction of ELIMINATED poses
    behind the back-substitution against the oracle's update (check_problem: 1e-13)"""
    info, st, cnt = run_case(name, order)
    assert info.has_schur == 1 and info.nschur_blocks == 120 and info.nreduced_dof == 90 and cnt["elim_sizes"] == [6]
    assert st["fast"] == 0 and st["slow"] > 0 and st["mf_trials"] == 0, st


# ---- fixed variables ----------------------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ["chain-100", "caterpillar-30", "shared_leaves-20", "hub-61", "triangular_lattice-12", "square_lattice-12", "curves_ab-30x5", "curves_a-60x5", "curves_d-60x5", "curves_a-70x5",
            "mixed-linear3", "mixed-cost3", "mixed-adaptive_mean", "many_cameras-affine", "many_cameras-so3"]


@pytest.mark.parametrize("name", FAMILIES)
def test_two_fixed_variables(name):
    """one variable of the eliminated set and one of the reduced system fixed (blockindices(p, unfixed)): their cost blocks stay, with fewer free slots"""
    uf = fixed_pair(name); _, want, elim = case_problem(name)
    assert (~uf).sum() == 2 and (not elim.any() or (elim[~uf].sum() == 1))
    info, st, cnt = run_case(name, unfixed=uf)
    # (the greedy set depends on the blocks that are left: the square lattice and the two-parameter curves reach half of their blocks once two are fixed -- 72 of 142 and
    # 30 of 60 -- and take a Schur complement with reduced-reduced blocks; run_case holds the device to the mirror either way)
    print(f"FIXED {name}: schur={info.has_schur} eliminated {info.nschur_blocks} reduced-reduced blocks {cnt['reduced_reduced']}")
    if want["nelim"]: assert info.has_schur == 1


# ---- the layers above the solve ---------------------------------------------------------------------------------------------------------------------------------------
LAYERS = ["shared_leaves-20", "mixed-linear3"]


def _fresh(name):
    return CASES[name][0]()


@pytest.mark.parametrize("name", LAYERS)
def test_optimize_matches_oracle(name):
    """tests/test_gpu_functional.test_randomized_optimize_matches_oracle: 60 iterations; the scalar graph has a zero-residual optimum (every variable 1: a (1 - x) and
    b (x^2 - y) all vanish) that both must reach, below 1e-15 per cost block; the mixed problem (noise, a Huber kernel) the same best cost to 1e-6"""
    p = _fresh(name); op = oracle_problem(_fresh(name))
    res = N.optimize(p, N.NLLSOptions(maxiters=60)); ores = op.optimize(maxiters=60)
    print(f"OPTIMIZE {name}: {res.startcost:.6e} -> {res.bestcost:.12e} (oracle {ores.bestcost:.12e})")
    if name.startswith("shared_leaves"):
        assert res.bestcost < 1e-15 * p.ncosts() and ores.bestcost < 1e-15 * p.ncosts(), (res.bestcost, ores.bestcost)
        assert np.max(np.abs(p.variables - 1.0)) < 1e-7
    else:
        assert res.bestcost < res.startcost and np.isclose(res.bestcost, ores.bestcost, rtol=1e-6), (res.bestcost, ores.bestcost)


@pytest.mark.parametrize("name", LAYERS)
def test_native_lm_loop_is_the_python_loop(name):
    """tests/test_gpu_functional.test_native_lm_loop_is_the_python_loop on these problems: nlls_lm_iterations against the Python statements of the same loop, one outer
    iteration at a time"""
    from nllssolver_jl_amd import iterators as It, optimizer as Opt
    from nllssolver_jl_amd.linearsystem import makesymmvls
    hist = {}
    for native in (True, False):
        p = _fresh(name)
        ls = makesymmvls(p, np.ones(p.nvariables, bool), 0, 0)
        data = Opt.NLLSInternal(ls, time.perf_counter_ns())
        loop = Opt.OuterLoop(p, N.NLLSOptions(maxiters=12), data, It.LevMarData(), It.iterate_levmar, N.nullcallback, native)
        assert loop.native == native
        loop.start(); rows = []
        while True:
            c = loop.iterations(1)
            rows.append((loop.cost, data.bestcost, loop.iteratedata.lambda_, data.linearsolvers, data.costcomputations, data.gradientcomputations, c))
            if c: break
        loop.finish()
        hist[native] = (rows, data.iternum); ls.close()
    (ra, na), (rb, nb) = hist[True], hist[False]
    assert na == len(ra) and nb == len(rb) and abs(na - nb) <= 2, (na, nb)
    prev = None
    for k, (x, y) in enumerate(zip(ra, rb)):
        early = k < 8 and (prev is None or (prev - x[1]) > 1e-6 * abs(prev))
        prev = x[1]
        assert np.isclose(x[0], y[0], rtol=1e-8) and np.isclose(x[1], y[1], rtol=1e-8), (k, x, y)
        if early: assert np.isclose(x[2], y[2], rtol=1e-5) and x[3:6] == y[3:6], (k, x, y)
    assert ra[-1][6] != 0 and rb[-1][6] != 0


def test_optimizesingles_over_a_mixed_slot_eliminated_set():
    """nlls_optimize_singles over the mirror's eliminated set of the shared-leaves graph: a variable's cslot list holds 0 and 1; leaf 0 has 67 blocks (its three edges listed
    22 times, and its unary block) and takes the wave kernel, every other leaf (4 blocks) a thread.  Against the oracle as
    tests/test_gpu_functional.test_randomized_optimizesingles_matches_oracle."""
    from tests.test_gpu_functional import _oracle_optimizesingles
    from nllssolver_jl_amd import optimizer
    e, n = shared_leaves_edges(20, 120, heavy=21); p = scalar_graph_problem(e, n, seed=5)
    elim = expected_elimination(oracle_problem(p).linear_system(blockindices(p))); sel = np.nonzero(elim)[0] + 1
    cptr, _, _, cslot = p.costlists(sel)
    assert sel.size == 120 and cptr[1] - cptr[0] >= 64 and set(cslot[cptr[0]:cptr[1]].tolist()) == {0, 1}
    both = sum(set(cslot[cptr[i]:cptr[i + 1]][:-1].tolist()) == {0, 1} for i in range(sel.size)); assert both >= 30, both
    c0 = N.cost(p)
    expect = _oracle_optimizesingles(p, sel)
    iters = N.optimizesingles(p, N.NLLSOptions(), indices=sel)
    err = np.max(np.abs(p.variables - expect))
    print(f"SINGLES shared_leaves: cost {c0:.6e} -> {N.cost(p):.6e}, max |variables - oracle| {err:.3e}, {optimizer.last_singles_stats}")
    assert iters.shape == (120,) and iters.min() >= 1 and N.cost(p) <= c0
    assert optimizer.last_singles_stats["singles_wave"] >= 1 and optimizer.last_singles_stats["singles_thread"] >= 1, optimizer.last_singles_stats
    assert err < 1e-7, err


@pytest.mark.parametrize("name", LAYERS)
def test_eval_blocks_of_every_group(name):
    from tests.test_gpu_blockeval import check_against_oracle
    p = _fresh(name); assert len(p.costs) == (2 if name.startswith("shared") else 4)
    check_against_oracle(name, p)


@pytest.mark.parametrize("name,kind,a_moves", [("shared_leaves-20", K.RES_ROSENBROCK_B, True), ("mixed-linear3", K.RES_LINEAR3, False)])
def test_set_cost_data(name, kind, a_moves):
    from tests.test_gpu_update import run_case as update_case
    p = _fresh(name); group = [g.res_kind for g in p.costs.values()].index(kind)
    update_case(p, group=group, a_moves=a_moves, lam_scale=CASES[name][1].get("lam", 1e-6))
