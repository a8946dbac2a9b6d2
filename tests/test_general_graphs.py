"""Problems that are not bundle adjustment, pinned on the CPU: what tests/test_gpu_general_graphs.py runs on the device.

nlls_upload_structure takes any graph of cost blocks; every sparse problem of the generators is bipartite, with the eliminated variable in one fixed slot of one
two- or three-slot kind, 3-dof points eliminated and one block size in the reduced system.  CASES lists graphs of other shapes (tests/helpers.py: chains, lattices,
caterpillars, leaves shared by consecutive hubs, a hub coupled to everything, curve families over four slots, bundle adjustment beside components of other sizes,
cameras that outnumber their points).  For each of them this file pins, with the oracle alone:
  * the linear system is block-sparse;
  * the mirror of select_elimination (tests/helpers.expected_elimination) gives an independent set of the size, block sizes, slot mix and number of reduced-reduced
    stored blocks the case was written for -- a case that claims mixed slots has eliminated variables seen in both slots of one cost group;
  * the oracle's damped step lies within 1e-9 (relative, max-norm) of tests/helpers.longdouble_schur_step over the mirror's set: 100 x under the 1e-7 the device's step is
    held to, so the reference alone stays inside the device tests' tolerance;
  * tests/helpers.permute_variables leaves the oracle's cost and step unchanged, to the tolerances of tests/test_variable_order.py."""
import numpy as np
import pytest

from tests.helpers import (oracle_problem, blockindices, bsm_to_csr, longdouble_schur_step, permute_variables, to_original_order, variable_sizes, NAMED_ORDERS,
                           expected_elimination, structure_counts, greedy_independent_set, scalar_graph_problem, chain_edges, lattice_edges,
                           caterpillar_edges, shared_leaves_edges, hub_edges, curve_family_problem, mixed_sizes_problem, many_cameras_problem)

U = np.finfo(np.float64).eps / 2
STEP_BOUND = 1e-9
ORDERS = ("identity", "elim_first", "reversed", "random")


def _scalar(builder, *args, seed=0, **kw):
    return lambda mix_slots=True: scalar_graph_problem(*builder(*args), seed=seed, mix_slots=mix_slots, **kw)


# name -> (maker, what the case is written for).  nelim / rr (reduced-reduced stored blocks) / nred (reduced dof) in the identity order with nothing fixed; mixed: eliminated
# variables are seen in both slots of the coupling group; sizes: (eliminated block size, reduced block sizes); lam: the damping of the device checks, relative to max |diag|.
CASES = {
    # one-dof graphs, b (x^2 - y) on the edges and a - x on every variable
    "chain-100": (_scalar(chain_edges, 100, seed=1), dict(nelim=50, rr=1, nred=50, mixed=True, sizes=(1, [1]))),
    "chain-300": (_scalar(chain_edges, 300, seed=2), dict(nelim=150, rr=1, nred=150, mixed=True, sizes=(1, [1]))),
    "caterpillar-30": (_scalar(caterpillar_edges, 30, seed=3), dict(nelim=120, rr=57, nred=30, mixed=False, sizes=(1, [1]))),
    "caterpillar-130": (_scalar(caterpillar_edges, 130, seed=4), dict(nelim=520, rr=257, nred=130, mixed=False, sizes=(1, [1]))),
    "shared_leaves-20": (_scalar(shared_leaves_edges, 20, 120, seed=5), dict(nelim=120, rr=19, nred=20, mixed=True, sizes=(1, [1]))),
    "shared_leaves-130": (_scalar(shared_leaves_edges, 130, 400, seed=6), dict(nelim=400, rr=129, nred=130, mixed=True, sizes=(1, [1]))),
    "hub-61": (_scalar(hub_edges, 61, 40, seed=7), dict(nelim=71, rr=30, nred=31, mixed=True, sizes=(1, [1]), border=True)),
    "hub-301": (_scalar(hub_edges, 301, seed=8), dict(nelim=151, rr=150, nred=151, mixed=True, sizes=(1, [1]), border=True)),
    # independent sets under half of the blocks: no Schur complement, the whole block-sparse system goes to the dense solver
    "triangular_lattice-12": (_scalar(lattice_edges, 12, 12, True, seed=9), dict(nelim=0, nred=144, sizes=(None, [1]))),
    "square_lattice-12": (_scalar(lattice_edges, 12, 12, False, seed=10), dict(nelim=0, nred=144, sizes=(None, [1]))),
    "curves_ab-30x5": (lambda: curve_family_problem(30, 5, (0, 1), seed=11), dict(nelim=0, nred=62, sizes=(None, [1]))),
    # four slots: the curves' own parameter eliminated in slot 0 / slot 3, the three shared scalars fully coupled by the same blocks
    "curves_a-60x5": (lambda: curve_family_problem(60, 5, (0,), seed=12), dict(nelim=60, rr=3, nred=3, mixed=False, sizes=(1, [1]), elim_slots=[0])),
    "curves_d-60x5": (lambda: curve_family_problem(60, 5, (3,), seed=13), dict(nelim=60, rr=3, nred=3, mixed=False, sizes=(1, [1]), elim_slots=[3])),
    # 70 eliminated scalars (64 or more): each shared scalar couples to all of them and becomes a BORDER block -- the reduced system is border only, its band part empty
    "curves_a-70x5": (lambda: curve_family_problem(70, 5, (0,), seed=14), dict(nelim=70, rr=3, nred=3, mixed=False, sizes=(1, [1]), elim_slots=[0], border=True)),
    # several block sizes
    "mixed-linear3": (lambda: mixed_sizes_problem("linear3"), dict(nelim=150, rr=39, nred=112, mixed=False, sizes=(3, [1, 6]), lam=1e-4)),
    "mixed-cost3": (lambda: mixed_sizes_problem("cost3"), dict(nelim=150, rr=39, nred=112, mixed=False, sizes=(3, [1, 6]), lam=1e-4)),
    "mixed-adaptive_mean": (lambda: mixed_sizes_problem("adaptive_mean"), dict(nelim=151, rr=0, nred=74, mixed=False, sizes=(3, [1, 6]), lam=1e-4)),
    # the 6-dof class eliminated
    "many_cameras-affine": (lambda: many_cameras_problem(False), dict(nelim=120, rr=0, nred=90, mixed=False, sizes=(6, [3]), lam=1e-4)),
    "many_cameras-so3": (lambda: many_cameras_problem(True), dict(nelim=120, rr=0, nred=90, mixed=False, sizes=(6, [3]), lam=1e-4)),
}
SCALAR_SCHUR = [n for n in CASES if n.split("-")[0] in ("chain", "caterpillar", "shared_leaves", "hub")]
NO_SCHUR = ["triangular_lattice-12", "square_lattice-12", "curves_ab-30x5"]

_cache = {}


def case_problem(name):
    """(problem, expectations, eliminated variables by the mirror): built once; callers must not change the problem (permute_variables copies)"""
    if name not in _cache:
        p = CASES[name][0](); ols = oracle_problem(p).linear_system(blockindices(p))
        _cache[name] = (p, CASES[name][1], expected_elimination(ols))
    return _cache[name]


def case_order(order, elim):
    """perm[new] = old of a named order; elim_first where the generator already lists the eliminated variables first (the curves' own parameters, the cameras that
    outnumber their points) lists the reduced ones first instead: the order the generator does not have"""
    perm = NAMED_ORDERS[order](elim)
    if order == "elim_first" and np.array_equal(perm, np.arange(len(elim))): perm = NAMED_ORDERS[order](~np.asarray(elim, bool))
    return perm


def fixed_pair(name):
    """`unfixed` with two variables fixed: the first the mirror eliminates and the last it leaves in the reduced system"""
    p, _, elim = case_problem(name); unfixed = np.ones(p.nvariables, bool)
    unfixed[np.nonzero(elim)[0][0] if elim.any() else 0] = False; unfixed[np.nonzero(~elim)[0][-1]] = False
    return unfixed


def _linearise(p, lam_scale, unfixed=None):
    op = oracle_problem(p); ols = op.linear_system(blockindices(p, unfixed)); c = ols.costgradhess()
    lam = ols.max_abs_diag() * lam_scale; assert ols.solve(lam) == 0
    return ols, c, lam


@pytest.mark.parametrize("name", list(CASES))
def test_structure_is_what_the_case_was_written_for(name):
    p, want, elim = case_problem(name)
    ols = oracle_problem(p).linear_system(blockindices(p))
    assert ols.info.is_sparse == 1
    got = structure_counts(p, ols, elim)
    print(f"STRUCTURE {name}: ndof={ols.info.ndof} blocks={ols.info.nblocks} {got}")
    assert got["independent"] and got["nelim"] == want["nelim"] and got["nreduced_dof"] == want["nred"]
    assert got["reduced_sizes"] == want["sizes"][1]
    if want["nelim"] == 0:
        assert name in NO_SCHUR
        return
    assert 2 * got["nelim"] >= ols.info.nblocks and got["elim_sizes"] == [want["sizes"][0]]
    assert got["reduced_reduced"] == want["rr"]
    assert (got["mixed_slots"] > 0) == want["mixed"], got
    if "elim_slots" in want: assert got["elim_slots"] == want["elim_slots"]
    if name in SCALAR_SCHUR:
        assert got["elim_unary"] == got["nelim"]                            # a unary group lies on the eliminated variables beside the coupling group
        q = CASES[name][0](mix_slots=False); oq = oracle_problem(q).linear_system(blockindices(q))
        assert np.array_equal(expected_elimination(oq), elim)               # (the orientation of an edge does not change the graph)
        assert structure_counts(q, oq, elim)["mixed_slots"] == 0            # the switch the regression check of notes/r11.md turns
        gB = next(iter(q.costs.values())); assert np.array_equal(greedy_independent_set(q.nvariables, gB.arrays()[0] - 1), elim)


def test_mixed_size_components():
    for name in ("mixed-linear3", "mixed-cost3"):
        p, _, elim = case_problem(name)
        assert elim[12:162].all() and not elim[:12].any() and not elim[162:].any()          # the points; cameras and the scalar chain stay
        assert structure_counts(p, oracle_problem(p).linear_system(blockindices(p)), elim)["elim_unary"] == 50
    p, _, elim = case_problem("mixed-adaptive_mean")
    assert elim[162] and not elim[163:].any()                                               # the ContaminatedGaussian variable is taken, its two means are not
    for name, kind in (("many_cameras-affine", 1), ("many_cameras-so3", 5)):
        p, _, elim = case_problem(name)
        assert elim[:120].all() and not elim[120:].any() and np.all(p.var_kind[:120] == kind)


def test_heavy_leaf_keeps_the_structure():
    """the optimizesingles case: leaf 0 of the shared-leaves graph with 66 coupling blocks on its three stored blocks (and its unary block): the same graph"""
    e, n = shared_leaves_edges(20, 120, heavy=21); p = scalar_graph_problem(e, n, seed=5)
    ols = oracle_problem(p).linear_system(blockindices(p)); elim = expected_elimination(ols)
    assert np.array_equal(elim, case_problem("shared_leaves-20")[2])
    cptr, _, _, cslot = p.costlists(np.nonzero(elim)[0] + 1)
    assert cptr[1] - cptr[0] == 67 and set(cslot[cptr[0]:cptr[1]].tolist()) == {0, 1} and np.all(np.diff(cptr)[1:] == 4)


@pytest.mark.parametrize("fixed", [False, True], ids=["free", "two_fixed"])
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_step_against_the_long_double_schur_step(name, fixed):
    p, want, _ = case_problem(name); unfixed = fixed_pair(name) if fixed else None
    ols, _, lam = _linearise(p, 1e-6, unfixed)
    elim = expected_elimination(ols)
    if fixed and want["nelim"]: assert elim.sum() >= want["nelim"] - 1 - (name.startswith("chain") or name.startswith("hub"))
    x_ref, _ = longdouble_schur_step(ols.data, ols.bsm_index(), ols.b, lam, elim)
    err = float(np.max(np.abs(ols.x - x_ref)) / np.max(np.abs(x_ref)))
    print(f"STEP {name} fixed={fixed}: eliminated {int(elim.sum())} of {ols.info.nblocks}, oracle step against the long-double Schur step {err:.2e}")
    assert err <= STEP_BOUND, err


@pytest.mark.parametrize("name,order", [(n, o) for n in CASES for o in ORDERS[1:] if not (n in NO_SCHUR and o == "elim_first")])      # (nothing eliminated: elim_first is the identity)
def test_oracle_is_indifferent_to_the_variable_order(name, order):
    p, want, elim = case_problem(name); lam_scale = 1e-6
    perm = case_order(order, elim); q, new_of_old = permute_variables(p, perm)
    assert not np.array_equal(perm, np.arange(p.nvariables))
    storage, dof = variable_sizes(p)
    assert np.array_equal(to_original_order(q.variables, storage, new_of_old), p.variables)
    ols0, c0, lam0 = _linearise(p, lam_scale); ols1, c1, lam1 = _linearise(q, lam_scale)
    assert np.isclose(c1, c0, rtol=1e-14, atol=0) and np.isclose(lam1, lam0, rtol=1e-14, atol=0)
    g1 = to_original_order(ols1.b, dof, new_of_old); x1 = to_original_order(ols1.x, dof, new_of_old)
    assert np.max(np.abs(g1 - ols0.b)) <= 1e-13 * np.max(np.abs(ols0.b))
    n = ols0.info.ndof
    H = bsm_to_csr(ols0.bsm_index(), ols0.data, n).toarray() + lam0 * np.eye(n)
    bound = max(1e-12, 1e2 * U * np.linalg.cond(H)); err = np.max(np.abs(x1 - ols0.x)) / np.max(np.abs(ols0.x))
    print(f"ORDER {name} {order}: step difference {err:.2e} (bound {bound:.2e}); eliminated in this order {int(expected_elimination(ols1).sum())}")
    assert err <= bound, (err, bound)
