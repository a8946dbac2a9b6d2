"""The order the caller lists the variables in must not matter: the reference's LDL' orders itself (src/linearsystem.jl:52,68), and the CPU oracle restates
the reference.  This pins tests/helpers.permute_variables and its named orders on the CPU: the permuted problem is the same problem (variables, kinds, cost
blocks), and the oracle's cost and damped step, mapped back, are the identity order's.  tests/test_gpu_variable_order.py then runs the device code, which DOES
branch on the order, on the same inputs."""
import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import synthetic
from tests.helpers import (oracle_problem, blockindices, bsm_to_csr, permute_variables, to_original_order, variable_sizes, eliminated_mask, NAMED_ORDERS,
                           order_var_last, order_var_middle)

U = np.finfo(np.float64).eps / 2


def ba_affine():
    return synthetic.perturb_ba_problem(synthetic.create_ba_problem(12, 80, 0.3, seed=5, robust=N.HuberKernel(0.05), outlier_frac=0.1, outlier_sigma=0.05), 1e-3, 1e-3), 1e-6


def so3_adaptive():
    return synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(8, 60, 0.5, seed=2, adaptive=True), 1e-3, 1e-3), 1e-4


ORDERS = dict(NAMED_ORDERS, kernel_last=order_var_last(0), kernel_middle=order_var_middle(0))
CASES = [("ba_affine", ba_affine, o) for o in NAMED_ORDERS] + [("so3_adaptive", so3_adaptive, o) for o in ORDERS]


def _linearise(p, lam_scale):
    op = oracle_problem(p); ols = op.linear_system(blockindices(p)); c = ols.costgradhess()
    lam = ols.max_abs_diag() * lam_scale; assert ols.solve(lam) == 0
    return op, ols, c, lam


@pytest.mark.parametrize("name,make,order", CASES, ids=[f"{c[0]}-{c[2]}" for c in CASES])
def test_oracle_is_indifferent_to_the_variable_order(name, make, order):
    p, lam_scale = make()
    perm = ORDERS[order](eliminated_mask(p))
    q, new_of_old = permute_variables(p, perm)
    # the helper itself: the same variables and cost blocks under new numbers
    assert np.array_equal(new_of_old[perm], np.arange(p.nvariables))
    if order == "identity": assert np.array_equal(perm, np.arange(p.nvariables))
    else: assert not np.array_equal(perm, np.arange(p.nvariables))
    storage, dof = variable_sizes(p)
    assert np.array_equal(to_original_order(q.variables, storage, new_of_old), p.variables)
    assert np.array_equal(q.var_kind[new_of_old], p.var_kind) and np.array_equal(q.var_dim[new_of_old], p.var_dim)
    for gp, gq in zip(p.groups(), q.groups()):
        assert gp["res_kind"] == gq["res_kind"] and gp["robust_kind"] == gq["robust_kind"] and np.array_equal(gp["robust_params"], gq["robust_params"])
        assert np.array_equal(gq["varind"], new_of_old[gp["varind"] - 1] + 1) and np.array_equal(gp["data"], gq["data"])
    # the oracle: cost (the blocks are summed in the same order: rounding of the blocks' own arithmetic at most), gradient and damped step mapped back
    _, ols0, c0, lam0 = _linearise(p, lam_scale)
    _, ols1, c1, lam1 = _linearise(q, lam_scale)
    assert np.isclose(c1, c0, rtol=1e-14, atol=0) and np.isclose(lam1, lam0, rtol=1e-14, atol=0)
    g1 = to_original_order(ols1.b, dof, new_of_old); x1 = to_original_order(ols1.x, dof, new_of_old)
    assert np.max(np.abs(g1 - ols0.b)) <= 1e-13 * np.max(np.abs(ols0.b))
    # two backward-stable solves of one system, eliminated in different orders, differ by u x cond(H + lam I) (the bound of tests/test_gpu_mf_shapes.py)
    n = ols0.info.ndof
    H = bsm_to_csr(ols0.bsm_index(), ols0.data, n).toarray() + lam0 * np.eye(n)
    bound = max(1e-12, 1e2 * U * np.linalg.cond(H))
    err = np.max(np.abs(x1 - ols0.x)) / np.max(np.abs(ols0.x))
    print(f"ORDER {name} {order}: cost {c1:.16e} step difference {err:.2e} (bound {bound:.2e})")
    assert err <= bound, (err, bound)
