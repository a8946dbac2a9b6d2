"""The cases of tests/sweep_cases.py without a GPU: the CPU oracle's costgradhess() equals the integer reference bit for bit at both variable sets -- so the reference,
not the kernel under test, defines the bits tests/test_gpu_sweep_exact.py asks for -- and every case's edge predicate holds on the restated tile loop."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import sweep_cases as S


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", list(S.CASES))
def test_oracle_equals_integer_reference(name):
    case = S.CASES[name](); sp = case.sp
    op, ols = sp.oracle()
    for v in (sp.variables, sp.variables2):
        A, b, cost = S.exact_system(sp, variables=v)
        op.set_variables(v)
        c_ora = ols.costgradhess(); A_ora = ols.data.copy()
        if not ols.info.is_sparse: A_ora = S.mirror_dense(A_ora, ols.info.ndof)
        assert np.array_equal(bits(A_ora), bits(A)) and np.array_equal(bits(ols.b), bits(b))
        assert c_ora == cost and op.cost() == cost
    op.set_variables(sp.variables)
    A1, b1, c1 = S.exact_system(sp); A2, b2, c2 = S.exact_system(sp, variables=sp.variables2)
    nz = A1 != 0                                             # (structural zeros of J'J stay; a few products coincide by chance)
    assert np.count_nonzero(A1[nz] != A2[nz]) >= 0.9 * np.count_nonzero(nz), "the second variable set does not move the entries"
    assert np.count_nonzero(b1 != b2) >= 0.9 * b1.size and c1 != c2


@pytest.mark.parametrize("name", list(S.CASES))
def test_edge_predicate(name):
    case = S.CASES[name]()
    t = case.assert_edge()
    print(f"EDGE {name}: sparse={t['sparse']} " + " ".join(f"{k[6:]}={v}" for k, v in t["counters"].items()) + f" costs={sum(len(g['varind']) for g in case.sp.groups)} env={case.env}")


def test_sums_do_not_depend_on_the_order():
    """the premise: a random permutation of the costs leaves the oracle's bits unchanged (3 cameras x 1100 points)"""
    inc = S.rows_of((1100, 1100, 1100)); sp = S.dyadic_ba(inc)
    A, b, cost = S.exact_system(sp)
    g = sp.groups[0]; o = np.random.default_rng(1).permutation(len(inc))
    op = O.OracleProblem(sp.var_kind, sp.var_dim, [dict(g, varind=g["varind"][o], data=g["data"][o])]); op.set_variables(sp.variables)
    ols = op.linear_system(sp.bi); c = ols.costgradhess()
    assert c == cost and np.array_equal(bits(ols.data), bits(A)) and np.array_equal(bits(ols.b), bits(b))
    assert np.array_equal(A * 65536, np.rint(A * 65536)) and np.abs(A).max() * 65536 < 2 ** 53
