"""The extended-precision references of tests/helpers.py (the backward error and the long-double Schur step that tests/test_gpu_mf_shapes.py holds the
matrix-free LM trial against) checked against the oracle's own damped solve, and shown able to fail; and the structure generator of those tests checked
on the CPU for every case they run."""
import numpy as np
import pytest

from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic
from tests.helpers import oracle_problem, blockindices, structured_problem, check_structure, longdouble_backward_error, longdouble_schur_step
from tests.test_gpu_mf_shapes import MF_CASES, SMALL_DAMPING, CALL_ORDER


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))


def _small_problems():
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(12, 150, 0.4, seed=3), 1e-3, 1e-3)
    yield "ba", p, np.r_[np.zeros(12, bool), np.ones(150, bool)]
    for ps in (1, 0):
        q, meta = structured_problem(K.RES_ROSENBROCK_B, [(7, 30), (3, 20), (12, 25)], 70, ps)
        yield f"rosenbrock_ps{ps}", q, meta["elim_blocks"]


@pytest.mark.parametrize("lam_scale", [1e-6, 1e-3])
def test_references_agree_with_the_oracle_solve(lam_scale):
    for name, p, elim in _small_problems():
        op = oracle_problem(p); ols = op.linear_system(blockindices(p)); ols.costgradhess()
        assert ols.info.is_sparse
        lam = ols.max_abs_diag() * lam_scale
        assert ols.solve(lam) == 0
        x = ols.x.copy()
        eta = longdouble_backward_error(ols.data, ols.bsm_index(), ols.b, lam, x)
        assert 0 < eta <= 1e-14, (name, eta)
        x_ref, S = longdouble_schur_step(ols.data, ols.bsm_index(), ols.b, lam, elim)
        assert rel(x, x_ref.astype(np.float64)) < 1e-10, (name, rel(x, x_ref.astype(np.float64)))
        assert longdouble_backward_error(ols.data, ols.bsm_index(), ols.b, lam, x_ref.astype(np.float64)) <= 1e-15, name
        assert S.shape[0] == int(np.sum(~elim) * (6 if name == "ba" else 1))


def test_backward_error_sees_one_perturbed_entry():
    """One entry of H 1e-8 off (relative) in the system that is solved: the backward error against the true H rises past 1e-9 (the measure can fail),
    while against the system that was solved it stays at rounding."""
    for name, p, elim in _small_problems():
        op = oracle_problem(p); ols = op.linear_system(blockindices(p)); ols.costgradhess()
        lam = ols.max_abs_diag() * 1e-6; idx = ols.bsm_index()
        x_ref, _ = longdouble_schur_step(ols.data, idx, ols.b, lam, elim)
        # the diagonal entry with the largest |H_ii x_i| (entry (i, i) of a diagonal block at its nzval offset + i (1 + block size): column-major)
        cp, rv, nz, bo = (np.asarray(a, np.int64) for a in idx); bs = np.diff(np.r_[bo - 1, len(ols.b)])
        pos, dof = [], []
        for row in range(len(cp) - 1):
            q = next(q for q in range(cp[row] - 1, cp[row + 1] - 1) if rv[q] - 1 == row)
            pos += [nz[q] - 1 + i * (1 + bs[row]) for i in range(bs[row])]; dof += [bo[row] - 1 + i for i in range(bs[row])]
        pos, dof = np.asarray(pos), np.asarray(dof)
        k = pos[np.argmax(np.abs(ols.data[pos] * x_ref.astype(np.float64)[dof]))]
        bad = ols.data.copy(); bad[k] *= 1 + 1e-8
        x_bad, _ = longdouble_schur_step(bad, idx, ols.b, lam, elim)
        x_bad = x_bad.astype(np.float64)
        eta = longdouble_backward_error(ols.data, idx, ols.b, lam, x_bad)
        assert eta > 1e-9, (name, eta)
        assert longdouble_backward_error(bad, idx, ols.b, lam, x_bad) <= 1e-15, name


@pytest.mark.parametrize("case", list(MF_CASES) + list(SMALL_DAMPING) + [CALL_ORDER + (True,)], ids=lambda c: c[0])
def test_generated_structures_are_the_intended_ones(case):
    """Before any GPU run: every structure tests/test_gpu_mf_shapes.py uploads, as the oracle's linear system stores it, is the one the case names."""
    name, kind, runs, nred, ps, _ = case
    p, meta = structured_problem(kind, runs, nred, ps)
    ols = oracle_problem(p).linear_system(blockindices(p))
    check_structure(ols, meta)
    expect = sum(-(-m // 128) for _, m in runs)                    # (one supernode per run, cut at 128 members) -- plus the generator's added runs
    assert meta["supernodes"] >= expect
    dv = 3 if kind == K.RES_BA_AFFINE else 1
    assert ols.info.ndof - dv * int(meta["elim_blocks"].sum()) >= 64          # (the reduced system is not the small dense one)
