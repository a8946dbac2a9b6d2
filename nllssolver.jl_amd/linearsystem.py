"""MultiVariateLSgpu: the device-resident linear system that replaces MultiVariateLSsparse /
MultiVariateLSdense (src/linearsystem.jl:44-87) behind the same generic functions the iterators call
(SURVEY.md 8b).  All arithmetic happens in csrc/libnlls_amd.so; this class only forwards.
"""
import numpy as np

from . import _capi
from ._capi import VARS_CURRENT, VARS_NEXT, VARS_BEST


class MultiVariateLSgpu:
    def __init__(self, problem, unfixed, flags=0, device=0, stream=None):
        unfixed = np.asarray(unfixed, dtype=bool)
        assert unfixed.size == problem.nvariables
        # blockindices: linearsystem.jl:93-102
        self.blockindices = np.zeros(problem.nvariables, np.uint64)
        self.blockindices[unfixed] = np.arange(1, int(unfixed.sum()) + 1, dtype=np.uint64)
        self.ctx = self._make_context(device)
        if stream is not None:
            self.ctx.set_stream(stream)
        self.info = self.ctx.upload(problem.var_kind, problem.var_dim, self.blockindices, problem.groups(), flags)
        self.ctx.set_variables(problem.variables, VARS_CURRENT)
        self.ctx.copy_variables(VARS_NEXT, VARS_CURRENT)        # setupiterator: varnext = deepcopy(variables)
        self._x = None

    def _make_context(self, device):
        return _capi.Context(device)

    # ---- the generic functions of SURVEY 8b -------------------------------------------------------
    def costgradhess(self, want_cost=True):
        """zero!(linsystem); costgradhess!(linsystem, vars, costs)   src/optimize.jl:118,167-170.
        want_cost=False (the outer loop between iterations discards the value): enqueue only."""
        self._x = None
        return self.ctx.sweep_gradhess(want_cost)

    def cost(self, which=VARS_NEXT):
        """cost(vars, costs)   src/cost.jl:10-13"""
        return self.ctx.sweep_cost(which)

    def eval_blocks(self, group, which=VARS_CURRENT, want=("r", "sqerr", "rho", "weight")):
        """computeresidual / r'r / robustify / rho' of every block of a cost group, in the problem's order   src/NLLSsolver.jl:16, src/residual.jl:52"""
        return self.ctx.eval_blocks(group, which, want)

    def eval_jacobians(self, group, which=VARS_CURRENT, index=None, want=("r", "J")):
        """computeresjac of blocks of a cost group, every variable free (index 1-based, None: all; nlls_eval_jacobians)   src/autodiff.jl:78-93"""
        return self.ctx.eval_jacobians(group, which, index, want)

    def eval_gradhess(self, group, which=VARS_CURRENT, index=None, want=("cost", "g", "H")):
        """computecostgradhess of blocks of a cost group, every variable free (index 1-based, None: all; nlls_eval_gradhess)   src/residual.jl:57-111"""
        return self.ctx.eval_gradhess(group, which, index, want)

    def hess_apply(self, v, lam=0.0, which=VARS_CURRENT):
        """(hessian + lam I) * v without A.data (nlls_hess_apply)   src/linearsystem.jl:180-190, src/iterators.jl:47-115, src/utils.jl:71-106"""
        return self.ctx.hess_apply(v, lam, which)

    def jac_apply(self, group, v, which=VARS_CURRENT):
        """J v per block of a cost group (nlls_jac_apply)"""
        return self.ctx.jac_apply(group, v, which)

    def jact_apply(self, group, u, which=VARS_CURRENT):
        """J' u of a cost group's blocks (nlls_jact_apply)"""
        return self.ctx.jact_apply(group, u, which)

    def hess_block_diag(self, lam=0.0, which=VARS_CURRENT):
        """the diagonal blocks of hessian + lam I (nlls_hess_block_diag)   src/BlockSparseMatrix.jl:83-99"""
        return self.ctx.hess_block_diag(lam, which)

    def adaptive_em(self, kernel_var=1, which=VARS_NEXT, maxiters=10):
        """optimize(kernel::ContaminatedGaussian, squarederrors, maxiters)   src/robustadaptive.jl:48-73"""
        return self.ctx.adaptive_em(kernel_var, which, maxiters)

    def set_cost_data(self, group, data, index=None):
        """new measurements for blocks of a cost group on the uploaded structure (index 1-based; nlls_set_cost_data)   the reference's mutable costs, src/optimize.jl:5-17"""
        self._x = None; self.ctx.set_cost_data(group, data, index)

    def set_robust_params(self, group, params):
        """new parameters for a cost group's robust kernel (nlls_set_robust_params)"""
        self._x = None; self.ctx.set_robust_params(group, params)

    def uniformscaling(self, k):
        """uniformscaling!(hessian, k)   src/iterators.jl:149,162"""
        self.ctx.damp(k)

    def solve(self):
        """negate!(solve!(linsystem, options))   src/iterators.jl:152"""
        self._x = None
        self.ctx.solve()

    def solve_pcg(self, precond="blockjacobi", maxiters=None, rtol=1e-8, want_x=False):
        """solve by conjugate gradients on the matrix-free operator, where solve() factors (nlls_solve_pcg) -> (x or None, stats); maxiters None: 4 ndof"""
        self._x = None
        return self.ctx.solve_pcg(precond, maxiters, rtol, want_x)

    def solve_pcg_schur(self, precond="blockjacobi", maxiters=None, rtol=1e-8, want_x=False):
        """solve_pcg on the reduced system of the upload's eliminated set (nlls_solve_pcg_schur) -> (x or None, stats)   src/linearsolver.jl:20-32"""
        self._x = None
        return self.ctx.solve_pcg_schur(precond, maxiters, rtol, want_x)

    def solve_pcg_tr(self, radius, precond="blockjacobi", maxiters=None, rtol=1e-8, want_x=False):
        """solve_pcg inside the trust region ||y||_M <= radius, M the preconditioner (Steihaug-Toint; nlls_solve_pcg_tr) -> (x or None, stats with mnorm and model)
        in the place of the dogleg iterator's Cauchy point plus Gauss-Newton solve   src/iterators.jl:47-115"""
        self._x = None
        return self.ctx.solve_pcg_tr(radius, precond, maxiters, rtol, want_x)

    def schur_info(self):
        """(nred, nelim, is_elim per unfixed block, positions of the reduced unknowns in the gradient) (nlls_schur_info)"""
        return self.ctx.schur_info()

    def schur_apply(self, v, lam=0.0, which=VARS_CURRENT):
        """S(lam) v, S = B + lam I - E (C + lam I)^-1 E', never formed (nlls_schur_apply)"""
        return self.ctx.schur_apply(v, lam, which)

    def schur_block_diag(self, lam=0.0, which=VARS_CURRENT):
        """the diagonal blocks of S(lam), one per reduced block, unfactored (nlls_schur_block_diag)"""
        return self.ctx.schur_block_diag(lam, which)

    def schur_reduce(self, b, lam=0.0, which=VARS_CURRENT):
        """b_r - E (C + lam I)^-1 b_e (nlls_schur_reduce)"""
        return self.ctx.schur_reduce(b, lam, which)

    def schur_expand(self, b, yr, lam=0.0, which=VARS_CURRENT):
        """yr on the reduced entries, (C + lam I)^-1 (b_e - E' yr) on the eliminated ones (nlls_schur_expand)"""
        return self.ctx.schur_expand(b, yr, lam, which)

    def solve_pcg_rhs(self, B, lam=0.0, which=VARS_CURRENT, precond="blockjacobi", maxiters=None, rtol=1e-8):
        """(hessian + lam I) x_k = b_k for right-hand sides of the caller's, eight at a time on the device (nlls_solve_pcg_rhs) -> (X, stats); the linear system is
        left as it is   src/linearsolver.jl:20-32"""
        return self.ctx.solve_pcg_rhs(B, lam, which, precond, maxiters, rtol)

    def marginal_cov(self, varindices, lam=0.0, which=VARS_CURRENT, precond="blockjacobi", maxiters=None, rtol=1e-8):
        """the block of (hessian + lam I)^-1 of the listed variables (1-based, unfixed; nlls_marginal_cov) -> (cov, stats); the reference has no such routine"""
        return self.ctx.marginal_cov(varindices, lam, which, precond, maxiters, rtol)

    def lm_trial(self, dlambda):
        """uniformscaling!(H, dlambda); solve!; update!(next, current); cost(next)   src/iterators.jl:149-157, fused
        into one call of the library (one synchronisation).  Returns the trial cost."""
        self._x = None
        return self.ctx.lm_trial(dlambda, VARS_NEXT, VARS_CURRENT)

    def update(self, to=VARS_NEXT, frm=VARS_CURRENT):
        """update!(to, from, linsystem)   src/linearsystem.jl:206-213"""
        self.ctx.retract(to, frm)

    def initlambda(self):
        """src/iterators.jl:131-137"""
        return self.ctx.max_abs_diag() * 1e-6

    def quadform(self):
        """(fast_bAb(hessian, x), dot(gradient, x))   src/iterators.jl:163"""
        return self.ctx.quadform()

    def grad_quadform(self):
        """fast_bAb(hessian, gradient)   src/iterators.jl:52"""
        return self.ctx.grad_quadform()

    def step_maxabs(self):
        return self.ctx.step_maxabs()

    def step_norm(self):
        return self.ctx.step_norm()

    @property
    def x(self):
        """linsystem.x, fetched lazily (callbacks read it: src/callbacks.jl:47,105)"""
        if self._x is None:
            self._x = self.ctx.get_step()
        return self._x

    @x.setter
    def x(self, value):
        self._x = np.array(value, dtype=np.float64)
        self.ctx.set_step(self._x)

    @property
    def b(self):
        return self.ctx.get_grad()

    def swap(self, a, b):
        self.ctx.swap_variables(a, b)

    def copy(self, dst, src):
        self.ctx.copy_variables(dst, src)

    def variables(self, which=VARS_CURRENT):
        return self.ctx.get_variables(which)

    def close(self):
        self.ctx.close()


def makesymmvls(problem, unfixed, flags=0, device=0, stream=None):
    """makesymmvls(problem, unfixed, nblocks)   src/linearsystem.jl:91-124"""
    return MultiVariateLSgpu(problem, unfixed, flags, device, stream)
