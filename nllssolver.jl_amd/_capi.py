"""ctypes binding of csrc/libnlls_amd.so (the C ABI of include/nlls_amd.h).

The product path has NO CPU fallback: if the shared library is missing, or no gfx950 device is
visible, every compute entry point raises NllsError.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# NLLS_AMD_LIB: another build of the library -- one with USER residual kinds (include/nlls_amd.h, NLLS_RES_USER0 .. 7; the Julia shim reads the same variable)
LIB_PATH = os.environ.get("NLLS_AMD_LIB") or os.path.join(_HERE, "csrc", "libnlls_amd.so")

OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_NOT_READY, ERR_NOT_SPD, ERR_NO_DEVICE = 0, -1, -2, -3, -4, -5, -6
FLAG_FORCE_ATOMIC, FLAG_NO_SCHUR, FLAG_FORCE_SPARSE, FLAG_NO_BAND, FLAG_NO_TWIST, FLAG_NO_BCR, FLAG_DETERMINISTIC = 1, 2, 4, 8, 16, 32, 64
FLAG_PRESHARDED = 128
FLAG_NO_REORDER = 256
FLAG_NO_TILE_SPARSE = 512
FLAG_NO_PIVOT_FLOOR = 1024
FLAG_MATERIALIZE = 2048
OPT_MATERIALIZE, OPT_LOOKAHEAD, OPT_PHASE_EVENTS = 1, 2, 3
OPT_APPLY_SCRATCH, OPT_APPLY_WAVE_MIN = 4, 5
OPT_PCG_ROUND, OPT_PCG_GRID_MAX = 6, 7
PCG_PRECOND_NONE, PCG_PRECOND_BLOCK_JACOBI, PCG_PRECOND_SCHUR_JACOBI = 0, 1, 3      # (2 is unassigned: every entry point refuses it)
PCG_PRECONDS = {"none": PCG_PRECOND_NONE, None: PCG_PRECOND_NONE, "blockjacobi": PCG_PRECOND_BLOCK_JACOBI, "schurjacobi": PCG_PRECOND_SCHUR_JACOBI}
PCG_STATUS = {0: "converged", 1: "maxiters", 2: "breakdown", 3: "preconditioner not positive definite", 4: "trust-region boundary", 5: "non-positive curvature, to the boundary"}
APPLY_MAX_VEC = 8
VARS_CURRENT, VARS_NEXT, VARS_BEST = 0, 1, 2

# every symbol include/nlls_amd.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = """nlls_ctx_create nlls_ctx_destroy nlls_last_error nlls_set_stream nlls_set_shard nlls_var_storage nlls_var_dof nlls_robust_nparams nlls_robustify
nlls_res_ndeps nlls_res_nres nlls_res_ndata nlls_res_slot_kind nlls_rcm_order nlls_nd_tiles nlls_upload_structure nlls_get_info nlls_get_bsm_index
nlls_set_variables nlls_get_variables nlls_swap_variables nlls_copy_variables nlls_sweep_gradhess nlls_sweep_cost
nlls_get_grad nlls_get_bsm_data nlls_max_abs_diag nlls_grad_sqnorm nlls_grad_quadform nlls_damp nlls_solve nlls_get_solve_stats nlls_set_step
nlls_get_step nlls_step_maxabs nlls_step_norm nlls_quadform nlls_retract nlls_sweep_gradhess_local
nlls_sweep_gradhess_finish nlls_sweep_cost_local nlls_sweep_cost_finish nlls_solve_local nlls_solve_finish
nlls_get_reduce_buffer nlls_get_step_shard nlls_get_shard_info nlls_get_grad_owned nlls_trial_local nlls_solve_finish_async nlls_lm_trial nlls_optimize_singles nlls_time_sweep_gradhess nlls_time_sweep_accumulate nlls_time_sweep_cost nlls_time_solve nlls_time_reduced_solve nlls_profile_sweep nlls_profile_sweep_dispatch nlls_solve_finish_replicated nlls_get_variables_owned nlls_lm_iterations
nlls_set_allreduce nlls_comm_unique_id nlls_comm_init_rccl nlls_comm_post_flag nlls_comm_agreed_flag nlls_comm_info nlls_get_memory_info nlls_flush_cache nlls_check_analytic nlls_set_option nlls_get_time_buckets nlls_get_phase_times
nlls_eval_blocks nlls_adaptive_em nlls_set_cost_data nlls_set_robust_params
nlls_eval_jacobians nlls_eval_gradhess nlls_res_jac_cols nlls_res_gh_dim
nlls_hess_apply nlls_jac_apply nlls_jact_apply nlls_hess_block_diag nlls_solve_pcg nlls_solve_pcg_rhs nlls_marginal_cov
nlls_schur_info nlls_schur_apply nlls_schur_reduce nlls_schur_expand nlls_solve_pcg_schur nlls_solve_pcg_tr nlls_schur_block_diag""".split()


class LmOptions(C.Structure):          # nlls_lm_options
    _fields_ = [("reldcost", C.c_double), ("absdcost", C.c_double), ("dstep", C.c_double), ("maxfails", C.c_int64), ("maxiters", C.c_int64),
                ("stoptime_ns", C.c_int64)]


class LmState(C.Structure):            # nlls_lm_state
    _fields_ = [("lambda_", C.c_double), ("bestcost", C.c_double), ("cost", C.c_double), ("iternum", C.c_int64), ("fails", C.c_int64),
                ("have_best", C.c_int64), ("converged", C.c_int64), ("linearsolvers", C.c_int64), ("costcomputations", C.c_int64),
                ("gradientcomputations", C.c_int64), ("singulartrials", C.c_int64), ("timesolver_ns", C.c_int64), ("timegradient_ns", C.c_int64), ("timecost_ns", C.c_int64)]


class NllsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"nlls_amd error {code}: {msg}")
        self.code = code


class CostGroup(C.Structure):
    _fields_ = [("res_kind", C.c_int32), ("robust_kind", C.c_int32), ("robust_params", C.c_double * 4),
                ("ncost", C.c_int64), ("varind", C.c_void_p), ("data", C.c_void_p)]


class Info(C.Structure):
    _fields_ = [("is_sparse", C.c_int32), ("has_schur", C.c_int32), ("nvar", C.c_int64), ("nblocks", C.c_int64),
                ("ndof", C.c_int64), ("nnz_data", C.c_int64), ("nblocks_stored", C.c_int64), ("ncost", C.c_int64),
                ("var_storage", C.c_int64), ("nschur_blocks", C.c_int64), ("nreduced_dof", C.c_int64),
                ("owner_path", C.c_int64), ("solve_mode", C.c_int64), ("bandwidth", C.c_int64), ("nborder_dof", C.c_int64)]


def build(force=False):
    """Compile libnlls_amd.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-s", "-C", csrc, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", csrc, "libnlls_amd.so"])
    return LIB_PATH


_lib = None


def lib():
    """Load the shared library or fail loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NllsError(ERR_NO_DEVICE, f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C nllssolver.jl_amd/csrc); "
                                           "there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
        L.nlls_ctx_create.argtypes = [vp, i32, C.POINTER(vp)]
        L.nlls_ctx_destroy.argtypes = [vp]
        L.nlls_last_error.argtypes = [vp]; L.nlls_last_error.restype = C.c_char_p
        L.nlls_set_stream.argtypes = [vp, vp]
        L.nlls_set_shard.argtypes = [vp, i32, i32]
        L.nlls_var_storage.argtypes = [i32, i32]; L.nlls_var_dof.argtypes = [i32, i32]
        L.nlls_robust_nparams.argtypes = [i32]; L.nlls_robustify.argtypes = [vp, i32, vp, i64, vp, vp]
        L.nlls_res_ndeps.argtypes = [i32]; L.nlls_res_nres.argtypes = [i32]; L.nlls_res_ndata.argtypes = [i32]
        L.nlls_res_slot_kind.argtypes = [i32, i32, vp, vp]
        L.nlls_rcm_order.argtypes = [i32, vp, vp, vp]
        L.nlls_nd_tiles.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, i64, vp]
        L.nlls_upload_structure.argtypes = [vp, i64, vp, vp, vp, i32, vp, i32]
        L.nlls_get_info.argtypes = [vp, vp]
        L.nlls_lm_iterations.argtypes = [vp, vp, vp, i64]
        L.nlls_get_bsm_index.argtypes = [vp, vp, vp, vp, vp]
        L.nlls_set_variables.argtypes = [vp, i32, vp]; L.nlls_get_variables.argtypes = [vp, i32, vp]
        L.nlls_swap_variables.argtypes = [vp, i32, i32]; L.nlls_copy_variables.argtypes = [vp, i32, i32]
        L.nlls_sweep_gradhess.argtypes = [vp, vp]; L.nlls_sweep_cost.argtypes = [vp, i32, vp]
        L.nlls_get_grad.argtypes = [vp, vp]; L.nlls_get_bsm_data.argtypes = [vp, vp]; L.nlls_get_grad_owned.argtypes = [vp, vp]
        L.nlls_max_abs_diag.argtypes = [vp, vp]; L.nlls_grad_sqnorm.argtypes = [vp, vp]; L.nlls_grad_quadform.argtypes = [vp, vp]
        L.nlls_damp.argtypes = [vp, dbl]
        L.nlls_get_solve_stats.argtypes = [vp, vp, i32]
        L.nlls_solve.argtypes = [vp, vp]; L.nlls_set_step.argtypes = [vp, vp]; L.nlls_get_step.argtypes = [vp, vp]
        L.nlls_step_maxabs.argtypes = [vp, vp]; L.nlls_step_norm.argtypes = [vp, vp]
        L.nlls_quadform.argtypes = [vp, vp, vp]
        L.nlls_retract.argtypes = [vp, i32, i32]; L.nlls_lm_trial.argtypes = [vp, C.c_double, i32, i32, vp]
        L.nlls_optimize_singles.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, i32, i32, i32, C.c_double, C.c_double, C.c_double, vp]
        L.nlls_sweep_gradhess_local.argtypes = [vp]; L.nlls_sweep_gradhess_finish.argtypes = [vp, vp]
        L.nlls_sweep_cost_local.argtypes = [vp, i32]; L.nlls_sweep_cost_finish.argtypes = [vp, vp]
        L.nlls_solve_local.argtypes = [vp]; L.nlls_solve_finish.argtypes = [vp, vp]
        L.nlls_get_reduce_buffer.argtypes = [vp, i32, vp, vp]; L.nlls_trial_local.argtypes = [vp, i32, i32, vp]; L.nlls_solve_finish_async.argtypes = [vp]
        L.nlls_get_step_shard.argtypes = [vp, vp, vp, vp, vp]
        L.nlls_get_shard_info.argtypes = [vp, vp, i32]
        L.nlls_time_sweep_gradhess.argtypes = [vp, i32, vp]; L.nlls_time_sweep_cost.argtypes = [vp, i32, vp]; L.nlls_time_sweep_accumulate.argtypes = [vp, i32, vp]
        L.nlls_time_solve.argtypes = [vp, i32, vp]; L.nlls_time_reduced_solve.argtypes = [vp, i32, vp]
        L.nlls_profile_sweep.argtypes = [vp, i32, vp, vp, vp, vp]; L.nlls_profile_sweep_dispatch.argtypes = [vp, vp, vp, vp, vp]
        L.nlls_solve_finish_replicated.argtypes = [vp]; L.nlls_get_variables_owned.argtypes = [vp, i32, vp]
        L.nlls_set_allreduce.argtypes = [vp, vp, vp]; L.nlls_comm_unique_id.argtypes = [vp]; L.nlls_comm_init_rccl.argtypes = [vp, vp]
        L.nlls_get_memory_info.argtypes = [vp, vp, i32]; L.nlls_flush_cache.argtypes = [vp, i64]; L.nlls_check_analytic.argtypes = [vp, vp, i32]
        L.nlls_set_option.argtypes = [vp, i32, i64]; L.nlls_get_time_buckets.argtypes = [vp, vp, i32]; L.nlls_get_phase_times.argtypes = [vp, vp, i32]
        L.nlls_eval_blocks.argtypes = [vp, i32, i32, vp, vp, vp, vp]; L.nlls_adaptive_em.argtypes = [vp, i32, i64, i32, vp, vp]
        L.nlls_set_cost_data.argtypes = [vp, i32, i64, vp, vp]; L.nlls_set_robust_params.argtypes = [vp, i32, vp]
        L.nlls_eval_jacobians.argtypes = [vp, i32, i32, i64, vp, vp, vp]; L.nlls_eval_gradhess.argtypes = [vp, i32, i32, i64, vp, vp, vp, vp]
        L.nlls_res_jac_cols.argtypes = [i32]; L.nlls_res_gh_dim.argtypes = [i32]
        L.nlls_hess_apply.argtypes = [vp, i32, dbl, i32, vp, vp]; L.nlls_jac_apply.argtypes = [vp, i32, i32, i32, vp, vp]
        L.nlls_jact_apply.argtypes = [vp, i32, i32, i32, vp, vp]; L.nlls_hess_block_diag.argtypes = [vp, i32, dbl, vp]
        L.nlls_solve_pcg.argtypes = [vp, i32, i32, dbl, vp, vp]
        L.nlls_solve_pcg_rhs.argtypes = [vp, i32, dbl, i32, i32, dbl, i32, vp, vp, vp]; L.nlls_marginal_cov.argtypes = [vp, i32, dbl, i64, vp, i32, i32, dbl, vp, vp]
        L.nlls_schur_info.argtypes = [vp, vp, vp, vp]; L.nlls_schur_apply.argtypes = [vp, i32, dbl, i32, vp, vp]; L.nlls_schur_reduce.argtypes = [vp, i32, dbl, i32, vp, vp]
        L.nlls_schur_expand.argtypes = [vp, i32, dbl, i32, vp, vp, vp]; L.nlls_solve_pcg_schur.argtypes = [vp, i32, i32, dbl, vp, vp]
        L.nlls_schur_block_diag.argtypes = [vp, i32, dbl, vp]
        L.nlls_solve_pcg_tr.argtypes = [vp, i32, i32, dbl, dbl, vp, vp]
        L.nlls_comm_post_flag.argtypes = [vp, dbl]; L.nlls_comm_agreed_flag.argtypes = [vp, dbl, vp]; L.nlls_comm_info.argtypes = [vp, vp, i32]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """Owns one nlls_ctx."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        dev = np.array([device], np.int32)
        rc = self.L.nlls_ctx_create(_p(dev), 1, C.byref(self.h))
        if rc != OK:
            self.h = None
            raise NllsError(rc, "nlls_ctx_create failed: no gfx950 (MI355X) device visible -- there is no CPU fallback"
                            if rc == ERR_NO_DEVICE else "nlls_ctx_create failed")
        self.info = None
        self._keep = None
        self._groups = []
        self._ndata = []

    def close(self):
        if getattr(self, "h", None):
            self.L.nlls_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            exc = getattr(self, "_reduce_exc", None)
            if exc is not None:             # the installed all-reduce raised inside the library's call: that exception is the cause, not "all-reduce failed"
                self._reduce_exc = None
                raise NllsError(rc, self.L.nlls_last_error(self.h).decode() + f" ({type(exc).__name__}: {exc})") from exc
            raise NllsError(rc, self.L.nlls_last_error(self.h).decode())
        return rc

    def set_stream(self, stream_ptr):
        self._chk(self.L.nlls_set_stream(self.h, C.c_void_p(stream_ptr)))

    def upload(self, var_kind, var_dim, blockindices, groups, flags=0):
        """nlls_upload_structure; groups = list of dicts as produced by NLLSProblem.groups()."""
        vk = np.ascontiguousarray(var_kind, np.int32); vd = np.ascontiguousarray(var_dim, np.int32)
        bi = np.ascontiguousarray(blockindices, np.uint64)
        arr = (CostGroup * max(len(groups), 1))()
        keep = [vk, vd, bi]
        for i, g in enumerate(groups):
            vi = np.ascontiguousarray(g["varind"], np.int64); da = np.ascontiguousarray(g["data"], np.float64)
            keep += [vi, da]
            arr[i].res_kind = int(g["res_kind"]); arr[i].robust_kind = int(g.get("robust_kind", 0))
            rp = list(g.get("robust_params", ())) + [0.0] * 4
            for k in range(4):
                arr[i].robust_params[k] = float(rp[k])
            arr[i].ncost = vi.shape[0]; arr[i].varind = vi.ctypes.data; arr[i].data = da.ctypes.data
        self._var_kind, self._var_dim = vk, vd                   # (marginal_cov: the dof of the listed variables)
        self._nred_of_upload = None
        self._kinds = [int(g["res_kind"]) for g in groups]      # (eval_jacobians / eval_gradhess: the record sizes of a group's kind)
        self._groups = []; self._ndata = [int(da.size // max(vi.shape[0], 1)) for vi, da in zip(keep[3::2], keep[4::2])]     # doubles of payload per block, per group (set_cost_data)
        self._chk(self.L.nlls_upload_structure(self.h, len(vk), _p(vk), _p(vd), _p(bi), len(groups), arr, flags))
        for i, g in enumerate(groups):             # (ncost, residuals per block) of every group, for eval_blocks; a dynamic kind's nres is its variable's run-time length
            nres = self.L.nlls_res_nres(int(g["res_kind"]))
            if nres < 0 and arr[i].ncost:
                nres = int(vd[int(np.asarray(g["varind"]).reshape(arr[i].ncost, -1)[0, 0]) - 1])
            self._groups.append((int(arr[i].ncost), max(int(nres), 1)))
        self.info = Info()
        self._chk(self.L.nlls_get_info(self.h, C.byref(self.info)))
        return self.info

    def bsm_index(self):
        nb, ns = self.info.nblocks, self.info.nblocks_stored
        cp = np.zeros(nb + 1, np.int64); rv = np.zeros(max(ns, 1), np.int64); nz = np.zeros(max(ns, 1), np.int64)
        bo = np.zeros(max(nb, 1), np.int64)
        self._chk(self.L.nlls_get_bsm_index(self.h, _p(cp), _p(rv), _p(nz), _p(bo)))
        return cp, rv[:ns], nz[:ns], bo[:nb]

    def set_variables(self, packed, which=VARS_CURRENT):
        packed = np.ascontiguousarray(packed, np.float64)
        assert packed.size == self.info.var_storage
        self._chk(self.L.nlls_set_variables(self.h, which, _p(packed)))

    def get_variables(self, which=VARS_CURRENT):
        out = np.zeros(self.info.var_storage)
        self._chk(self.L.nlls_get_variables(self.h, which, _p(out)))
        return out

    def swap_variables(self, a, b):
        self._chk(self.L.nlls_swap_variables(self.h, a, b))

    def copy_variables(self, dst, src):
        self._chk(self.L.nlls_copy_variables(self.h, dst, src))

    def _scalar(self, fn, *args):
        out = C.c_double()
        self._chk(fn(self.h, *args, C.byref(out)))
        return out.value

    def sweep_gradhess(self, want_cost=True):
        if not want_cost:                          # enqueue only: no cost reduction, no synchronisation
            self._chk(self.L.nlls_sweep_gradhess(self.h, None)); return None
        return self._scalar(self.L.nlls_sweep_gradhess)

    def sweep_cost(self, which=VARS_CURRENT):
        return self._scalar(self.L.nlls_sweep_cost, which)

    def eval_blocks(self, group, which=VARS_CURRENT, want=("r", "sqerr", "rho", "weight")):
        """nlls_eval_blocks: the blocks of cost group `group` (0-based, upload order) at variable set `which` -- a dict with the entries of `want`:
        "r" (ncost x nres) computeresidual, "sqerr" r'r, "rho" robustify(kernel, r'r), "weight" rho' (the IRLS weight)."""
        want = (want,) if isinstance(want, str) else tuple(want)
        assert want and set(want) <= {"r", "sqerr", "rho", "weight"}
        g = self._groups[group] if 0 <= group < len(self._groups) else None
        n, nres = (g if g is not None else (0, 1))
        out = {k: np.zeros((n, nres) if k == "r" else n) for k in want}
        self._chk(self.L.nlls_eval_blocks(self.h, int(which), int(group), *(_p(out.get(k)) if k in out else None for k in ("r", "sqerr", "rho", "weight"))))
        return out

    def _lin_select(self, group, index):
        """(n, index array or None, res_kind) of a selection of blocks of `group`: index 1-BASED, any order, repeats allowed; None: every block"""
        ncost = self._groups[group][0] if 0 <= group < len(self._groups) else 0
        kind = self._kinds[group] if 0 <= group < len(self._groups) else -1
        ix = None if index is None else np.ascontiguousarray(index, np.int64).ravel()
        return (int(ix.size) if ix is not None else ncost), ix, kind

    def eval_jacobians(self, group, which=VARS_CURRENT, index=None, want=("r", "J")):
        """nlls_eval_jacobians: computeresjac of blocks of cost group `group` (0-based) at variable set `which`, every slot free -- a dict with the entries of `want`:
        "r" (n, M) the residual and "J" (n, M, NJ), J[i, m, j] = d r_m / d (tangent entry j of the non-kernel slots, in slot order).  index: 1-BASED blocks in upload
        order (any order, repeats allowed), None: every block; record i belongs to index[i]."""
        want = (want,) if isinstance(want, str) else tuple(want)
        assert want and set(want) <= {"r", "J"}
        n, ix, kind = self._lin_select(group, index)
        M, NJ = max(self.L.nlls_res_nres(kind), 0), max(self.L.nlls_res_jac_cols(kind), 0)
        out = {k: np.zeros((n, M) if k == "r" else (n, NJ, M)) for k in want}           # (J comes column-major: M x NJ per block)
        self._chk(self.L.nlls_eval_jacobians(self.h, int(which), int(group), n, _p(ix), _p(out.get("r")), _p(out.get("J"))))
        if "J" in out:
            out["J"] = np.ascontiguousarray(out["J"].transpose(0, 2, 1))
        return out

    def eval_gradhess(self, group, which=VARS_CURRENT, index=None, want=("cost", "g", "H")):
        """nlls_eval_gradhess: computecostgradhess of blocks of cost group `group` (0-based) at variable set `which`, every slot free -- "cost" (n,) 0.5 rho (a cost kind:
        the value), "g" (n, P) the robustified gradient, "H" (n, P, P) the robustified Hessian; adaptive kinds: the kernel's three entries first.  index as in eval_jacobians."""
        want = (want,) if isinstance(want, str) else tuple(want)
        assert want and set(want) <= {"cost", "g", "H"}
        n, ix, kind = self._lin_select(group, index)
        P = max(self.L.nlls_res_gh_dim(kind), 0)
        out = {k: np.zeros({"cost": (n,), "g": (n, P), "H": (n, P, P)}[k]) for k in want}
        self._chk(self.L.nlls_eval_gradhess(self.h, int(which), int(group), n, _p(ix), _p(out.get("cost")), _p(out.get("g")), _p(out.get("H"))))
        if "H" in out:
            out["H"] = np.ascontiguousarray(out["H"].transpose(0, 2, 1))                 # (column-major P x P per block -> H[i, row, column])
        return out

    # ---- matrix-free products with the linearisation (include/nlls_amd.h) ------------------------------------
    def _apply(self, fn, head, vin, nin, nout):
        """vin (nin,) or (nvec, nin) -> (nout,) or (nvec, nout) through fn(ctx, *head, nvec, in, out), at most APPLY_MAX_VEC vectors per call"""
        a = np.ascontiguousarray(vin, np.float64); one = a.ndim == 1
        a = a.reshape(1, -1) if one else a
        assert a.ndim == 2 and a.shape[1] == nin, f"expected vectors of length {nin}"
        out = np.zeros((a.shape[0], nout))
        for k0 in range(0, a.shape[0], APPLY_MAX_VEC):
            ak = np.ascontiguousarray(a[k0:k0 + APPLY_MAX_VEC]); ok = out[k0:k0 + APPLY_MAX_VEC]
            self._chk(fn(self.h, *head, ak.shape[0], _p(ak if ak.size else np.zeros(1)), _p(ok if ok.size else np.zeros(1))))      # (vectors of no entry: pointers that are not null)
        return out[0] if one else out

    def _group_rows(self, group):
        """doubles of u per vector for cost group `group`: ncost * M (0 for a group the library will refuse)"""
        if not 0 <= group < len(self._groups):
            return 0
        return self._groups[group][0] * max(self.L.nlls_res_nres(self._kinds[group]), 0)

    def hess_apply(self, v, lam=0.0, which=VARS_CURRENT):
        """nlls_hess_apply: (H + lam I) v at variable set `which`, H the sum of the blocks' nlls_eval_gradhess Hessians over the free unknowns -- evaluated, not read
        from A.data.  v (ndof,) -> (ndof,); (nvec, ndof) -> (nvec, ndof)."""
        n = self.info.ndof
        return self._apply(self.L.nlls_hess_apply, (int(which), float(lam)), v, n, n)

    def jac_apply(self, group, v, which=VARS_CURRENT):
        """nlls_jac_apply: J v per block of cost group `group` (0-based): (ndof,) -> (ncost * M,), block i at [i * M, (i + 1) * M); 2-D input: one row per vector"""
        return self._apply(self.L.nlls_jac_apply, (int(which), int(group)), v, self.info.ndof, self._group_rows(int(group)))

    def jact_apply(self, group, u, which=VARS_CURRENT):
        """nlls_jact_apply: J' u of cost group `group`'s blocks alone: (ncost * M,) -> (ndof,); 2-D input: one row per vector"""
        return self._apply(self.L.nlls_jact_apply, (int(which), int(group)), u, self._group_rows(int(group)), self.info.ndof)

    def hess_block_diag(self, lam=0.0, which=VARS_CURRENT):
        """nlls_hess_block_diag: the diagonal blocks of H + lam I, one (dof, dof) array per unfixed block, in block order"""
        bs = self.block_sizes(); out = np.zeros(int((bs * bs).sum()))
        self._chk(self.L.nlls_hess_block_diag(self.h, int(which), float(lam), _p(out)))
        off = np.concatenate(([0], np.cumsum(bs * bs)))
        return [out[off[b]:off[b + 1]].reshape(bs[b], bs[b]).T.copy() for b in range(bs.size)]

    def block_sizes(self):
        """dof of every unfixed block, in block order (from nlls_get_bsm_index's offsets)"""
        bo = np.asarray(self.bsm_index()[3], np.int64) - 1
        return np.diff(np.concatenate((bo, [self.info.ndof]))).astype(np.int64)

    def adaptive_em(self, kernel_var=1, which=VARS_NEXT, maxiters=10):
        """nlls_adaptive_em: the ContaminatedGaussian variable `kernel_var` (1-based) of set `which` re-estimated by Expectation-Maximization on the device, written
        back into that set.  Returns (storage (1/sigma1, 1/sigma2, w), passes made)."""
        st = np.zeros(3); it = C.c_int32(0)
        self._chk(self.L.nlls_adaptive_em(self.h, int(which), int(kernel_var), int(maxiters), _p(st), C.byref(it)))
        return st, int(it.value)

    def set_cost_data(self, group, data, index=None):
        """nlls_set_cost_data: new payload records for blocks of cost group `group` (0-based) of the uploaded structure -- `data` (n x ndata) for the blocks `index`
        (1-BASED, the caller's upload order of that group, as everywhere in the ABI; distinct) or, index=None, for the first n blocks (n = ncost: the whole group).
        No linearisation is held afterwards: sweep_gradhess before the next trial."""
        da = np.ascontiguousarray(data, np.float64)
        ix = None if index is None else np.ascontiguousarray(index, np.int64).ravel()
        nd = self._ndata[group] if 0 <= group < len(self._ndata) else 0
        n = int(ix.size) if ix is not None else (int(da.size // nd) if nd else (da.shape[0] if da.ndim > 1 else 0))
        assert not nd or da.size == n * nd, "set_cost_data: data must hold ndata doubles per listed block"      # (an unknown group is the library's to refuse)
        self._chk(self.L.nlls_set_cost_data(self.h, int(group), n, _p(ix), _p(da)))

    def set_robust_params(self, group, params):
        """nlls_set_robust_params: the robust kernel's parameters of cost group `group` (0-based; the kind stays) -- a kinds.Robustifier's .params or up to four numbers"""
        par = np.zeros(4); v = np.asarray(getattr(params, "params", params), np.float64).ravel(); par[:min(v.size, 4)] = v[:4]
        self._chk(self.L.nlls_set_robust_params(self.h, int(group), _p(par)))

    def get_grad(self):
        out = np.zeros(self.info.ndof); self._chk(self.L.nlls_get_grad(self.h, _p(out))); return out

    def get_grad_owned(self):
        out = np.zeros(self.info.ndof); self._chk(self.L.nlls_get_grad_owned(self.h, _p(out))); return out

    def get_bsm_data(self):
        out = np.zeros(self.info.nnz_data); self._chk(self.L.nlls_get_bsm_data(self.h, _p(out))); return out

    def max_abs_diag(self):
        return self._scalar(self.L.nlls_max_abs_diag)

    def grad_sqnorm(self):
        return self._scalar(self.L.nlls_grad_sqnorm)

    def grad_quadform(self):
        return self._scalar(self.L.nlls_grad_quadform)

    def damp(self, delta):
        self._chk(self.L.nlls_damp(self.h, float(delta)))

    def solve(self, want_x=False):
        out = np.zeros(self.info.ndof) if want_x else None
        self._chk(self.L.nlls_solve(self.h, _p(out)))
        return out

    def solve_pcg(self, precond=PCG_PRECOND_BLOCK_JACOBI, maxiters=None, rtol=1e-8, want_x=False):
        """nlls_solve_pcg: the step by conjugate gradients on the matrix-free operator, (H + lambda I) y = b from 0, x = -y, where solve() factors.  precond: 1 / "blockjacobi",
        0 / "none"; maxiters: 4 ndof when None.  -> (x or None, stats) with stats = dict(iterations, status (0 converged, 1 maxiters), bnorm, rnorm, rounds, launches).
        A breakdown (status 2, 3) raises NllsError with code ERR_NOT_SPD, as solve() does for a bad pivot, and leaves the step as it was; last_pcg holds its stats."""
        pc = PCG_PRECONDS[precond] if isinstance(precond, str) or precond is None else int(precond)
        mi = max(4 * int(self.info.ndof), 1) if maxiters is None else int(maxiters)
        out = np.zeros(self.info.ndof) if want_x else None; st = np.zeros(8)
        rc = self.L.nlls_solve_pcg(self.h, pc, mi, float(rtol), _p(out), _p(st))
        self.last_pcg = dict(iterations=int(st[0]), status=int(st[1]), bnorm=float(st[2]), rnorm=float(st[3]), rounds=int(st[4]), launches=int(st[5]))
        self._chk(rc)
        return out, self.last_pcg

    # ---- the reduced system, matrix-free (include/nlls_amd.h) -----------------------------------------------------
    def schur_info(self):
        """nlls_schur_info: (nred, nelim, is_elim, red_index) -- the dof of the reduced system, the number of eliminated blocks, a bool per unfixed block, and the
        positions of the reduced unknowns in b (ascending block order: the order of a reduced vector)"""
        nb = int(self.info.nblocks); nred, nelim = C.c_int64(0), C.c_int64(0); mask = np.zeros(max(nb, 1), np.uint8)
        self._chk(self.L.nlls_schur_info(self.h, C.byref(nred), C.byref(nelim), _p(mask)))
        is_elim = mask[:nb].astype(bool); bs = self.block_sizes()
        red_index = np.flatnonzero(np.repeat(~is_elim, bs)).astype(np.int64)
        return int(nred.value), int(nelim.value), is_elim, red_index

    def _nred(self):
        if getattr(self, "_nred_of_upload", None) is None:       # (asked once per upload: the products need it to shape their arrays)
            nred = C.c_int64(0); self._chk(self.L.nlls_schur_info(self.h, C.byref(nred), None, None)); self._nred_of_upload = int(nred.value)
        return self._nred_of_upload

    def schur_apply(self, v, lam=0.0, which=VARS_CURRENT):
        """nlls_schur_apply: S(lam) v, S = B + lam I - E (C + lam I)^-1 E' over the upload's eliminated set, H evaluated at variable set `which` and never formed.
        v (nred,) -> (nred,); (nvec, nred) -> (nvec, nred).  An upload that eliminated nothing raises NllsError (ERR_UNSUPPORTED)."""
        n = self._nred()
        return self._apply(self.L.nlls_schur_apply, (int(which), float(lam)), v, n, n)

    def schur_reduce(self, b, lam=0.0, which=VARS_CURRENT):
        """nlls_schur_reduce: b_r - E (C + lam I)^-1 b_e.  b (ndof,) -> (nred,); 2-D input: one row per vector"""
        return self._apply(self.L.nlls_schur_reduce, (int(which), float(lam)), b, self.info.ndof, self._nred())

    def schur_expand(self, b, yr, lam=0.0, which=VARS_CURRENT):
        """nlls_schur_expand: yr on the reduced entries, (C + lam I)^-1 (b_e - E' yr) on the eliminated ones: expand(b, S^-1 reduce(b)) solves (H + lam I) y = b.
        b (ndof,), yr (nred,) -> (ndof,); 2-D inputs: one row per vector"""
        n, nr = self.info.ndof, self._nred()
        a = np.ascontiguousarray(b, np.float64); y = np.ascontiguousarray(yr, np.float64); one = a.ndim == 1
        a = a.reshape(1, -1) if one else a; y = y.reshape(1, -1) if y.ndim == 1 else y
        assert a.ndim == 2 and a.shape[1] == n and y.shape == (a.shape[0], nr), f"expected b of length {n} and yr of length {nr}, one row per vector"
        out = np.zeros((a.shape[0], n))
        for k0 in range(0, a.shape[0], APPLY_MAX_VEC):
            ak = np.ascontiguousarray(a[k0:k0 + APPLY_MAX_VEC]); yk = np.ascontiguousarray(y[k0:k0 + APPLY_MAX_VEC]); ok = out[k0:k0 + APPLY_MAX_VEC]
            self._chk(self.L.nlls_schur_expand(self.h, int(which), float(lam), ak.shape[0], _p(ak), _p(yk if yk.size else np.zeros(1)), _p(ok)))      # (nred 0: a pointer that is not null)
        return out[0] if one else out

    def schur_block_diag(self, lam=0.0, which=VARS_CURRENT):
        """nlls_schur_block_diag: the diagonal blocks of S(lam) itself -- B_ii + lam I - sum over the eliminated neighbours e of E_ie (C_e + lam I)^-1 E_ie' -- one
        (dof, dof) array per REDUCED block, in ascending block order, unfactored (what "schurjacobi" inverts).  An eliminated block without a factor raises
        NllsError (ERR_NOT_SPD); an upload that eliminated nothing raises ERR_UNSUPPORTED."""
        is_elim = self.schur_info()[2]; bs = self.block_sizes()[~is_elim]; out = np.zeros(max(int((bs * bs).sum()), 1))
        self._chk(self.L.nlls_schur_block_diag(self.h, int(which), float(lam), _p(out)))
        off = np.concatenate(([0], np.cumsum(bs * bs)))
        return [out[off[b]:off[b + 1]].reshape(bs[b], bs[b]).T.copy() for b in range(bs.size)]

    def solve_pcg_schur(self, precond=PCG_PRECOND_BLOCK_JACOBI, maxiters=None, rtol=1e-8, want_x=False):
        """nlls_solve_pcg_schur: solve_pcg on the reduced system -- conjugate gradients from 0 on S yr = reduce(b), y = expand(b, yr), x = -y as the step.  precond:
        1 / "blockjacobi" (the diagonal blocks of B + lambda I), 3 / "schurjacobi" (the diagonal blocks of S itself), 0 / "none"; maxiters: 4 ndof when None; rtol on the REDUCED residual.  -> (x or None, stats) with
        solve_pcg's dictionary, bnorm and rnorm those of the reduced system.  A breakdown (status 2, 3; an eliminated block without a factor is 3) raises NllsError
        with code ERR_NOT_SPD and leaves the step as it was; last_pcg_schur holds its stats.  An upload that eliminated nothing raises ERR_UNSUPPORTED."""
        pc = PCG_PRECONDS[precond] if isinstance(precond, str) or precond is None else int(precond)
        mi = max(4 * int(self.info.ndof), 1) if maxiters is None else int(maxiters)
        out = np.zeros(self.info.ndof) if want_x else None; st = np.zeros(8)
        rc = self.L.nlls_solve_pcg_schur(self.h, pc, mi, float(rtol), _p(out), _p(st))
        self.last_pcg_schur = dict(iterations=int(st[0]), status=int(st[1]), bnorm=float(st[2]), rnorm=float(st[3]), rounds=int(st[4]), launches=int(st[5]))
        self._chk(rc)
        return out, self.last_pcg_schur

    def solve_pcg_tr(self, radius, precond=PCG_PRECOND_BLOCK_JACOBI, maxiters=None, rtol=1e-8, want_x=False):
        """nlls_solve_pcg_tr: solve_pcg inside the trust region ||y||_M <= radius (Steihaug-Toint), M the preconditioner (the identity under "none"); +inf is allowed.
        -> (x or None, stats) with solve_pcg's dictionary plus mnorm (||y||_M at exit) and model (the predicted reduction b'y - 1/2 y'(H + lambda I)y >= 0); status 0
        converged and 1 maxiters inside the region, 4 stopped on the boundary, 5 non-positive curvature followed to the boundary: all four set the step.  A breakdown
        (status 2, 3) raises NllsError with code ERR_NOT_SPD and leaves the step as it was; last_pcg_tr holds its stats, last_pcg stays solve_pcg's."""
        pc = PCG_PRECONDS[precond] if isinstance(precond, str) or precond is None else int(precond)
        mi = max(4 * int(self.info.ndof), 1) if maxiters is None else int(maxiters)
        out = np.zeros(self.info.ndof) if want_x else None; st = np.zeros(8)
        rc = self.L.nlls_solve_pcg_tr(self.h, pc, mi, float(rtol), float(radius), _p(out), _p(st))
        self.last_pcg_tr = dict(iterations=int(st[0]), status=int(st[1]), bnorm=float(st[2]), rnorm=float(st[3]), rounds=int(st[4]), launches=int(st[5]),
                                mnorm=float(st[6]), model=float(st[7]))
        self._chk(rc)
        return out, self.last_pcg_tr

    @staticmethod
    def _pcg_rhs_stats(st, n):
        cols = st[:4 * n].reshape(n, 4)
        return dict(iterations=cols[:, 0].astype(np.int64), status=cols[:, 1].astype(np.int64), bnorm=cols[:, 2].copy(), rnorm=cols[:, 3].copy(),
                    synchronisations=int(st[4 * n]), launches=int(st[4 * n + 1]), product_vectors=int(st[4 * n + 2]), batches=int(st[4 * n + 3]))

    def solve_pcg_rhs(self, B, lam=0.0, which=VARS_CURRENT, precond=PCG_PRECOND_BLOCK_JACOBI, maxiters=None, rtol=1e-8):
        """nlls_solve_pcg_rhs: (H + lam I) x_k = b_k by conjugate gradients on the device for right-hand sides of the caller's, H evaluated at variable set `which`; no
        sign flip, nothing of the context changes.  B (ndof,) -> X (ndof,); (nrhs, ndof) -> (nrhs, ndof): eight columns iterate together, the preconditioner is set up
        once.  maxiters: 4 ndof when None.  -> (X, stats) with stats = dict of arrays iterations, status (0 converged, 1 maxiters), bnorm, rnorm -- one entry per
        column -- and the call's synchronisations, launches, product_vectors, batches.  A breakdown of any column (status 2, 3) raises NllsError with code ERR_NOT_SPD;
        last_pcg_rhs holds the stats."""
        pc = PCG_PRECONDS[precond] if isinstance(precond, str) or precond is None else int(precond)
        mi = max(4 * int(self.info.ndof), 1) if maxiters is None else int(maxiters)
        a = np.ascontiguousarray(B, np.float64); one = a.ndim == 1
        a = a.reshape(1, -1) if one else a
        assert a.ndim == 2 and a.shape[1] == self.info.ndof, f"expected right-hand sides of length {self.info.ndof}"
        n = a.shape[0]; out = np.zeros_like(a); st = np.zeros(4 * n + 4)
        rc = self.L.nlls_solve_pcg_rhs(self.h, int(which), float(lam), pc, mi, float(rtol), n, _p(a), _p(out), _p(st))
        self.last_pcg_rhs = self._pcg_rhs_stats(st, n)
        self._chk(rc)
        return (out[0] if one else out), self.last_pcg_rhs

    def marginal_cov(self, varindices, lam=0.0, which=VARS_CURRENT, precond=PCG_PRECOND_BLOCK_JACOBI, maxiters=None, rtol=1e-8):
        """nlls_marginal_cov: the rows and columns of (H + lam I)^-1 that belong to the listed variables (1-BASED indices of the upload, any order, unfixed, distinct), in
        the listed order: (m, m) with m the sum of their dof, in the tangent space of their update().  Column j is the solve for unit vector j through solve_pcg_rhs's
        solver; symmetry is not enforced.  -> (cov, stats) with stats as solve_pcg_rhs, a column per unknown; a breakdown raises NllsError (ERR_NOT_SPD), last_pcg_rhs
        holds the stats.  A column with status 1 has NOT converged: check stats["status"]."""
        pc = PCG_PRECONDS[precond] if isinstance(precond, str) or precond is None else int(precond)
        mi = max(4 * int(self.info.ndof), 1) if maxiters is None else int(maxiters)
        vi = np.ascontiguousarray(varindices, np.int64).ravel()
        vk, vd = getattr(self, "_var_kind", ()), getattr(self, "_var_dim", ())
        m = int(sum(max(self.L.nlls_var_dof(int(vk[v - 1]), int(vd[v - 1])), 0) for v in vi[(vi >= 1) & (vi <= len(vd))]))      # (a list the library refuses: it says why)
        cov = np.zeros((m, m)); st = np.zeros(4 * m + 4)
        rc = self.L.nlls_marginal_cov(self.h, int(which), float(lam), int(vi.size), _p(vi), pc, mi, float(rtol), _p(cov), _p(st))
        self.last_pcg_rhs = self._pcg_rhs_stats(st, m)
        self._chk(rc)
        return np.ascontiguousarray(cov.T), self.last_pcg_rhs

    def lm_trial(self, dlambda, to=VARS_NEXT, frm=VARS_CURRENT):
        """damp + solve + retract + cost sweep in one call / one synchronisation; returns the trial cost."""
        out = C.c_double()
        self._chk(self.L.nlls_lm_trial(self.h, float(dlambda), to, frm, C.byref(out)))
        return out.value

    def optimize_singles(self, varindices, cptr, cgroup, cindex, cslot, maxiters=100, maxfails=3, reldcost=1e-15, absdcost=1e-15, dstep=1e-15, iterator=1):
        """nlls_optimize_singles; returns the iterations each listed variable took."""
        vi = np.ascontiguousarray(varindices, np.int64); cp = np.ascontiguousarray(cptr, np.int64)
        cg = np.ascontiguousarray(cgroup, np.int32); ci = np.ascontiguousarray(cindex, np.int64); cs = np.ascontiguousarray(cslot, np.int32)
        assert cp.size == vi.size + 1 and cg.size == ci.size == cs.size == (int(cp[-1]) if cp.size else 0)
        iters = np.zeros(vi.size, np.int64)
        self._chk(self.L.nlls_optimize_singles(self.h, vi.size, _p(vi), _p(cp), _p(cg), _p(ci), _p(cs), int(iterator), int(maxiters), int(maxfails),
                                                float(reldcost), float(absdcost), float(dstep), _p(iters)))
        return iters

    # ---- collectives behind the ABI (include/nlls_amd.h) ------------------------------------------------------
    ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p)

    def set_allreduce(self, fn):
        """fn(dev_ptr, count, op, hip_stream) -> 0: in-place all-reduce of `count` doubles in device memory (op 0 sum, 1 max).  The LM
        loop's entry points then run collectively inside the library (nlls_lm_iterations included).  fn = None removes it."""
        if fn is None:
            self._reduce_cb = None
            self._chk(self.L.nlls_set_allreduce(self.h, None, None)); return
        def tramp(user, ptr, count, op, stream):
            try:
                return int(fn(ptr, count, op, stream) or 0)
            except Exception as e:          # (an exception must not unwind through the C frames)
                self._reduce_exc = e; return 1
        self._reduce_cb = self.ALLREDUCE_FN(tramp)       # kept alive with the context
        self._chk(self.L.nlls_set_allreduce(self.h, self._reduce_cb, None))

    @staticmethod
    def comm_unique_id():
        buf = (C.c_ubyte * 128)()
        rc = lib().nlls_comm_unique_id(buf)
        if rc != OK:
            raise NllsError(rc, "nlls_comm_unique_id: librccl could not be loaded")
        return bytes(buf)

    def comm_init_rccl(self, id128):
        """RCCL inside the library: one communicator for this context (after set_shard), collectives on the context's stream."""
        buf = (C.c_ubyte * 128).from_buffer_copy(id128)
        self._chk(self.L.nlls_comm_init_rccl(self.h, buf))

    def memory_info(self):
        out = np.zeros(5, np.int64); self._chk(self.L.nlls_get_memory_info(self.h, _p(out), 5))
        return dict(working_set_bytes=int(out[0]), arena_bytes=int(out[1]), a_data_bytes=int(out[2]), reduced_system_bytes=int(out[3]), sharded_reduce_bytes=int(out[4]))

    def check_analytic(self):
        """closed-form Jacobians / kernel derivatives against the dual-number statement, per quantity (include/nlls_amd.h)"""
        out = np.zeros(7); self._chk(self.L.nlls_check_analytic(self.h, _p(out), 7))
        return dict(zip(("J", "Jtr", "cost", "drho", "d2rho", "dkernel", "d2kernel"), out.tolist()))

    def robustify(self, robust, costs):
        """robustify / robustifydcost of a kinds.Robustifier at each cost, evaluated on the device (nlls_robustify): an (n, 4) array of (robustify, rho, rho', rho'')"""
        c = np.ascontiguousarray(costs, dtype=np.float64).ravel(); out = np.zeros((c.size, 4)); par = np.array(robust.params, dtype=np.float64)
        self._chk(self.L.nlls_robustify(self.h, int(robust.kind), _p(par), c.size, _p(c), _p(out)))
        return out

    def flush_cache(self, nbytes):
        self._chk(self.L.nlls_flush_cache(self.h, int(nbytes)))

    def comm_post_flag(self, value):
        self._chk(self.L.nlls_comm_post_flag(self.h, float(value)))

    def comm_agreed_flag(self, local_value):
        out = C.c_double(0.0); self._chk(self.L.nlls_comm_agreed_flag(self.h, float(local_value), C.byref(out))); return float(out.value)

    def comm_info(self):
        """what the library's own communicator reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice), not the launcher's environment"""
        out = np.zeros(4, np.int64); self._chk(self.L.nlls_comm_info(self.h, _p(out), 4))
        return dict(nranks=int(out[0]), rank=int(out[1]), device=int(out[2]), transport={0: "none", 1: "rccl", 2: "caller-installed all-reduce"}[int(out[3])])

    def set_option(self, option, value):
        """nlls_set_option: OPT_MATERIALIZE (1: nlls_lm_trial eliminates from the materialised A.data, 0: matrix-free where it applies), OPT_LOOKAHEAD,
        OPT_APPLY_SCRATCH (bytes of record scratch of the matrix-free products), OPT_APPLY_WAVE_MIN (incidences from which a row gets a wavefront),
        OPT_PCG_ROUND (iterations solve_pcg enqueues between two looks at its stop flag), OPT_PCG_GRID_MAX (most workgroups of its vector kernels)"""
        self._chk(self.L.nlls_set_option(self.h, int(option), int(value)))

    def phase_times(self):
        """nlls_get_phase_times: microseconds per collective trial by phase (stream events; NLLS_OPT_PHASE_EVENTS) and per gradient sweep"""
        out = np.zeros(15); self._chk(self.L.nlls_get_phase_times(self.h, _p(out), 15)); nt, ns = max(out[6], 1.0), max(out[7], 1.0)
        return dict(trials=int(out[6]), sweeps=int(out[7]), elimination_us=1e3 * out[0] / nt, allreduce_S_us=1e3 * out[1] / nt, reduced_solve_us=1e3 * out[2] / nt,
                    backsub_retraction_us=1e3 * out[3] / nt, trial_tail_us=1e3 * out[4] / nt, gradient_sweep_us=1e3 * out[5] / ns,
                    update_scatter_us=1e3 * out[8], update_copies=int(out[9]),
                    linearize_us=1e3 * out[10], linearize_bytes=int(out[11]),
                    apply_us=1e3 * out[12], apply_bytes=int(out[13]), pcg_us=1e3 * out[14])

    def time_buckets(self):
        """device-timed NLLSResult buckets since the upload: seconds (gradient, cost, solver) and the trials counted"""
        out = np.zeros(4, np.int64); self._chk(self.L.nlls_get_time_buckets(self.h, _p(out), 4))
        return dict(timegradient=out[0] * 1e-9, timecost=out[1] * 1e-9, timesolver=out[2] * 1e-9, trials=int(out[3]))

    def solve_stats(self):
        out = np.zeros(56, np.int64); self._chk(self.L.nlls_get_solve_stats(self.h, _p(out), 56))
        return dict(status=int(out[0]), band_factor_cycles=int(out[1]), band_backward_cycles=int(out[2]), solve_mode=int(out[3]),
                    elim_supernodes=int(out[4]), bandwidth=int(out[5]), bcr_mfma_issued=int(out[6]), bcr_launches=int(out[7]), bcr_levels=int(out[8]),
                    band_dof=int(out[9]), dropped_pivots=int(out[10]), reduced_row_sums=int(out[11]), lazy_trials=int(out[12]),
                    reordered=int(out[13]), bandwidth_caller_order=int(out[14]), dense_window=int(out[15]),
                    tsp_tiles=int(out[16]), tsp_levels=int(out[17]), tsp_lower_tiles=int(out[18]), tsp_launches=int(out[19]), tsp_products=int(out[20]),
                    lookahead_hits=int(out[21]), lookahead_misses=int(out[22]), mf_trials=int(out[23]), reduced_sweeps=int(out[24]), full_sweeps=int(out[25]), bcr_block=int(out[26]),
                    singles_wave=int(out[27]), singles_thread=int(out[28]),
                    # the branches the upload chose: supernodes of the elimination by kernel class, neighbour blocks read transposed / in all, slab assembly in use;
                    # tiles of the accumulate sweep by class (summed over groups and slots), folded groups, groups the last full sweep launched fused
                    elim_fast60=int(out[29]), elim_fast_narrow=int(out[30]), elim_fast_wide=int(out[31]), elim_slow_acc=int(out[32]), elim_slow_noacc=int(out[33]),
                    elim_nbrs_transposed=int(out[34]), elim_nbrs=int(out[35]), elim_slab=int(out[36]),
                    sweep_light_tiles=int(out[37]), sweep_image_tiles=int(out[38]), sweep_direct_tiles=int(out[39]), sweep_partial_tiles=int(out[40]),
                    sweep_fold_groups=int(out[41]), sweep_fused_groups=int(out[42]),
                    # eval_jacobians / eval_gradhess: doubles of LDS a wavefront stages records in, lanes staged at a time for the last J / g / H asked for (0: stored directly)
                    linearize_slab=int(out[43]), linearize_batch_J=int(out[44]), linearize_batch_g=int(out[45]), linearize_batch_H=int(out[46]),
                    # the last matrix-free product: rows gathered one lane per unknown / a wavefront each, chunks its vectors were cut into, doubles of record scratch
                    apply_short_rows=int(out[47]), apply_wave_rows=int(out[48]), apply_chunks=int(out[49]), apply_scratch=int(out[50]),
                    # the chain kernels' form of the band solve (0: not theirs; 1 register window, 2 blocked one-sided, 3 blocked twisted); form 1: 1000 SEG + 10 NSLOT + CH / 8
                    chain_form=int(out[51]), chain_window=int(out[52]),
                    # the last solve_pcg: iterations made, status (0 converged, 1 maxiters, 2 / 3 breakdown), stream synchronisations
                    pcg_iterations=int(out[53]), pcg_status=int(out[54]), pcg_rounds=int(out[55]))

    def set_step(self, x):
        x = np.ascontiguousarray(x, np.float64); assert x.size == self.info.ndof
        self._chk(self.L.nlls_set_step(self.h, _p(x)))

    def get_step(self):
        out = np.zeros(self.info.ndof); self._chk(self.L.nlls_get_step(self.h, _p(out))); return out

    def step_maxabs(self):
        return self._scalar(self.L.nlls_step_maxabs)

    def step_norm(self):
        return self._scalar(self.L.nlls_step_norm)

    def quadform(self):
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.nlls_quadform(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def retract(self, to=VARS_NEXT, frm=VARS_CURRENT):
        self._chk(self.L.nlls_retract(self.h, to, frm))

    # ---- sharding ------------------------------------------------------------------------------------------
    def set_shard(self, rank, nranks):
        self._chk(self.L.nlls_set_shard(self.h, rank, nranks))

    def shard_info(self):
        out = np.zeros(6, np.int64); self._chk(self.L.nlls_get_shard_info(self.h, _p(out), 6))
        return dict(rank=int(out[0]), nranks=int(out[1]), local_ncost=int(out[2]), local_nnz_data=int(out[3]), local_ndof=int(out[4]), replicated=int(out[5]))

    def sweep_gradhess_local(self):
        self._chk(self.L.nlls_sweep_gradhess_local(self.h))

    def solve_finish_async(self):
        self._chk(self.L.nlls_solve_finish_async(self.h))

    def trial_local(self, to=VARS_NEXT, frm=VARS_CURRENT):
        out = np.zeros(6); self._chk(self.L.nlls_trial_local(self.h, to, frm, _p(out))); return out

    def lm_iterations(self, options, state, niter):
        """nlls_lm_iterations: up to niter outer Levenberg-Marquardt iterations in the library's own host loop (state updated in place)"""
        self._chk(self.L.nlls_lm_iterations(self.h, C.byref(options), C.byref(state), int(niter)))

    def trial_local_enqueue(self, to=VARS_NEXT, frm=VARS_CURRENT):
        """no synchronisation: the scalars stay on the device (reduce_buffer(3))"""
        self._chk(self.L.nlls_trial_local(self.h, to, frm, None))

    def solve_finish_replicated(self):
        self._chk(self.L.nlls_solve_finish_replicated(self.h))

    def get_variables_owned(self, which=VARS_CURRENT):
        out = np.zeros(self.info.var_storage); self._chk(self.L.nlls_get_variables_owned(self.h, which, _p(out))); return out

    def sweep_gradhess_finish(self, want_cost=True):
        if not want_cost:
            self._chk(self.L.nlls_sweep_gradhess_finish(self.h, None)); return None
        return self._scalar(self.L.nlls_sweep_gradhess_finish)

    def solve_local(self):
        self._chk(self.L.nlls_solve_local(self.h))

    def solve_finish(self):
        self._chk(self.L.nlls_solve_finish(self.h, None))

    def reduce_buffer(self, stage):
        ptr, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.nlls_get_reduce_buffer(self.h, stage, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def time_sweep_gradhess(self, reps=10):
        ms = C.c_float(); self._chk(self.L.nlls_time_sweep_gradhess(self.h, reps, C.byref(ms))); return ms.value

    def time_sweep_accumulate(self, reps=10):
        ms = C.c_float(); self._chk(self.L.nlls_time_sweep_accumulate(self.h, reps, C.byref(ms))); return ms.value

    def time_sweep_cost(self, reps=10):
        ms = C.c_float(); self._chk(self.L.nlls_time_sweep_cost(self.h, reps, C.byref(ms))); return ms.value

    def profile_sweep(self, on=True, read=False):
        """In-situ timing of the accumulate launches (event pairs inside the caller's loop): read=True -> (avg, min, max ms, samples)."""
        if not read:
            self._chk(self.L.nlls_profile_sweep(self.h, 1 if on else 0, None, None, None, None)); return None
        a, mn, mx, n = C.c_float(), C.c_float(), C.c_float(), C.c_int64()
        self._chk(self.L.nlls_profile_sweep(self.h, 1 if on else 0, C.byref(a), C.byref(mn), C.byref(mx), C.byref(n)))
        return a.value, mn.value, mx.value, n.value

    def profile_sweep_dispatch(self):
        """(avg, min, max ms, samples) of the recorded accumulate launches by their dispatch timestamps (what a kernel trace reports); read before profile_sweep(False, read=True) resets nothing"""
        a, mn, mx, n = C.c_float(), C.c_float(), C.c_float(), C.c_int64()
        self._chk(self.L.nlls_profile_sweep_dispatch(self.h, C.byref(a), C.byref(mn), C.byref(mx), C.byref(n)))
        return a.value, mn.value, mx.value, n.value

    def time_reduced_solve(self, reps=3):
        ms = C.c_float(); self._chk(self.L.nlls_time_reduced_solve(self.h, reps, C.byref(ms))); return ms.value

    def time_solve(self, reps=3):
        ms = C.c_float(); self._chk(self.L.nlls_time_solve(self.h, reps, C.byref(ms))); return ms.value
