/*
 * nlls_amd.h -- C ABI of the MI355X-native Gauss-Newton / Levenberg-Marquardt inner loop
 *               for NLLSsolver.jl (drop-in for the hot path only).
 *
 * The reference (NLLSsolver.jl v4.0.3, pure Julia) has no FFI of its own.  The seam this library
 * plugs into is Julia dispatch on the linear-system type: NLLSInternal{LSType} is parametric
 * (src/structs.jl:81-104) and the only factory is makesymmvls (src/linearsystem.jl:91-124, called
 * from src/optimize.jl:16).  A Julia shim type `MultiVariateLSgpu` (julia/NLLSsolverAMD.jl, shown in
 * INTEGRATION.md) overloads exactly the generic functions listed next to each entry point below and
 * `ccall`s them.  Every function:
 *   - returns int: 0 = NLLS_OK, negative = error (message via nlls_last_error),
 *   - never throws / longjmps across the boundary,
 *   - takes plain pointers + sizes; host buffers are only read/written during the call,
 *   - takes variable indices 1-BASED exactly as NLLSsolver stores them (SimpleError2.varind,
 *     src/residual.jl:4-7; blockindices, src/linearsystem.jl:93-102) and rebases internally,
 *   - is synchronous on return for anything it writes to a host pointer.
 * One context per host task; no re-entrancy (the reference is single threaded).
 *
 * Closed-world kinds: a HIP kernel cannot call a Julia closure, so residuals,
 * variables and robustifiers are a registry of kinds with device implementations.  Anything else
 * makes nlls_upload_structure return NLLS_ERR_UNSUPPORTED and the shim keeps the reference's CPU
 * linear system (decline, not failure).
 */
#ifndef NLLS_AMD_H
#define NLLS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nlls_ctx nlls_ctx;

/* ---- error codes ------------------------------------------------------------------------- */
#define NLLS_OK                 0
#define NLLS_ERR_INVALID_ARG   (-1)
#define NLLS_ERR_UNSUPPORTED   (-2) /* unregistered kind / structure: caller falls back to CPU path */
#define NLLS_ERR_HIP           (-3) /* a HIP runtime call failed                                    */
#define NLLS_ERR_NOT_READY     (-4) /* call order violated (e.g. solve before sweep)                */
#define NLLS_ERR_NOT_SPD       (-5) /* factorisation hit a non-positive / zero pivot                */
#define NLLS_ERR_NO_DEVICE     (-6) /* no gfx950 device visible: the product path never falls back  */

/* ---- compile-time limits mirrored from src/NLLSsolver.jl:28-30 ----------------------------- */
#define NLLS_MAX_ARGS        10
#define NLLS_MAX_BLOCK_SZ    32
#define NLLS_MAX_STATIC_VAR  64
#define NLLS_SINGLES_MAX_DOF 12   /* widest variable nlls_optimize_singles relaxes (the largest storage a fixed-size kind may have) */

/* ---- variable kinds: nvars()/update() of src/variable.jl:3-32, src/robustadaptive.jl:3-23 --- */
#define NLLS_VAR_EUCLIDEAN              1 /* EuclideanVector{N} / Number (N=1): dof N, storage N, v+d       */
#define NLLS_VAR_ZERO_TO_INF            2 /* ZeroToInfScalar: dof 1, storage 1, max(v,floatmin)*exp(d)      */
#define NLLS_VAR_ZERO_TO_ONE            3 /* ZeroToOneScalar: dof 1, storage 1, src/variable.jl:29-32       */
#define NLLS_VAR_CONTAMINATED_GAUSSIAN  4 /* ContaminatedGaussian: dof 3, storage 3 = (1/s1, 1/s2, w)       */
#define NLLS_VAR_POSE_SO3               5 /* NEW: R (3x3 col-major) + t, dof 6, storage 12,
                                             R <- R*expm([d(1:3)]x), t <- t + d(4:6)                      */
#define NLLS_VAR_DYNAMIC                6 /* DynamicVector{Float64}: a Euclidean vector of RUN-TIME length `dim` (1 .. NLLS_MAX_DYN_DIM):
                                             storage = dof = dim, update = v + delta (src/variable.jl); only under the DYN residual kinds */
#define NLLS_MAX_DYN_DIM             4096
/* USER variable kinds: the reference's variable blocks are any type with nvars() and update() (src/variable.jl; the Jacobian is taken through
 * update(var, dualzeros), src/autodiff.jl:57-61).  Ids 100 .. 107 are reserved for kinds a user header adds at BUILD time, next to its user residual
 * kinds (see NLLS_RES_USER0 below; variable and residual kinds are separate namespaces).  The header specialises
 *     template <> struct nlls::Var<NLLS_VAR_USERk> {
 *         static constexpr int STORAGE, DOF;             // 1 <= DOF <= STORAGE <= 12, DOF <= NLLS_MAX_BLOCK_SZ
 *         template <class T> static NLLS_HD void update(const double* v, const T* d, T* out);   // out = update(v, d), generic in T like Res<>::eval
 *     };
 * and lists its kinds in NLLS_USER_VAR(X), as it lists its residual kinds in NLLS_USER_RES(X).  The Jacobian of a user residual w.r.t. such a
 * variable is update() differentiated at d = 0 by dual numbers; the retraction of an LM step is update<double>.  A slot of a user residual names the
 * kind in SK (its SD is the kind's DOF); the variable's var_dim is its DOF.  User variable kinds are never Euclidean for the solver: an eliminated
 * one takes the materialised Schur elimination, a reduced one keeps the matrix-free LM trial.  They are refused in non-squared cost kinds.
 * In a library built without a user header nlls_var_storage / nlls_var_dof return a negative value for these ids. */
#define NLLS_VAR_USER0          100
#define NLLS_VAR_USER1          101
#define NLLS_VAR_USER2          102
#define NLLS_VAR_USER3          103
#define NLLS_VAR_USER4          104
#define NLLS_VAR_USER5          105
#define NLLS_VAR_USER6          106
#define NLLS_VAR_USER7          107

/* ---- residual kinds: computeresidual() bodies ----------------------------------------------- */
#define NLLS_RES_BA_AFFINE        1 /* SimpleError2{2}: (pose[1:3].X, pose[4:6].X) - meas; vars (EUCL6, EUCL3);
                                       data = meas[2]                      test/optimizeba.jl:4               */
#define NLLS_RES_ROSENBROCK_A     2 /* a*(1-x); vars (EUCL1); data = a     test/functional.jl:5-16            */
#define NLLS_RES_ROSENBROCK_B     3 /* b*(x^2-y); vars (EUCL1,EUCL1); data = b   test/functional.jl:18-25     */
#define NLLS_RES_ROSENBROCK_2D    4 /* (a(1-x1), b(x1^2-x2)); vars (EUCL2); data = (a,b)  examples/rosenbrock.jl:10-20 */
#define NLLS_RES_CURVE_EXP4       5 /* a*exp(b*t)+c*t+d - y; vars 4x EUCL1; data = (t,y)  (BASELINE config 2) */
#define NLLS_RES_ADAPTIVE_MEAN    6 /* AbstractAdaptiveResidual: mean - data; vars (CONT_GAUSS, EUCL1);
                                       data = value                        test/adaptivecost.jl:3-13          */
#define NLLS_RES_BA_SO3           7 /* NEW: pinhole projection of R*X+t, normalised image plane;
                                       vars (POSE_SO3, EUCL3); data = meas[2]                                  */
#define NLLS_RES_BA_SO3_ADAPTIVE  8 /* NEW: as 7 with the robust kernel as variable #1 (src/residual.jl:46-47);
                                       vars (CONT_GAUSS, POSE_SO3, EUCL3); data = meas[2]                      */
#define NLLS_RES_LINEAR3          9 /* LinearResidualStatic: X*w - y; vars (EUCL3); data = (y[3], X[9] column-major)   test/nonsquaredcost.jl:4-14 */
#define NLLS_COST_LINEAR3        10 /* NON-SQUARED AbstractCost (src/autodiff.jl:144-159): computecost = y'w, vars (EUCL3); data = y[3].  The block adds
                                       its value (not half a squared norm) to the cost, its gradient and Hessian -- by second-order duals through update() --
                                       to the linear system; robust_kind is ignored.                              test/nonsquaredcost.jl:28-37 */
#define NLLS_RES_DYN_LINEAR      11 /* DYNAMIC-size (src/autodiff.jl:96-121): LinearResidual X'w - y over one NLLS_VAR_DYNAMIC variable of run-time
                                       length n; data = (y, X[n]) -- n + 1 doubles per block; nres 1            test/dynamicvars.jl:3-11 */
#define NLLS_RES_DYN_NORM        12 /* DYNAMIC-size: NormResidual w over one NLLS_VAR_DYNAMIC variable: nres = n, no data    test/dynamicvars.jl:13-21.
                                       Dynamic kinds: every block of a group has the same n; the residual kinds take the robust kernels like any other residual
                                       (src/residual.jl:76-101), the non-squared cost kind none; the system may come out dense or block-sparse
                                       (src/linearsystem.jl:105-123 decides; round 4: block-sparse systems are taken too -- a dynamic variable's block
                                       row holds its diagonal block only, it is never eliminated; under nlls_set_shard its blocks are owned round robin); nlls_res_ndata / nlls_res_nres
                                       return -1 where the count is n-dependent */
#define NLLS_RES_DYN_LINEARSQ    13 /* DYNAMIC-size: LinearResidualDynamic X*w - y with a square X (n x n, column-major) over one NLLS_VAR_DYNAMIC
                                       variable of length n; data = (y[n], X[n*n]); nres = n; n <= 512              test/nonsquaredcost.jl:16-26 */
#define NLLS_COST_DYN_LINEAR     14 /* DYNAMIC-size NON-SQUARED AbstractCost: LinearCostDynamic, computecost = y'w; data = y[n]: value y'w, gradient y,
                                       Hessian 0 (src/autodiff.jl:144-159)                                          test/nonsquaredcost.jl:39-46 */
#define NLLS_RES_SCALE_MIX       15 /* s * (w a + (1 - w) b) - y over a STANDALONE ZeroToInfScalar s and a standalone ZeroToOneScalar w
                                     (src/variable.jl:18-32): vars (ZERO_TO_INF, ZERO_TO_ONE); data = (a, b, y).  No counterpart in the
                                     reference's tests; it makes the two bounded scalar kinds reachable outside ContaminatedGaussian */
#define NLLS_RES_KIND_COUNT      16
/* USER residual kinds (round 5).  The reference takes any Julia function as a residual and differentiates it with ForwardDiff (/root/reference/src/autodiff.jl:81-93,
 * README.md:36-46); a HIP kernel cannot call those, so the registry above is closed at run time -- but not at BUILD time: ids 100 .. 107 are reserved for kinds a user
 * header adds.  Such a header (nllssolver.jl_amd/csrc/Makefile: `make user USER_KINDS=/abs/path/kinds.hpp LIB=libmine.so OBJDIR=build_mine`) specialises
 * nlls::Res<NLLS_RES_USERk> -- NDEPS (<= MAX_SLOTS = 10 slots, the reference's MAX_ARGS), M, NDATA, the slots' variable kinds SK / dimensions SD, and ONE templated eval<T>(data, variables, r), generic in the
 * scalar type exactly like the reference's computeresidual -- and lists its kinds in NLLS_USER_RES(X).  Everything else follows from that: the Jacobian w.r.t. the tangent of
 * update() by dual numbers, the accumulate kernels, the cost sweep, optimizesingles, the Schur path.  tests/user_kinds/radial_ba.hpp is a worked example (an affine camera
 * with one radial distortion coefficient), built by __graft_entry__.build() and exercised on the GPU by tests/test_gpu_userkind.py. */
#define NLLS_RES_USER0          100
#define NLLS_RES_USER1          101
#define NLLS_RES_USER2          102
#define NLLS_RES_USER3          103
#define NLLS_RES_USER4          104
#define NLLS_RES_USER5          105
#define NLLS_RES_USER6          106
#define NLLS_RES_USER7          107

/* ---- robust kernels: src/robust.jl:7-77 ------------------------------------------------------ */
#define NLLS_ROBUST_NONE           0 /* NoRobust                                               */
#define NLLS_ROBUST_HUBER          1 /* HuberKernel(w):   params[0] = width                    */
#define NLLS_ROBUST_HUBER2O        2 /* Huber2oKernel(w): params[0] = width                    */
#define NLLS_ROBUST_GEMAN_MCCLURE  3 /* GemanMcclureKernel(w): params[0] = width               */
#define NLLS_ROBUST_SCALED      0x10 /* OR-ed flag: Scaled(inner, height): params[1] = height  */
/* adaptive residual kinds ignore robust_kind: their kernel is variable #1. */
/* USER robust kernels: the reference robustifies with any AbstractRobustifier -- robustify(kernel, cost), and robustifydcost either by second-order
 * autodiff of it (src/robust.jl:14, src/autodiff.jl:163) or in a closed form of the kernel's own (HuberKernel, src/robust.jl:48-55).  Ids 8 .. 15 are
 * reserved for kernels a user header adds at BUILD time, next to its residual and variable kinds; they compose with NLLS_ROBUST_SCALED like the built-in
 * ones.  The header specialises
 *     template <> struct nlls::Robust<NLLS_ROBUST_USERk> {
 *         static constexpr int NPARAM;                                        // 0 .. 2: p[0] = robust_params[0], p[1] = robust_params[2]
 *         template <class T> static NLLS_DEV T robustify(const double* p, T cost);                    // generic in T: double, and the jet nlls::Jet2
 *         static NLLS_DEV void dcost(const double* p, double cost, double& rho, double& d1, double& d2);   // optional: robustifydcost in closed form
 *     };
 * and lists its kernels in NLLS_USER_ROBUST(X).  Without dcost, (rho, d1, d2) are robustify and its first and second derivatives at the cost, by the
 * one-variable second-order dual nlls::Jet2 (+ - * / with doubles and jets, dsqrt, dexp, dexpm1, dlog, dlog1p; dval for branches on the value).
 * robust_params[1] stays Scaled's height.  In a library built without a user header these ids are refused (NLLS_ERR_UNSUPPORTED). */
#define NLLS_ROBUST_USER0          8
#define NLLS_ROBUST_USER1          9
#define NLLS_ROBUST_USER2         10
#define NLLS_ROBUST_USER3         11
#define NLLS_ROBUST_USER4         12
#define NLLS_ROBUST_USER5         13
#define NLLS_ROBUST_USER6         14
#define NLLS_ROBUST_USER7         15

/* ---- problem description --------------------------------------------------------------------- */
/* One group per Julia cost type (one VectorRepo entry, src/VectorRepo.jl:1-7), in values(costs)
 * order, each cost's fields struct-of-arrays. */
typedef struct nlls_cost_group {
    int32_t        res_kind;          /* NLLS_RES_*                                                  */
    int32_t        robust_kind;       /* NLLS_ROBUST_* (| NLLS_ROBUST_SCALED)                        */
    double         robust_params[4];
    int64_t        ncost;
    const int64_t* varind;            /* [ncost][ndeps], 1-based variable indices (varindices())     */
    const double*  data;              /* [ncost][ndata] per-cost payload (measurement etc.)          */
} nlls_cost_group;

typedef struct nlls_info {
    int32_t is_sparse;       /* 1: MultiVariateLSsparse/BlockSparseMatrix, 0: MultiVariateLSdense   */
    int32_t has_schur;       /* 1: an independent variable set is eliminated before the dense solve  */
    int64_t nvar;            /* number of variable blocks                                            */
    int64_t nblocks;         /* number of unfixed blocks                                             */
    int64_t ndof;            /* length of b / x                                                      */
    int64_t nnz_data;        /* length of A.data (BSM) or ndof*ndof (dense)                          */
    int64_t nblocks_stored;  /* number of stored blocks in the BSM                                   */
    int64_t ncost;           /* total number of cost blocks                                          */
    int64_t var_storage;     /* length of the packed variable vector                                 */
    int64_t nschur_blocks;   /* number of eliminated (Schur) variable blocks                         */
    int64_t nreduced_dof;    /* order of the dense reduced system                                    */
    int64_t owner_path;      /* 1: deterministic owner-gather accumulate, 0: atomic scatter          */
    int64_t solve_mode;      /* 0 small (one wave), 1 dense blocked LDL' (MFMA), 2 bordered band, 3 tile-sparse LDL' (nested dissection) */
    int64_t bandwidth;       /* half bandwidth (dof) of the banded part of the reduced system         */
    int64_t nborder_dof;     /* dof ordered last in the reduced system (dense border)                 */
} nlls_info;

/* flags for nlls_upload_structure */
#define NLLS_FLAG_FORCE_ATOMIC   0x1  /* always use the generic atomic scatter accumulate            */
#define NLLS_FLAG_NO_SCHUR       0x2  /* solve the full system densely (small problems / testing); taken automatically when an
                                         eliminated block has more neighbour dof than the Schur kernels stage in LDS */
#define NLLS_FLAG_FORCE_SPARSE   0x4  /* makesymmvls(...; formarginalization) style: BSM regardless   */
#define NLLS_FLAG_NO_BAND        0x8  /* never use the bordered-band solver (dense MFMA path instead)  */
#define NLLS_FLAG_NO_TWIST       0x10 /* band solver: factor from the top only (one workgroup), testing */
#define NLLS_FLAG_DETERMINISTIC  0x40 /* reduced system assembled without atomics (slab per supernode + ordered gather): x is bit-reproducible.  Takes effect where the
                                         reduced system is a band solved by block cyclic reduction (solve_mode 2, one rank, every eliminated block on the fast path);
                                         the dense and tile-sparse solvers assemble with atomic adds -- x reproducible to rounding -- and ignore it            */
#define NLLS_FLAG_PRESHARDED     0x80 /* under nlls_set_shard(rank, nranks > 1): the caller uploads ONLY this rank's share -- every uploaded cost block is this rank's,
                                         the eliminated variables present are its own, the other (reduced) variables are the same, in the same order, on every
                                         rank (bundle adjustment: all cameras + this rank's points).  Nothing is partitioned by the library; variable indices are
                                         the rank's own.  Lets each process of a large job generate and upload 1/N of the problem                       */
#define NLLS_FLAG_NO_BCR         0x20 /* band solver: the round-1 chain kernels (twisted blocked LDL') instead of block cyclic reduction */
#define NLLS_FLAG_NO_REORDER    0x100 /* keep the reduced variables in the caller's block order.  Default: the reduced blocks are put in reverse Cuthill-McKee
                                         order whenever that narrows the band of the reduced system -- the reference orders its factorisation itself
                                         (ldl_analyze, src/linearsystem.jl:52,68) and does not care how the caller numbers the variables; neither does x here */
#define NLLS_FLAG_NO_TILE_SPARSE 0x200 /* reduced solver: never the tile-sparse LDL' (solve_mode 3: nested dissection of the reduced blocks' graph, factored level by
                                         level of its elimination tree); the reduced system that is neither a narrow band nor small then takes the dense / windowed LDL' */
#define NLLS_FLAG_NO_PIVOT_FLOOR 0x400 /* damped solves (block cyclic reduction, tile-sparse LDL'): no pivot floor.  Default (round 5): a pivot that has lost eleven orders of
                                         magnitude against its unknown's original diagonal entry is dropped -- the unknown gets no step -- and counted (nlls_get_solve_stats()[10]),
                                         the rule undamped solves have had since round 2.  Silent while lambda / |diagonal| > 1e-11; below that it keeps rounding noise in the
                                         gauge directions of a converged problem from deciding the trial (the reference's LDL' divides by that noise: /root/reference/src/linearsolver.jl:28-32) */

/* variable-set ids for the on-device copies of problem.variables / varnext / varbest
 * (src/problem.jl:9-12) */
#define NLLS_FLAG_MATERIALIZE    0x800 /* never the matrix-free LM trial (round 6): nlls_lm_trial then eliminates from the materialised A.data as rounds 1-5 did.  Default: two-slot
                                       * Schur problems whose eliminated blocks all take the fast path (bundle adjustment) evaluate their cost blocks inside the elimination and the
                                       * back-substitution launches; A.data in the reference's layout is then formed on demand only (nlls_get_bsm_data, nlls_solve, ...). */
#define NLLS_VARS_CURRENT 0
#define NLLS_VARS_NEXT    1
#define NLLS_VARS_BEST    2

/* ---- lifecycle --------------------------------------------------------------------------------
 * replaces: GC-managed MultiVariateLSsparse/dense objects (src/linearsystem.jl:44-87).          */
int  nlls_ctx_create(const int32_t* device_ids, int32_t ndev, nlls_ctx** out);
int  nlls_ctx_destroy(nlls_ctx* ctx);
const char* nlls_last_error(const nlls_ctx* ctx);
/* run all launches of this context on an externally owned hipStream_t (0 = the context's own) */
int  nlls_set_stream(nlls_ctx* ctx, void* hip_stream);
/* observation sharding for N ranks: must precede nlls_upload_structure */
int  nlls_set_shard(nlls_ctx* ctx, int32_t rank, int32_t nranks);

/* static helpers (no context): storage length / dof of a variable kind; ndeps/nres/ndata of a
 * residual kind, and the variable kind+dim it expects in each slot. */
int  nlls_var_storage(int32_t var_kind, int32_t var_dim);
int  nlls_var_dof(int32_t var_kind, int32_t var_dim);
/* number of parameters of a robust kernel this library has (built-in or NLLS_ROBUST_USER0 .. 7 of its user header; the id without NLLS_ROBUST_SCALED),
 * negative for any other id */
int  nlls_robust_nparams(int32_t robust_kind);
int  nlls_res_ndeps(int32_t res_kind);
int  nlls_res_nres(int32_t res_kind);
int  nlls_res_ndata(int32_t res_kind);
int  nlls_res_slot_kind(int32_t res_kind, int32_t slot, int32_t* var_kind, int32_t* var_dim);
/* host-only helper (no context, no device): the ordering nlls_upload_structure applies to the banded part of the reduced system -- reverse
 * Cuthill-McKee (pseudo-peripheral start node, neighbours by ascending degree, components one after the other) of a symmetric graph in CSR form
 * (adjptr[n+1], adj: 0-based neighbours, no self loops; both directions listed).  perm_out[new position] = node.  Stands where the reference
 * calls ldl_analyze (src/linearsystem.jl:52,68), which orders the factorisation itself: the solve must not depend on the caller's numbering. */
int  nlls_rcm_order(int32_t n, const int64_t* adjptr, const int32_t* adj, int32_t* perm_out);
/* host-only helper (no context, no device): the symbolic phase of the tile-sparse reduced solver (solve_mode 3) -- nested dissection of the reduced
 * blocks' graph by breadth-first level structures, every part and separator packed into tiles of at most 128 unknowns, then the elimination tree and
 * the fill of the TILE graph.  n nodes with dof[i] unknowns each (CSR adjacency as for nlls_rcm_order) followed by nborder border nodes that couple
 * to everything (dof has n + nborder entries; nodes coupled to an eighth of all nodes or more are treated the same way: ordered last, their tiles neighbours of
 * every tile).  Out: tile_of / row_in_tile [n + nborder] (a node's tile, in elimination order, and its first row in
 * it); parent / level [max_tiles] (elimination tree over the tiles, -1 = root; tiles of one level are factored in one launch); the lower triangle of
 * the tile pattern of L as CSR (colptr [max_tiles + 1], rows [max_rows]: tiles i > k of column k, ascending).  Returns the number of tiles, or
 * NLLS_ERR_INVALID_ARG (malformed graph, a node wider than 128, outputs too small).  The reference's counterpart is ldl_analyze
 * (src/linearsystem.jl:52,68). */
int  nlls_nd_tiles(int32_t n, int32_t nborder, const int64_t* adjptr, const int32_t* adj, const int32_t* dof, int32_t* tile_of, int32_t* row_in_tile,
                   int32_t max_tiles, int32_t* parent, int32_t* level, int64_t* colptr, int64_t max_rows, int32_t* rows);

/* ---- factory ----------------------------------------------------------------------------------
 * replaces: makesymmvls(problem, unfixed, nblocks)   src/linearsystem.jl:91-124
 * Builds blocksizes, the sparse/dense decision (src/utils.jl:108-120), the BlockSparseMatrix
 * pattern and offsets exactly as src/BlockSparseMatrix.jl:30-47, boffsets
 * (src/linearsystem.jl:36-41) and all device-side work lists.
 * blockindices[i] = 0 for a fixed variable, else its 1-based block number (linearsystem.jl:93-102). */
int  nlls_upload_structure(nlls_ctx* ctx,
                           int64_t nvar, const int32_t* var_kind, const int32_t* var_dim,
                           const uint64_t* blockindices,
                           int32_t ngroups, const nlls_cost_group* groups,
                           int32_t flags);
int  nlls_get_info(const nlls_ctx* ctx, nlls_info* out);
/* parity/debug: indicestransposed of the BSM as CSC (colptr[nblocks+1], rowval, nzval; all 1-based)
 * and boffsets[nblocks] (1-based).  Any pointer may be NULL. */
int  nlls_get_bsm_index(const nlls_ctx* ctx, int64_t* colptr, int64_t* rowval, int64_t* nzval,
                        int64_t* boffsets);

/* ---- variables --------------------------------------------------------------------------------
 * packed layout: variable i occupies nlls_var_storage(kind_i, dim_i) doubles, in variable order. */
int  nlls_set_variables(nlls_ctx* ctx, int32_t which, const double* packed);
int  nlls_get_variables(nlls_ctx* ctx, int32_t which, double* packed);
int  nlls_swap_variables(nlls_ctx* ctx, int32_t a, int32_t b);   /* src/optimize.jl:207-214 */
int  nlls_copy_variables(nlls_ctx* ctx, int32_t dst, int32_t src);/* deepcopy, src/optimize.jl:81,141 */

/* ---- sweeps -----------------------------------------------------------------------------------
 * replaces: zero!(linsystem) + costgradhess!(linsystem, vars, costs)
 *           src/optimize.jl:118,167-170 -> src/cost.jl:29-54, src/residual.jl:57-111,
 *           src/linearsystem.jl:132-175.  Evaluated at NLLS_VARS_CURRENT.  Resets the damping.
 * cost_out == NULL: the cost is not wanted (the outer loop discards it between iterations, src/optimize.jl:167-170):
 * the sweep is only enqueued -- no cost reduction, no synchronisation; the next synchronising call waits for it.
 * The linearisation is that of the values NLLS_VARS_CURRENT holds at this call, whatever is written to them afterwards: a trial
 * after nlls_set_variables / nlls_copy_variables / nlls_retract into CURRENT (without a sweep between) solves with A and b of the
 * old values and retracts from the new ones -- also where the sweep is deferred or the trial is matrix-free.  One exception, the
 * same on every path: once an nlls_lm_trial has enqueued its look-ahead sweep (A and b then hold the linearisation at the trial
 * point), a trial from a CURRENT written after it is linearised at the new values. */
int  nlls_sweep_gradhess(nlls_ctx* ctx, double* cost_out);
/* replaces: cost(vars, costs)  src/cost.jl:10-13, src/residual.jl:49-55 */
int  nlls_sweep_cost(nlls_ctx* ctx, int32_t which, double* cost_out);
/* replaces: computeresidual (src/NLLSsolver.jl:16), cost(residual, vars) before the kernel (src/residual.jl:52), robustify and the rho' of
 * robustifydcost (src/robust.jl), per cost block.  For the ncost blocks of cost group `group` (0-based index of the nlls_cost_group at upload), IN THE
 * CALLER'S UPLOAD ORDER, at variable set `which`:
 *   r_out[i * nres .. ]  the residual (nres = nlls_res_nres of the kind; dynamic kinds: the group's run-time n, 1 for NLLS_RES_DYN_LINEAR),
 *   sqerr_out[i]         r'r,
 *   rho_out[i]           robustify(kernel, r'r): 0.5 * sum(rho_out) is the group's share of nlls_sweep_cost,
 *   weight_out[i]        rho' at r'r, the IRLS weight (1 without a robust kernel).
 * Any pointer may be NULL; all NULL is NLLS_ERR_INVALID_ARG.  Adaptive kinds take their kernel from slot 0 of each block.  Blocks whose variables are
 * all fixed are evaluated like the others.  The non-squared cost kinds (NLLS_COST_LINEAR3, NLLS_COST_DYN_LINEAR) have no residual: NLLS_ERR_UNSUPPORTED.
 * Needs an upload, no sweep; reads only (no validity state of the context changes: a call between a sweep and a trial leaves the trial as it was).
 * Under nlls_set_shard with nranks > 1 (not replicas) a rank holds only its own blocks: NLLS_ERR_UNSUPPORTED. */
int  nlls_eval_blocks(nlls_ctx* ctx, int32_t which, int32_t group, double* r_out, double* sqerr_out, double* rho_out, double* weight_out);
/* replaces: optimize(kernel::ContaminatedGaussian, squarederrors, maxiters)  src/robustadaptive.jl:48-73 -- the adaptive kernel's parameters by
 * Expectation-Maximization between two iterations (the EM callback of test/adaptivecost.jl:15-25), on the device.  kernel_var: 1-based index of a
 * NLLS_VAR_CONTAMINATED_GAUSSIAN variable.  squarederrors = r'r, at variable set `which`, of every block of every group of an adaptive kind whose slot 0
 * is that variable (in group, then upload order; none: NLLS_ERR_INVALID_ARG).  The blocks are evaluated once; then up to `maxiters` passes, enqueued
 * without a host round trip, each a fixed-order sum (no atomics: the result is bit-identical run to run) and a finishing workgroup that forms the new
 * parameters, orders them like the constructor (src/robustadaptive.jl:12-19: narrowest Gaussian first) and stops the passes behind it once
 * isapprox(old, new; rtol = 1e-6) holds.  The kernel starts from its storage in set `which`; the result is written INTO THAT SET on the device and to
 * storage_out (1/sigma1, 1/sigma2, w); iters_out = passes made (both may be NULL).  maxiters == 0 leaves the storage untouched.  Writing the set is
 * the same state transition as nlls_set_variables(which): see nlls_sweep_gradhess for what a trial behind it is linearised at.
 * Under nlls_set_shard with nranks > 1 (not replicas): NLLS_ERR_UNSUPPORTED. */
int  nlls_adaptive_em(nlls_ctx* ctx, int32_t which, int64_t kernel_var, int32_t maxiters, double storage_out[3], int32_t* iters_out);

/* ---- the linearisation of single cost blocks -----------------------------------------------------------------------------
 * What the sweeps sum into A.data and b, per block and before any sum: to inspect the Jacobian of one outlier block, to hand J to a solver of the caller's own, to
 * propagate a measurement covariance, to check a user residual header against finite differences.
 * Both calls: `group`, `n`, `index` as in nlls_set_cost_data -- index[i] is 1-based, in the caller's upload order of that group; index == NULL: the first n blocks.
 * Nothing is written through the index: it may be in any order and may name a block more than once.  Output record i belongs to index[i].  Evaluated at variable set
 * `which` with EVERY slot treated as free (the kept entries of a varflags specialisation are identical: drop the rows and columns of fixed slots); blocks whose
 * variables are all fixed are evaluated like the others.  Derivatives are with respect to the tangent of update() at 0.  One launch, no atomics: two calls return
 * identical bytes.  Any output pointer may be NULL; all NULL is NLLS_ERR_INVALID_ARG.  n == 0: NLLS_OK.  NLLS_ERR_INVALID_ARG -- nothing enqueued, no output byte
 * written -- for a bad group, n < 0, n > ncost with index == NULL, or an index outside 1 .. ncost.  NLLS_ERR_UNSUPPORTED: nlls_eval_jacobians on a non-squared cost
 * kind (NLLS_COST_LINEAR3: it has no residual); both calls on the dynamic-size kinds (their Jacobian is their own payload); both calls under nlls_set_shard with
 * nranks > 1 (a rank holds only its own blocks).  Need an upload, no sweep (NLLS_ERR_NOT_READY before one); read only, like nlls_eval_blocks: no validity state of
 * the context changes, scratch of their own, a call between a sweep and a trial leaves the trial as it was.  Synchronous on return.
 *
 * replaces: computeresjac(varflags = all free, residual, vars...)  src/autodiff.jl:78-93, src/NLLSsolver.jl:16
 *   r_out[i * M + m]              the residual, the same values as nlls_eval_blocks' r (M = nlls_res_nres),
 *   J_out[i * M * NJ + m + M * j] the Jacobian, column-major M x NJ: NJ = nlls_res_jac_cols = the sum of the dof of the non-kernel slots, in slot order. */
int  nlls_eval_jacobians(nlls_ctx* ctx, int32_t which, int32_t group, int64_t n, const int64_t* index, double* r_out, double* J_out);
/* replaces: computecostgradhess / computerescostgradhess, all variables free  src/residual.jl:57-111, src/autodiff.jl:144-159
 *   cost_out[i]        0.5 rho (a non-squared cost kind: the value itself),
 *   g_out[i * P ..]    the robustified gradient, P = nlls_res_gh_dim,
 *   H_out[i * P * P ..] the robustified Hessian, full symmetric, column-major P x P.
 * Adaptive kinds: P = NJ + 3, the kernel's three entries first, the border as src/residual.jl:79-88,103-107.  NLLS_COST_LINEAR3: value, gradient and Hessian of the cost. */
int  nlls_eval_gradhess(nlls_ctx* ctx, int32_t which, int32_t group, int64_t n, const int64_t* index, double* cost_out, double* g_out, double* H_out);
/* static helpers, no context: columns of J; length of g (= order of H).  Negative (NLLS_ERR_UNSUPPORTED) for an unknown or a dynamic-size kind. */
int  nlls_res_jac_cols(int32_t res_kind);
int  nlls_res_gh_dim(int32_t res_kind);

/* ---- matrix-free products with the linearisation ---------------------------------------------------------------------------
 * The linearisation applied to vectors, without A.data: a residual ||(H + lambda I) x + g|| of any solve, Krylov methods of the caller's own (CG, LSQR, Lanczos,
 * Hutchinson probes), the model decrease of a step the caller formed.  No full accumulate sweep on a context that runs the matrix-free trial, no copy of A.data, no
 * matrix rebuilt from the BlockSparseMatrix index.
 * H = sum over cost blocks of P' H_blk P, H_blk exactly what nlls_eval_gradhess returns for the block (robustified, second-order term included; adaptive kinds: with
 * the kernel's three rows and columns; NLLS_COST_LINEAR3: the cost's own Hessian); P keeps the unknowns of the block's free slots and drops the fixed ones, a block
 * without a free slot contributes nothing.  lambda * v is added on every unknown (uniformscaling!, src/BlockSparseMatrix.jl:83-99).  J is that of
 * nlls_eval_jacobians: unrobustified, non-kernel slots only; fixed slots contribute 0 to J v and have no row in J' u, the kernel variable's rows of J' u are 0.
 * EVALUATED at variable set `which` at the time of the call, not read from a stored A.data: the products equal those with the sweep's A only while `which` still
 * holds what the sweep saw.  lambda is the argument, not the damping nlls_damp has accumulated.
 * Layouts: vectors over the unknowns have length ndof, in the order of b and x; vector k starts at v + k * ndof.  A group's u holds ncost * M doubles per vector
 * (M = nlls_res_nres): block i of the caller's upload order at u + k * ncost * M + i * M.  d_out holds the unfixed blocks in block order, block b at offset
 * sum_{c<b} dof_c^2, column-major dof_b x dof_b, full symmetric.  All pointers are host pointers; synchronous on return.
 * Two launches per chunk of vectors and no atomics: one lane per cost block leaves a record per block and vector, then every unknown's records are summed in
 * ascending (group, block, slot) order -- rows of fewer than NLLS_OPT_APPLY_WAVE_MIN incidences one lane per unknown, longer rows a wavefront each with a fixed
 * tree over its lanes (a row of more than 4096 incidences: a wavefront per segment of 4096, the segments added in order).  Two calls return identical bytes; vector k of a call of nvec equals the call on v_k alone, byte for byte; so does a call whose vectors were
 * cut into chunks because their records exceed NLLS_OPT_APPLY_SCRATCH bytes.
 * NLLS_ERR_INVALID_ARG -- nothing enqueued, no output byte written -- for a null context or pointer, `which` outside 0 .. 2, a bad group, nvec < 1 or
 * nvec > NLLS_APPLY_MAX_VEC, a non-finite lambda.  NLLS_ERR_NOT_READY before an upload.  NLLS_ERR_UNSUPPORTED: nlls_jac_apply / nlls_jact_apply on a non-squared cost
 * kind or a dynamic-size kind; nlls_hess_apply / nlls_hess_block_diag when any group is of a dynamic-size kind (no per-block Hessian: nlls_eval_gradhess refuses
 * them too); all four under nlls_set_shard with nranks > 1.  ndof == 0: NLLS_OK, nothing written.  Need an upload, no sweep; read only, like the nlls_eval_* calls:
 * no validity state of the context changes, scratch and an index of their own (built at the first call after an upload), a call between a sweep and a trial
 * leaves the trial as it was. */
#define NLLS_APPLY_MAX_VEC 8
/* replaces: hessian * x of the iterators (gethessgrad, src/linearsystem.jl:180-190, src/iterators.jl:47-115) and, as v . y, fast_bAb (src/utils.jl:71-106)
 *   y_k = (H + lambda I) v_k, k < nvec */
int  nlls_hess_apply(nlls_ctx* ctx, int32_t which, double lambda, int32_t nvec, const double* v, double* y_out);
/* replaces: the Jacobian-vector product behind the iterators' predicted residual (src/iterators.jl:47-115): u_k = J v_k, per block of one group */
int  nlls_jac_apply(nlls_ctx* ctx, int32_t which, int32_t group, int32_t nvec, const double* v, double* u_out);
/* replaces: the gradient J' r of gethessgrad (src/linearsystem.jl:180-190) for any u: y_k = J' u_k, this group's blocks alone */
int  nlls_jact_apply(nlls_ctx* ctx, int32_t which, int32_t group, int32_t nvec, const double* u, double* y_out);
/* replaces: the diagonal blocks of gethessgrad's hessian (block(A, i, i), src/BlockSparseMatrix.jl; src/linearsystem.jl:180-190) under uniformscaling!:
 *   the diagonal blocks of H + lambda I, a block-Jacobi preconditioner */
int  nlls_hess_block_diag(nlls_ctx* ctx, int32_t which, double lambda, double* d_out);

/* ---- conjugate gradients on the device ------------------------------------------------------------------------------
 * replaces: solve!(linsystem) + negate!(linsystem.x) of the iterators (src/linearsystem.jl:180-190, src/iterators.jl:149-157) by an ITERATIVE solve: no reduced
 *           system, no factorisation, no read of A.data; with maxiters small, a truncated-Newton (inexact) step.
 * nlls_solve_pcg stands where nlls_solve stands: it solves (H + lambda I) y = b by preconditioned conjugate gradients from y = 0 and leaves x = -y as the context's
 * step.  lambda: the damping nlls_damp has accumulated; b: the gradient of the last sweep, as nlls_get_grad returns it; H: applied by the launches of nlls_hess_apply at
 * NLLS_VARS_CURRENT, one vector per iteration, on device pointers (the caveat stated there holds: H is evaluated, and equals the sweep's A only while CURRENT holds what
 * the sweep saw).  The preconditioner is the identity or the inverse of the diagonal blocks of H + lambda I (nlls_hess_block_diag, factored once per call).
 * It stops when the residual of the recurrence satisfies ||r||_2 <= rtol ||b||_2 (status 0) or after maxiters iterations (status 1); both return NLLS_OK and set the
 * step -- a truncated iterate from 0 is a descent direction.  ||b|| == 0: x = 0, status 0, 0 iterations.  Breakdown: status 2 -- p'(H + lambda I)p is not > 0, or a
 * scalar of the recurrence is not finite -- and status 3 -- a diagonal block of the block-Jacobi preconditioner is not positive definite -- return NLLS_ERR_NOT_SPD
 * (what the iterators answer with more damping) and leave the context's step, x_out and everything else byte for byte as before the call: only stats_out and the
 * counters below are written.
 * stats_out[8] (may be NULL): [0] iterations made (status 2: the iteration that broke down, counted from 1), [1] status, [2] ||b||_2 (status 3: 0, the start never
 * ran), [3] ||r||_2 of the recurrence at exit, [4] stream synchronisations of the call (one per round of NLLS_OPT_PCG_ROUND iterations, one more for the step it
 * sets), [5] launches it enqueued, [6], [7] 0.
 * Every sum has a fixed order and nothing adds with atomics: two calls on the same sweep return identical bytes, and so do calls that differ only in
 * NLLS_OPT_PCG_ROUND.  The host looks at the stop flag once per round; the iterations enqueued behind a stop change nothing but the product's scratch.
 * NLLS_ERR_INVALID_ARG -- nothing enqueued -- for a null context, a precond other than the two, maxiters < 1, rtol not finite or < 0; NLLS_ERR_NOT_READY before an
 * upload or without a sweep (as nlls_solve); NLLS_ERR_UNSUPPORTED where nlls_hess_apply is: a group of a dynamic-size kind, nlls_set_shard with nranks > 1.
 * ndof == 0: NLLS_OK.  On success the step is the caller's as after nlls_set_step: nlls_retract, nlls_step_maxabs, nlls_step_norm, nlls_quadform and nlls_get_step
 * see it.  Success or breakdown, A.data, b, the variable sets, the damping and the validity state of the linearisation are untouched; the solver works in buffers of
 * its own (allocated at the first call after an upload).  nlls_get_solve_stats [53..55] and nlls_get_phase_times [14] report the last call; [47..50] there then
 * describe its last product. */
#define NLLS_PCG_PRECOND_NONE          0   /* M = I */
#define NLLS_PCG_PRECOND_BLOCK_JACOBI  1   /* M = the diagonal blocks of H + lambda I (nlls_hess_block_diag) */
/* 2 is unassigned and refused by every entry point, on purpose: it is the value the refusal tests of the four conjugate-gradient entry points hold */
#define NLLS_PCG_PRECOND_SCHUR_JACOBI  3   /* M = the diagonal blocks of S(lambda) (nlls_schur_block_diag); nlls_solve_pcg_schur only: the others refuse it with NLLS_ERR_INVALID_ARG */
int  nlls_solve_pcg(nlls_ctx* ctx, int32_t precond, int32_t maxiters, double rtol, double* x_out, double* stats_out);

/* ---- conjugate gradients on the caller's right-hand sides; marginal covariance blocks ----------------------------------
 * replaces: solve!(linsystem) for a right-hand side other than the gradient (src/linearsolver.jl:20-32: the reference solves with whatever the linear system's b
 *           holds, and a caller who wants another right-hand side overwrites it), as a call that takes the right-hand sides and leaves the linear system alone.
 * For every k < nrhs: (H + lambda I) x_k = b_k by the iteration of nlls_solve_pcg from x_k = 0.  Column k is at B + k * ndof and at X_out + k * ndof, host pointers, in
 * the order of b and x.  H is that of nlls_hess_apply, evaluated at variable set `which` at the time of the call; lambda is the ARGUMENT, not the damping nlls_damp has
 * accumulated.  No sign flip: X solves the system as written (with B = nlls_get_grad's vector, `which` = CURRENT, lambda = the context's damping and nrhs = 1, X_out is
 * -x of nlls_solve_pcg byte for byte, and the column's four statistics are equal).  Needs an upload and no sweep; read only, like the products: the context's step,
 * A.data, b, the variable sets, the damping, the validity state, a pending look-ahead sweep and the counters of the last nlls_solve_pcg are untouched.  Synchronous.
 * Status per column, as nlls_solve_pcg: 0 ||r_k|| <= rtol ||b_k|| (a zero column: status 0, 0 iterations, x_k = 0); 1 maxiters reached; 2 p'(H + lambda I)p not > 0
 * or a scalar not finite (a NaN in b_k ends here); 3 a diagonal block of the preconditioner has no Cholesky factor -- call-wide: every column reports 3 and 0
 * iterations.  A column that stops leaves the others running.  NLLS_OK when every column ended 0 or 1; NLLS_ERR_NOT_SPD when any ended 2 or 3: then no byte of X_out
 * is written and stats_out tells which column.
 * stats_out[4 * nrhs + 4] (may be NULL): per column k at [4 k ..]: iterations, status, ||b_k||_2, ||r_k||_2 of the recurrence at exit; then, for the call: stream
 * synchronisations, launches, product vectors (the sum over its products of the vectors each carried), batches.
 * At most NLLS_APPLY_MAX_VEC columns iterate together, each iteration ONE product over the columns still iterating; a call with more columns runs them in batches of
 * eight, in order.  The preconditioner is set up once per call.  The host looks at all columns' stop flags once per round of NLLS_OPT_PCG_ROUND iterations; a column
 * found stopped pays for no further product.  Column k's bytes and its four statistics do not depend on which other columns the call carries, on their order, on
 * nrhs, on where a batch ends or on NLLS_OPT_PCG_ROUND; two calls return identical bytes; different NLLS_OPT_PCG_GRID_MAX agree to rounding.
 * Memory: 6 * min(nrhs, 8) * ndof doubles of vectors and nrhs * ndof for the columns, outside the hot arena, allocated on demand.
 * NLLS_ERR_INVALID_ARG -- nothing enqueued, no output byte written -- for a null context, B or X_out, `which` outside 0 .. 2, nrhs < 1, a precond other than the two,
 * maxiters < 1, rtol not finite or < 0, lambda not finite; NLLS_ERR_NOT_READY before an upload; NLLS_ERR_UNSUPPORTED where nlls_hess_apply is (a dynamic-size group,
 * nlls_set_shard with nranks > 1); ndof == 0: NLLS_OK, X_out untouched, stats_out zeros. */
int  nlls_solve_pcg_rhs(nlls_ctx* ctx, int32_t which, double lambda, int32_t precond, int32_t maxiters, double rtol, int32_t nrhs, const double* B, double* X_out, double* stats_out);
/* replaces: nothing -- the reference has NO covariance routine.  The nearest thing in it is the vestigial `formarginalization` flag of makesymmvls
 *           (src/linearsystem.jl:91-118), which only orders the variables for a marginalisation it never performs; Ceres, g2o and GTSAM answer "how certain is this
 *           variable" with marginal covariance blocks, and this is that call.
 * The joint covariance block of the listed variables: with m = the sum of their dof, cov_out is m x m, column-major -- the rows and columns of (H + lambda I)^-1 that
 * belong to the listed variables, in the listed order, in the tangent space of their update() as x is.  varindices: nsel 1-based variable indices of the upload (as
 * nlls_optimize_singles takes them), in any order.  The entry is the inverse of H: scaling by a noise level is the caller's.  Column j is the solve for unit vector j
 * -- written on the device, nothing of length ndof crosses the bus, and only the m selected rows of a finished column are kept -- through the batched solver of
 * nlls_solve_pcg_rhs: eight columns at a time, the preconditioner once; so symmetry holds to the solve's accuracy and is not enforced, and every byte rule above holds.
 * A singular H at lambda = 0 (a problem whose gauge is free) shows as status 1, 2 or 3: fix the gauge with fixed variables, or pass a lambda > 0.
 * stats_out[4 * m + 4] (may be NULL) as above, a column per unknown.  NLLS_OK when every column ended 0 or 1 (check the statuses: a column that ended on maxiters is
 * not a covariance); NLLS_ERR_NOT_SPD on any 2 or 3, cov_out untouched.  Refusals as above, and NLLS_ERR_INVALID_ARG for nsel < 1, a null varindices, an index outside
 * 1 .. nvar, an index listed twice, a listed variable that is fixed (it has no row in H). */
int  nlls_marginal_cov(nlls_ctx* ctx, int32_t which, double lambda, int64_t nsel, const int64_t* varindices, int32_t precond, int32_t maxiters, double rtol, double* cov_out, double* stats_out);

/* ---- the reduced system, matrix-free: products with the Schur complement and conjugate gradients on it -----------------------
 * replaces: the reduced system the reference's direct solvers form and factor (src/linearsolver.jl:20-32) -- here it is applied, never formed: what Ceres calls
 *           ITERATIVE_SCHUR, and the only Schur path for a reduced system too large to store.
 * The upload picks an independent set of blocks to eliminate (nlls_info::nschur_blocks of them).  Two sets of unknowns:
 *   e   the eliminated blocks
 *   r   the other unfixed blocks, in ascending block order; nred is their dof, and a REDUCED vector has nred entries in that order
 * With H + lambda I = [[B, E], [E', C]] over (r, e), C is block diagonal, and S(lambda) = B + lambda I - E (C + lambda I)^-1 E'.
 * nlls_schur_info: nred, the number of eliminated blocks, and (is_elim_out not NULL) one byte per unfixed block, 1 where it is eliminated.  Needs an upload; no device work.
 * The three products follow the rules of nlls_hess_apply: H is evaluated at set `which` at the time of the call, never read from A.data; lambda is the argument; host
 * pointers, synchronous; they need an upload and no sweep, and change nothing -- no validity state, step, A.data, b, variable set, damping or pending look-ahead sweep;
 * nvec is 1 .. NLLS_APPLY_MAX_VEC, cut into chunks under NLLS_OPT_APPLY_SCRATCH; every sum has a fixed order (no atomics): two calls return identical bytes, vector k
 * of a call equals the call on it alone, a chunked call equals the unchunked one.
 *   nlls_schur_apply    y_k = S(lambda) v_k
 *   nlls_schur_reduce   s_k = b_r - E (C + lambda I)^-1 b_e
 *   nlls_schur_expand   the r entries of y_k are yr_k, bit for bit; the e entries are (C + lambda I)^-1 (b_e - E' yr_k): expand(b, S^-1 reduce(b)) solves (H + lambda I) y = b
 * NLLS_ERR_INVALID_ARG where nlls_hess_apply returns it (nothing enqueued, no byte written); NLLS_ERR_NOT_READY before an upload; NLLS_ERR_UNSUPPORTED where
 * nlls_hess_apply refuses, and when the upload eliminated nothing (a dense system, NLLS_FLAG_NO_SCHUR): nlls_last_error says so; NLLS_ERR_NOT_SPD when a block
 * C_e + lambda I has no Cholesky factor, no output byte written.
 * nlls_solve_pcg_schur stands where nlls_solve_pcg stands: the gradient of the last sweep, H at CURRENT, the context's damping.  Conjugate gradients from 0 on
 * S yr = reduce(b), then y = expand(b, yr) and x = -y as the context's step.  precond: NLLS_PCG_PRECOND_NONE, or NLLS_PCG_PRECOND_BLOCK_JACOBI -- here the diagonal
 * blocks of B + lambda I.  It stops on the recurrence's ||r|| <= rtol ||s|| of the REDUCED system.  Statuses, return codes and stats_out[8] as nlls_solve_pcg, with
 * ||s|| and the reduced ||r|| in [2], [3]; status 3 also covers an eliminated block without a factor; on 2 or 3 the step and x_out stay byte for byte.  The counters
 * of nlls_get_solve_stats and nlls_get_phase_times keep describing the last nlls_solve_pcg.  NLLS_OPT_PCG_ROUND, NLLS_OPT_PCG_GRID_MAX and NLLS_OPT_APPLY_WAVE_MIN
 * mean here what they mean for the full products.
 * Under NLLS_PCG_PRECOND_SCHUR_JACOBI (Ceres' SCHUR_JACOBI) M is the diagonal blocks of S(lambda) itself -- every eliminated neighbour takes its curvature off a reduced
 * block, which the blocks of B + lambda I do not see.  Everything above holds; status 3 also covers an S_ii without a Cholesky factor, and stats_out[5] counts the
 * set-up's extra launches (the off-diagonal records of every group, the subtraction).  The iteration's launches, scalars and synchronisations are block Jacobi's.
 * nlls_schur_block_diag returns those blocks, unfactored: for a reduced block i, with the sum over its eliminated neighbours e,
 *   S_ii = B_ii + lambda I - sum_e E_ie (C_e + lambda I)^-1 E_ie'
 * where E_ie is the SUM of the off-diagonal blocks of every cost block that joins i and e, taken before the product.  d_out (a HOST pointer, as every vector of the
 * products; synchronous): the reduced blocks in ascending block order -- the order of the reduced vector -- block i at offset sum_{c < i, c reduced} dof_c^2,
 * column-major, full symmetric: nlls_hess_block_diag's layout restricted to the r class.  A reduced block without an eliminated neighbour holds the bytes
 * nlls_hess_block_diag returns for it.  An indefinite S_ii is returned as it is.  Rules and refusals of nlls_schur_apply: H at set `which` at call time, lambda the
 * argument, an upload and no sweep, read only (the counters of the last nlls_solve_pcg included), fixed-order sums and identical bytes from two calls;
 * NLLS_ERR_INVALID_ARG for a null pointer, `which` outside 0 .. 2, a lambda that is not finite; NLLS_ERR_NOT_READY; NLLS_ERR_UNSUPPORTED for a sharded context, a
 * dynamic-size group, an upload that eliminated nothing; NLLS_ERR_NOT_SPD, no byte written, where a C_e + lambda I has no Cholesky factor; nred == 0: NLLS_OK, nothing
 * written. */
int  nlls_schur_block_diag(nlls_ctx* ctx, int32_t which, double lambda, double* d_out /* sum over the reduced blocks of dof^2 */);
int  nlls_schur_info(const nlls_ctx* ctx, int64_t* nred_out, int64_t* nelim_out, uint8_t* is_elim_out /* nblocks, may be NULL */);
int  nlls_schur_apply(nlls_ctx* ctx, int32_t which, double lambda, int32_t nvec, const double* v /* nvec x nred */, double* y_out /* nvec x nred */);
int  nlls_schur_reduce(nlls_ctx* ctx, int32_t which, double lambda, int32_t nvec, const double* b /* nvec x ndof */, double* s_out /* nvec x nred */);
int  nlls_schur_expand(nlls_ctx* ctx, int32_t which, double lambda, int32_t nvec, const double* b /* nvec x ndof */, const double* yr /* nvec x nred */, double* y_out /* nvec x ndof */);
int  nlls_solve_pcg_schur(nlls_ctx* ctx, int32_t precond, int32_t maxiters, double rtol, double* x_out, double* stats_out);

/* ---- conjugate gradients inside a trust region (Steihaug-Toint) --------------------------------------------------------------
 * replaces: the dogleg iterator's Cauchy point plus Gauss-Newton solve (src/iterators.jl:47-115) by ONE iterative call: without a preconditioner the first iterate of
 *           the method is the Cauchy point and its last the Newton step, with every piece of the path in between, and no factorisation.
 * nlls_solve_pcg_tr stands where nlls_solve_pcg stands: b the gradient of the last sweep, H evaluated at NLLS_VARS_CURRENT by the launches of nlls_hess_apply, lambda
 * the context's damping (normally 0 under a trust region; any finite value).  From y = 0 it approximately minimises q(y) = 1/2 y'(H + lambda I)y - b'y subject to
 * ||y||_M <= radius and leaves x = -y as the context's step.  M is the preconditioner: the identity under NLLS_PCG_PRECOND_NONE (the Euclidean norm), the diagonal
 * blocks of H + lambda I under NLLS_PCG_PRECOND_BLOCK_JACOBI (an ellipsoid) -- the norm in which the iterates of preconditioned conjugate gradients grow
 * monotonically, the only one in which "stop at the boundary" is well defined.  H need not be positive definite.  Statuses:
 *   0  ||r|| <= rtol ||b||, inside the region
 *   1  maxiters reached, inside the region
 *   4  the next iterate would leave the region: y = y_k + tau p_k with ||y||_M = radius
 *   5  p'(H + lambda I)p <= 0: y = y_k + tau p_k, to the boundary along p_k
 *   2  a scalar of the recurrence is not finite, or the curvature is not positive and radius is +inf (there is no boundary to go to)
 *   3  a block of the preconditioner has no Cholesky factor
 * 0, 1, 4 and 5 return NLLS_OK and set the step: every such exit is a descent step.  2 and 3 return NLLS_ERR_NOT_SPD and leave the step, x_out and everything else
 * byte for byte, as nlls_solve_pcg does.  tau is the positive root of pp tau^2 + 2 yp tau + (yy - radius^2) = 0 with yy = ||y_k||_M^2, yp = y_k'M p_k,
 * pp = ||p_k||_M^2, in the form that does not cancel: tau = (radius^2 - yy) / (yp + sqrt(yp^2 + pp (radius^2 - yy))).  The three follow from scalars the recurrence
 * has: the call makes the launches and synchronisations of nlls_solve_pcg, no more, and with radius = +inf on a positive definite system its x_out and stats_out[0..5]
 * are nlls_solve_pcg's byte for byte.
 * stats_out[8] (may be NULL): [0] .. [5] as nlls_solve_pcg, [3] the residual r_k - tau q_k at the returned point; [6] ||y||_M at exit (status 4, 5: the radius);
 * [7] the predicted reduction -q(y) = b'y - 1/2 y'(H + lambda I)y >= 0, in the units of nlls_sweep_cost: the denominator of the iterators' gain ratio, sign turned.
 * NLLS_ERR_INVALID_ARG -- nothing enqueued, nothing written -- for what nlls_solve_pcg refuses and for a radius that is NaN or <= 0 (+inf is allowed);
 * NLLS_ERR_NOT_READY and NLLS_ERR_UNSUPPORTED as nlls_solve_pcg (a sharded context among them); ndof == 0: NLLS_OK; ||b|| == 0: status 0, 0 iterations, x = 0.
 * The bit rules of nlls_solve_pcg hold.  The counters of nlls_get_solve_stats and nlls_get_phase_times keep describing the last nlls_solve_pcg. */
int  nlls_solve_pcg_tr(nlls_ctx* ctx, int32_t precond, int32_t maxiters, double rtol, double radius, double* x_out, double* stats_out);

/* ---- the costs of an uploaded structure, changed in place -------------------------------------------------------------
 * replaces: the reference's mutable cost objects -- a residual's measurement, a robust kernel's width -- and optimize! called again on the same
 *           problem (src/optimize.jl:5-17): graduated non-convexity, re-measurement, outer EM / IRLS loops, refits of new data on one structure.
 * nlls_upload_structure is the symbolic phase (entry lists, tiles, the eliminated set, supernodes, orderings); these two change what it was given
 * WITHOUT redoing it: which variables a block depends on, which are fixed, the kinds and ncost stay as uploaded.
 *
 * nlls_set_cost_data: new payload records for n blocks of cost group `group` (0-based index of the nlls_cost_group at upload, as in nlls_eval_blocks).
 *   data[i * ndata ..] is the record of block index[i] -- 1-based, in the caller's upload order of that group; index == NULL: of block i + 1, the first
 *   n blocks (n == ncost: the whole group).  ndata is what the upload used (nlls_res_ndata; dynamic kinds: the count their variable's length gives).
 *   Every device copy of the record is rewritten (the cost-order arrays, the entry lists, the dense list, the matrix-free trial's list) by one
 *   host-to-device copy and one launch on the context's stream, behind whatever is enqueued there.  `index` and `data` are read during the call only.
 *   NLLS_ERR_INVALID_ARG -- nothing enqueued, nothing changed -- for a bad group, n < 0, n > ncost, an index outside 1 .. ncost or listed twice,
 *   or data == NULL with n > 0.  n == 0: NLLS_OK, nothing changes (the state below included).
 * nlls_set_robust_params: robust_params of cost group `group` (the meaning of nlls_cost_group::robust_params; [3] is unused as there).  The kind stays,
 *   NLLS_ROBUST_SCALED included.  The kernels take the parameters by value with every launch: a host-side write.  An adaptive group's kernel is a
 *   variable, not a parameter: NLLS_ERR_INVALID_ARG.
 * Both: the linear system is of the old costs -- the state after an upload without a sweep: nlls_lm_trial, nlls_solve, nlls_get_grad, ... return
 *   NLLS_ERR_NOT_READY until the next nlls_sweep_gradhess; a look-ahead sweep pending behind the last trial is dropped.  nlls_sweep_cost,
 *   nlls_eval_blocks, nlls_optimize_singles and nlls_adaptive_em need no sweep and see the new costs at once.  The variable sets, the damping the
 *   caller holds and the counters of nlls_get_solve_stats are untouched.  NLLS_ERR_NOT_READY before a successful upload; under nlls_set_shard with
 *   nranks > 1: NLLS_ERR_UNSUPPORTED (a rank holds only its own blocks). */
int  nlls_set_cost_data(nlls_ctx* ctx, int32_t group, int64_t n, const int64_t* index, const double* data);
int  nlls_set_robust_params(nlls_ctx* ctx, int32_t group, const double params[4]);

/* ---- linear system access ---------------------------------------------------------------------
 * replaces: gethessgrad (src/linearsystem.jl:180-190), initlambda (src/iterators.jl:131-137). */
int  nlls_get_grad(nlls_ctx* ctx, double* b_out);                 /* linsystem.b            */
int  nlls_get_bsm_data(nlls_ctx* ctx, double* data_out);          /* A.data (BSM or dense)  */
int  nlls_max_abs_diag(nlls_ctx* ctx, double* out);               /* max_i |H_ii|           */
int  nlls_grad_sqnorm(nlls_ctx* ctx, double* out);                /* gradient' * gradient   */
int  nlls_grad_quadform(nlls_ctx* ctx, double* out);              /* fast_bAb(H, gradient)  */

/* replaces: uniformscaling!(hessian, k)  src/iterators.jl:149,162 */
int  nlls_damp(nlls_ctx* ctx, double delta);
/* replaces: negate!(solve!(linsystem, options))  src/iterators.jl:152 -> src/linearsolver.jl:28-32.
 * Solves (H + lambda I) y = b and stores x = -y on the device; x_out (length ndof) may be NULL. */
int  nlls_solve(nlls_ctx* ctx, double* x_out);
/* diagnostics of the last solve: [0] factorisation status (0 ok), [1] band factor shader cycles,
 * [2] band backward-pass cycles, [3] solve mode, [4] number of elimination supernodes, [5] bandwidth,
 * [6] v_mfma_f64_16x16x4_f64 instructions one reduced solve issues (block cyclic reduction; 2048 flop each), [7] its launches,
 * [8] its levels, [9] banded dof of the reduced system, [10] pivots the last UNDAMPED band solve dropped: with lambda == 0 (Newton,
 * dogleg's Gauss-Newton step) on a gauge-free problem the reduced system is singular, and the block-cyclic-reduction solver treats a
 * pivot that has lost eleven orders of magnitude against its original diagonal entry as infinite (that unknown gets no step) instead
 * of dividing rounding by rounding; NaN pivots are never dropped (they raise NLLS_ERR_NOT_SPD).  The chain and dense solvers
 * (NLLS_FLAG_NO_BCR, NLLS_FLAG_NO_BAND) have no such floor.  Collective route (see "collectives"): [11] sums over ranks of the reduced rows
 * of A.data / b since the upload, [12] LM trials since the upload that ran on rows NOT summed (nlls_sweep_gradhess(ctx, NULL) leaves them as the
 * rank's share: everything a trial takes from them is linear in them).  [13] 1: the reduced blocks are in reverse Cuthill-McKee order (0: the caller's),
 * [14] half bandwidth (dof) the caller's order would have given (-1: not computed), [15] 1: the dense LDL' (solve_mode 1) is restricted to the band of the
 * re-ordered reduced system and the border strip ("windowed": O(n w^2) work in dense storage, for bands too wide for the band kernels).
 * Tile-sparse solver (solve_mode 3): [16] tiles of 128 unknowns, [17] levels of the tile elimination tree (the dependent chain of the factorisation),
 * [18] lower tiles stored (fill included), [19] kernel launches per reduced solve, [20] 128^3 tile products per factorisation (updates + panels).
 * [21], [22] look-ahead sweeps used / thrown away; [23] matrix-free LM trials, [24] gradient sweeps of the reduced rows only, [25] full accumulate sweeps since the upload;
 * [26] unknowns per block of the block cyclic reduction (the smallest multiple of 16 that keeps the band block tridiagonal: may be below the bandwidth [5]);
 * [27], [28] variables the last nlls_optimize_singles call relaxed one per wavefront / one per thread (on this rank).
 * The branches nlls_upload_structure chose (host integers, for tests that must assert the path they were written for; on this rank):
 * elimination supernodes [29] on the fast path with at most 60 neighbour unknowns, [30] fast with 61..63, [31] fast with 64..70, [32] on the generic
 * (LDS-staged) path with pair accumulators in LDS, [33] generic without accumulators; [34] neighbour blocks of eliminated blocks that are stored in the
 * NEIGHBOUR's block row and read transposed (an eliminated variable listed before a reduced neighbour), [35] all neighbour blocks; [36] 1: the materialised
 * elimination assembles through slabs + gather (NLLS_FLAG_DETERMINISTIC took effect).  Accumulate sweep, summed over cost groups and their slots:
 * [37] light tiles, [38] heavy tiles that carry an LDS image, [39] heavy tiles that write straight to memory (rows too long for an image), [40] tiles (light or
 * heavy) whose rows are shared or split and flushed with atomics, [41] cost groups swept folded, [42] cost groups the last full accumulate sweep ran as one fused
 * launch (0 before the first sweep).  nlls_eval_jacobians / nlls_eval_gradhess: [43] doubles of LDS in which a wavefront stages its lanes' records before it
 * writes them out contiguously, [44], [45], [46] lanes of a wavefront staged at a time for the J / g / H of the last call that asked for them (64: all at once;
 * 0: stored directly, or not asked for yet).  The last matrix-free product (nlls_hess_apply, ...): [47] rows its gather summed one lane per unknown, [48] rows that
 * took a wavefront each, [49] chunks its vectors were cut into, [50] doubles of record scratch it used (nlls_jac_apply gathers nothing: 0, 0, 1, 0).
 * The chain kernels (solve_mode 2 without block cyclic reduction: bands wider than 80, NLLS_FLAG_NO_BCR), as chosen where they are launched: [51] their form -- 0: the reduced
 * solve is not theirs, 1: one persistent workgroup with the band window in registers, 2: the blocked factorisation from one end, 3: twisted (from both ends, NLLS_FLAG_NO_TWIST
 * off, no border, a separator of at most 16 ceil(bw / 16) columns) -- and [52], for form 1, the window as 1000 SEG + 10 NSLOT + CH / 8 (segment length, segments per lane,
 * columns per chunk of the HBM -> LDS ring); 0 otherwise.  The last nlls_solve_pcg: [53] iterations made, [54] its status (0 converged, 1 maxiters, 2 and 3
 * breakdown), [55] stream synchronisations it took; [47..50] then describe the last product it enqueued. */
int  nlls_get_solve_stats(nlls_ctx* ctx, int64_t* out, int32_t n);
/* Run-time switches of a context (A/B measurements, parity tests through both paths on ONE upload):
 *   NLLS_OPT_MATERIALIZE  value != 0: nlls_lm_trial eliminates from the materialised A.data (the round-5 path) although the structure qualifies for the
 *                         matrix-free trial; 0 (default): matrix-free where nlls_upload_structure found it applicable (NLLS_FLAG_MATERIALIZE: never).
 *   NLLS_OPT_LOOKAHEAD    value == 0: no look-ahead sweep behind an LM trial (the environment's NLLS_NO_LOOKAHEAD_SWEEP=1).
 *   NLLS_OPT_PHASE_EVENTS see below.
 *   NLLS_OPT_APPLY_SCRATCH  bytes of record scratch the matrix-free products may hold (default 256 MiB): a call whose vectors need more is cut into chunks of
 *                         vectors (one vector's records are always held).  NLLS_OPT_APPLY_WAVE_MIN  incidences from which an unknown's row is summed by a
 *                         wavefront of its own (default 64; values below 1 count as 1).  Both outlive an upload.
 *   NLLS_OPT_PCG_ROUND    iterations nlls_solve_pcg enqueues between two looks at its stop flag (default 1, >= 1): a longer round saves synchronisations and spends
 *                         up to round - 1 empty iterations behind the stop.  The result does not depend on it.  NLLS_OPT_PCG_GRID_MAX  most workgroups of its vector
 *                         kernels (default 1024, >= 1): longer vectors are walked with a grid-stride loop; the partial sums group by it, so results agree to
 *                         rounding, not to the bit, across values.  Both outlive an upload; values below 1: NLLS_ERR_INVALID_ARG. */
/* Device-timed NLLSResult buckets since the upload, nanoseconds: out[0] gradient, [1] cost, [2] solver, [3] trials counted (single-GPU sparse trials; others leave them untouched). */
int  nlls_get_time_buckets(nlls_ctx* ctx, int64_t* out, int32_t n);
#define NLLS_OPT_MATERIALIZE 1
#define NLLS_OPT_LOOKAHEAD   2
#define NLLS_OPT_APPLY_SCRATCH  4
#define NLLS_OPT_APPLY_WAVE_MIN 5
#define NLLS_OPT_PCG_ROUND     6
#define NLLS_OPT_PCG_GRID_MAX  7
#define NLLS_OPT_PHASE_EVENTS 3   /* value != 0: the COLLECTIVE nlls_lm_trial records stream events at its phase boundaries (resets the sums); nlls_get_phase_times reads them */
/* out[0..4]: milliseconds summed over the trials since NLLS_OPT_PHASE_EVENTS was set -- [0] this rank's assembly of [S | s] (elimination), [1] the all-reduce of [S | s] (wait included),
 * [2] the reduced solve (every rank), [3] back-substitution + retraction, [4] trial tail (statistics, cost sweep, the scalars' gather); [5] gradient sweeps (ms summed), [6] trials, [7] sweeps counted.
 * [8] milliseconds of the last nlls_set_cost_data's scatter launch alone (an event pair around it, while the option is set; waits for it), [9] the device copies of the payload the last such launch wrote.
 * [10] milliseconds of the last nlls_eval_jacobians / nlls_eval_gradhess launch alone (the same: an event pair, while the option is set), [11] the bytes of records that call's launch wrote.
 * [12] milliseconds of the last matrix-free product's launches (nlls_hess_apply, nlls_jac_apply, nlls_jact_apply, nlls_hess_block_diag: one event pair around all of them), [13] the bytes of records and output they wrote.
 * [14] milliseconds of the last nlls_solve_pcg's launches, products included (one event pair from its first launch to the launch that sets the step). */
int  nlls_get_phase_times(nlls_ctx* ctx, double* out, int32_t n);
int  nlls_set_option(nlls_ctx* ctx, int32_t option, int64_t value);
int  nlls_set_step(nlls_ctx* ctx, const double* x);               /* host-formed steps (dogleg, GD) */
int  nlls_get_step(nlls_ctx* ctx, double* x_out);
int  nlls_step_maxabs(nlls_ctx* ctx, double* out);                /* maximum(abs, linsystem.x) */
int  nlls_step_norm(nlls_ctx* ctx, double* out);                  /* norm(linsystem.x)         */
/* replaces: fast_bAb(hessian, x), dot(gradient, x)  src/iterators.jl:163, src/utils.jl:95-106.
 * Uses the CURRENT damping (the reference un-damps first, src/iterators.jl:162). */
int  nlls_quadform(nlls_ctx* ctx, double* xHx_out, double* gx_out);
/* replaces: update!(to, from, linsystem)  src/linearsystem.jl:206-213:
 * vars[to] = update(vars[from], x) for unfixed variables, copy for fixed ones. */
int  nlls_retract(nlls_ctx* ctx, int32_t to, int32_t from);
/* replaces: optimizesingles!(problem, options, indices)  src/optimize.jl:60-76,183-205.
 * Every listed variable (1-based) is optimised on its own, all others fixed, against the cost blocks that depend on it:
 * variable i owns the entries cptr[i] .. cptr[i+1]-1 (cptr[0] = 0) of (cgroup = index of the nlls_cost_group at upload,
 * cindex = 0-based position of the block inside that group, cslot = which of the block's variables it is).  No block may
 * contain two variables of ONE call (they are solved side by side, one thread each): listed variables that share a block are
 * relaxed one after the other by the reference (src/optimize.jl:183-205) -- the caller splits them into calls of independent
 * sets, in the reference's order (the Python host and the shim do).  iterator: 0 Newton, 1 Levenberg-Marquardt, 2 dogleg,
 * 3 gradient descent (src/iterators.jl), each reset per variable, with the outer loop and termination rules of
 * src/optimize.jl:109-180; operates on NLLS_VARS_CURRENT in place; iters_out (nsel, may be NULL) receives the iterations each
 * variable took.  Variables of at most NLLS_SINGLES_MAX_DOF dof.  A variable of more than 6 dof, or of at least 64 cost blocks (NLLS_SINGLES_WAVE_MIN=n in the environment of
 * nlls_ctx_create: n), is relaxed by one wavefront, whose lanes deal its blocks; every other one by one thread.  The result of a variable does not depend on which others the
 * call lists. */
int  nlls_optimize_singles(nlls_ctx* ctx, int64_t nsel, const int64_t* varindices, const int64_t* cptr, const int32_t* cgroup, const int64_t* cindex,
                           const int32_t* cslot, int32_t iterator, int32_t maxiters, int32_t maxfails, double reldcost, double absdcost, double dstep, int64_t* iters_out);
/* The Levenberg-Marquardt outer loop itself, on the host side of this ABI (csrc/nlls_lm.cpp): up to `niter` passes of the while-loop body
 * of optimizeinternal! (src/optimize.jl:124-171) with iterate!(::LevMarData) (src/iterators.jl:139-172) inside -- written only in terms of
 * the entry points of this header, i.e. the loop a binding would write, without an interpreter between two trials (the GPU waits for the
 * host there).  Before the first call: variables in NLLS_VARS_CURRENT and NLLS_VARS_NEXT, nlls_sweep_gradhess done, state zeroed except
 * bestcost = that sweep's cost.  Stops early when the termination flags (src/optimize.jl:147-158, bits 0-9) of an iteration are not 0:
 * they are left in state->converged.  The caller finishes like src/optimize.jl:173-176 (best variables back if !(bestcost >= cost)).
 * A host that has a per-iteration callback calls it with niter = 1.  Single GPU (it drives nlls_lm_trial). */
typedef struct nlls_lm_options {
    double  reldcost, absdcost, dstep;
    int64_t maxfails, maxiters;
    int64_t stoptime_ns;            /* CLOCK_MONOTONIC deadline in ns (starttime + maxtime); <= 0: none */
} nlls_lm_options;
typedef struct nlls_lm_state {
    double  lambda;                 /* LevMarData.lambda; 0: initialised from max|H_ii| * 1e-6 (src/iterators.jl:131-144) */
    double  bestcost, cost;         /* data.bestcost; cost returned by the last iteration */
    int64_t iternum, fails, have_best, converged;
    int64_t linearsolvers, costcomputations, gradientcomputations, singulartrials;
    int64_t timesolver_ns, timegradient_ns;
    int64_t timecost_ns;            /* (round 6, appended) NLLSResult.timecost (src/structs.jl:43, src/iterators.jl:157).  The three buckets are DEVICE times where the trials' launches
                                     * time themselves (nlls_get_time_buckets): solver = start of the assembly launch .. start of the cost launch, cost = .. end of the finishing
                                     * workgroup, gradient = end of a trial .. start of the next (the sweep between them and the host's turn-around).  Matrix-free trial: the cost
                                     * blocks are evaluated INSIDE the assembly and back-substitution launches, so their evaluation is booked under solver, and cost is the finishing
                                     * workgroup alone. */
} nlls_lm_state;
int  nlls_lm_iterations(nlls_ctx* ctx, const nlls_lm_options* options, nlls_lm_state* state, int64_t niter);
/* One Levenberg-Marquardt trial (src/iterators.jl:149-157) in one call and one synchronisation:
 * nlls_damp(dlambda); nlls_solve; nlls_retract(to, from); nlls_sweep_cost(to) -> *cost_out.  Same kernels in the same
 * order; the step statistics and the quadratic form of the step are answered from the host afterwards.  Single GPU only. */
int  nlls_lm_trial(nlls_ctx* ctx, double dlambda, int32_t to, int32_t from, double* cost_out);

/* ---- multi-GPU ----------------------------------------------------------------------
 * One process per GPU; nlls_set_shard(rank, nranks) BEFORE nlls_upload_structure.  Every rank uploads the
 * SAME full problem; the library keeps only the cost blocks this rank owns (a cost belongs to the rank
 * that owns its eliminated variable: contiguous ranges of eliminated blocks balanced by cost count).
 * Device buffers the caller sums over ranks (RCCL all-reduce over xGMI; pointers stay valid until the next
 * upload):
 *   stage 0  after nlls_sweep_gradhess_local : [cost | reduced-block rows of A.data | reduced part of b]
 *   stage 1  after nlls_solve_local          : [S | s]   the reduced system
 *   stage 2  after nlls_solve_finish         : x         (each rank holds its own eliminated blocks, rank 0 the rest)
 * nlls_sweep_gradhess_local and nlls_solve_local only ENQUEUE on the context's stream (nlls_set_stream): their buffers are
 * complete in stream order -- issue the collective on that stream, or synchronise it first.  nlls_sweep_gradhess_finish
 * with cost_out = NULL does not synchronise either; nlls_solve_finish does (it reports the factorisation status).
 * With nranks > 1, nlls_sweep_cost, nlls_quadform, nlls_grad_sqnorm, nlls_grad_quadform return this rank's
 * PARTIAL sums and nlls_max_abs_diag its partial maximum: the caller reduces those scalars itself. */
int  nlls_sweep_gradhess_local(nlls_ctx* ctx);
int  nlls_sweep_gradhess_finish(nlls_ctx* ctx, double* cost_out);
int  nlls_sweep_cost_local(nlls_ctx* ctx, int32_t which);
int  nlls_sweep_cost_finish(nlls_ctx* ctx, double* cost_out);
int  nlls_solve_local(nlls_ctx* ctx);
int  nlls_solve_finish(nlls_ctx* ctx, double* x_out);
/* after the stage-2 reduction (x complete): update!(to, from, x), cost(to), fast_bAb(H, x), dot(g, x), max|x|, |x|^2 of one
 * Levenberg-Marquardt trial (src/iterators.jl:155-163) with one synchronisation.  out[6] = [cost, x'Hx, g'x, max|x|, |x|^2, status]:
 * with nranks > 1 all of them are this rank's share (sum the first three and the fifth, take the maximum of the fourth and of the
 * factorisation status, and fail on EVERY rank when that is not 0); with one rank out[5] is not written and a bad pivot is an error.
 * out = NULL: enqueue only, no synchronisation -- the scalars stay on the device as reduce buffer 3 (eleven doubles: [0] cost, [8] x'Hx,
 * [5] g'x, [1] max|x|, [9] |x|^2 of this rank's share, [10] status), to be all-GATHERED on the device: a sharded trial then synchronises once. */
int  nlls_trial_local(nlls_ctx* ctx, int32_t to, int32_t from, double* out);   /* also reports a failed factorisation of the solve before it */
/* nlls_solve_finish without the synchronisation: for the step of an LM trial, whose status nlls_trial_local reports */
int  nlls_solve_finish_replicated(nlls_ctx* ctx);   /* ... and with the reduced part of the step on EVERY rank: no stage-2 reduction; each rank
                                                      retracts the reduced variables and its own eliminated ones (nlls_trial_local) */
/* this rank's share of a variable set (its own eliminated blocks' variables; rank 0: also all others), zeros elsewhere: sum over ranks */
int  nlls_get_variables_owned(nlls_ctx* ctx, int32_t which, double* packed);
int  nlls_solve_finish_async(nlls_ctx* ctx);
int  nlls_get_reduce_buffer(nlls_ctx* ctx, int32_t stage, void** dev_ptr, int64_t* count);
int  nlls_get_step_shard(nlls_ctx* ctx, void** dev_ptr_x, int64_t* reduced_count,
                         int64_t* own_offset, int64_t* own_count);
/* [0] rank, [1] nranks, [2] cost blocks owned, [3] doubles of A.data this rank writes, [4] dof of b it writes, [5] (n >= 6) 0, or -- REPLICAS -- the nranks of
 * nlls_set_shard: the uploaded problem does not shard (a dense system, or no eliminated variable set to partition by); every rank runs the whole problem as rank 0
 * of 1, no entry point enters a collective, every rank holds the complete result ([0], [1] then read 0, 1) */
int  nlls_get_shard_info(nlls_ctx* ctx, int64_t* out, int32_t n);
/* this rank's share of the gradient b (length ndof): the rows of the eliminated blocks it owns, the reduced rows on
 * rank 0, zeros elsewhere -- the sum over ranks is the full gradient that gethessgrad (src/linearsystem.jl:190) hands to
 * the dogleg / gradient-descent iterators (src/iterators.jl:48,191).  nranks == 1: identical to nlls_get_grad. */
int  nlls_get_grad_owned(nlls_ctx* ctx, double* b_out);

/* ---- profiling helper: run the accumulate kernel(s) `reps` times between two HIP events on the
 * context's stream; returns average ms per sweep (used by bench.py for the roofline line). */
int  nlls_time_sweep_gradhess(nlls_ctx* ctx, int32_t reps, float* ms_avg);
int  nlls_time_sweep_accumulate(nlls_ctx* ctx, int32_t reps, float* ms_avg);   /* the accumulate launches alone (what nlls_sweep_gradhess(ctx, NULL) enqueues) */
int  nlls_time_sweep_cost(nlls_ctx* ctx, int32_t reps, float* ms_avg);
int  nlls_time_solve(nlls_ctx* ctx, int32_t reps, float* ms_avg);
/* in-situ timing of the accumulate launches: on != 0 starts recording an event pair around every nlls_sweep_gradhess's accumulate
 * launch(es) inside the caller's own loop (last 64 kept); a call with any output pointer set synchronises and reports them. */
int  nlls_profile_sweep(nlls_ctx* ctx, int32_t on, float* ms_avg, float* ms_min, float* ms_max, int64_t* nsamples);
/* ... the same launches by their DISPATCH timestamps (begin .. end as the command processor records them for the launch: hipExtLaunchKernelGGL's
 * start / stop events) -- the duration rocprofv3 --kernel-trace reports per dispatch, measured inside the caller's own loop; read-only, synchronises. */
int  nlls_profile_sweep_dispatch(nlls_ctx* ctx, float* ms_avg, float* ms_min, float* ms_max, int64_t* nsamples);
int  nlls_time_reduced_solve(nlls_ctx* ctx, int32_t reps, float* ms_avg);  /* factorisation + backward pass of the (already assembled) reduced system alone */
/* measurement helpers.  nlls_get_memory_info: out[0] = bytes of the LM loop's working set (every device buffer an iteration reads or writes -- the
 * "hot arena"), out[1] = bytes reserved for it in one allocation (0: NLLS_NO_ARENA), out[2] = bytes of A.data, out[3] = bytes of the reduced system [S | s],
 * out[4] (n >= 5) = bytes of it a sharded trial sums over ranks (tile-sparse solver: the assembled tiles and s -- the fill tiles are zero until the factorisation).
 * nlls_flush_cache: streams `bytes` of foreign data through the memory side on the context's stream (a device-to-device copy between two scratch
 * halves): whatever the 256 MiB Infinity Cache held of the working set is gone afterwards -- a launch timed behind it is the COLD figure. */
int  nlls_get_memory_info(nlls_ctx* ctx, int64_t* out, int32_t n);
/* test hook (round 5): residual kinds may bring their Jacobian in closed form (the pinhole kinds) and the adaptive kernel's second derivatives are taken in
 * closed form -- the generic statement through dual numbers (/root/reference/src/autodiff.jl:81-93,164-165) stays in the library as the check.  Evaluates every
 * block of the uploaded problem at NLLS_VARS_CURRENT both ways; out[0..6] = largest difference of J, J'r, cost, rho', rho'', d rho / d kernel,
 * d2 rho / d kernel d(kernel, cost), each relative to the largest magnitude of that quantity in its block.  n >= 7. */
int  nlls_check_analytic(nlls_ctx* ctx, double* out, int32_t n);
/* robustify / robustifydcost (src/robust.jl) of a robust kernel (robust_kind and params as in nlls_cost_group) at n costs, evaluated on the device by the
 * functions every kernel of the path calls: out[4 i + 0] = robustify(cost[i]), out[4 i + 1 .. 3] = robustifydcost's (rho, rho', rho'').  Needs no upload;
 * an id the library does not have is NLLS_ERR_UNSUPPORTED. */
int  nlls_robustify(nlls_ctx* ctx, int32_t robust_kind, const double params[4], int64_t n, const double* cost, double* out);
int  nlls_flush_cache(nlls_ctx* ctx, int64_t bytes);

/* ---- collectives behind the ABI ("RCCL all-reduce over xGMI on the assembled normal equations") ----------------------
 * Under nlls_set_shard(rank, nranks) the entry points of the Levenberg-Marquardt loop -- nlls_sweep_gradhess, nlls_max_abs_diag,
 * nlls_lm_trial, nlls_sweep_cost, nlls_quadform, nlls_grad_sqnorm, and therefore nlls_lm_iterations -- become COLLECTIVE once an
 * all-reduce is installed: every rank calls them in the same order, the library reduces [cost | camera rows | camera part of b] after a
 * gradient sweep, [S | s] after the local elimination and the trial's scalars (gathered, with the factorisation status: a rank-local bad
 * pivot fails the call on EVERY rank) on its own stream, and returns the reduced values.  No host language stands between two trials.
 * Replaces nothing in the reference (single process); the loop driven is src/optimize.jl:124-171.
 *   nlls_comm_unique_id / nlls_comm_init_rccl : RCCL inside the library (librccl.so.1 is loaded on first use; one communicator per
 *                         context, collectives on the context's stream).  id: 128 bytes from rank 0, handed to every rank by the caller.
 *   nlls_set_allreduce  : any other transport -- fn reduces `count` doubles at dev_ptr (device memory) in place over all ranks, ordered
 *                         behind the work already enqueued on hip_stream and before work enqueued on it afterwards (a host-staged
 *                         implementation synchronises the stream itself); returns 0 on success.  fn == NULL removes it. */
#define NLLS_REDUCE_SUM 0
#define NLLS_REDUCE_MAX 1
typedef int (*nlls_allreduce_fn)(void* user, void* dev_ptr, int64_t count, int32_t op, void* hip_stream);
int  nlls_set_allreduce(nlls_ctx* ctx, nlls_allreduce_fn fn, void* user);
int  nlls_comm_unique_id(void* id128);
int  nlls_comm_init_rccl(nlls_ctx* ctx, const void* id128);
/* A termination word the ranks agree on WITHOUT a collective of its own (src/optimize.jl:158 compares the wall clock with starttime + maxtime:
 * under sharding every rank has its own clock, and a rank that leaves the loop alone leaves its peers inside the next trial's collectives).
 *   nlls_comm_post_flag(v)            : this rank's value (>= 0) rides in its row of the NEXT nlls_lm_trial's scalar gather;
 *   nlls_comm_agreed_flag(local, out) : *out = the MAXIMUM over ranks of the values posted before the last nlls_lm_trial -- the same number on
 *                                       every rank; without an installed all-reduce (one process) *out = local, the caller's own value now.
 * nlls_lm_iterations posts `now > stoptime` at the top of every outer iteration and stops on the agreed value: all ranks leave in the same
 * iteration, at most one iteration after the first of them crossed the deadline. */
int  nlls_comm_post_flag(nlls_ctx* ctx, double value);
int  nlls_comm_agreed_flag(nlls_ctx* ctx, double local_value, double* out);
/* what the library's own communicator reports (RCCL: ncclCommCount / ncclCommUserRank / ncclCommCuDevice), not what the launcher's
 * environment says: out[0] = ranks in the communicator, out[1] = this rank, out[2] = its device, out[3] = 1 RCCL inside the library /
 * 2 a caller-installed all-reduce / 0 none (then out[0] = 1, out[1] = 0).  n >= 4. */
int  nlls_comm_info(nlls_ctx* ctx, int64_t* out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* NLLS_AMD_H */
