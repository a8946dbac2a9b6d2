// nlls_state.hpp -- the events that change what nlls_ctx knows of its device buffers: lin, ahead, step, zero, fin (nlls_ctx.hpp states what each holds).
// Nothing else assigns those fields (included at the end of nlls_internal.hpp).  The events, and what each invalidates:
//   upload_started        everything but the look-ahead counters
//   sweep_enqueued        A and b become the swept set's linearisation, formed to the level swept: the step's statistics, E_v s and a matrix-free tail were of the old
//   sweep_asked           the caller asks for CURRENT's linearisation: a pending look-ahead sweep is consumed, CURRENT is fresh, the look-ahead is re-armed
//   new_linearisation     the caller holds it (damping from zero; the timing entries keep theirs); defer_linearisation: nothing of it is formed yet (matrix-free)
//   drop_lookahead        a sweep outside the look-ahead protocol (the _local pair, the timing entries): a pending look-ahead sweep is dropped uncounted
//   enqueue_lookahead     the look-ahead sweep of the trial point, behind the trial's finishing launch (which zero-filled its rows: zero.heavy_rows is used up)
//   lookahead_consume     CURRENT's linearisation is needed while a look-ahead sweep is pending: after the swap of an accepted trial it IS that (a hit); otherwise (a miss)
//                         nothing of A and b counts as formed -- the current point is swept again, the damping kept -- and the look-ahead rests until the next sweep asked for
//   vars_written          a variable set is about to be written (relaxed: nlls_optimize_singles changes it under the linear system); new_starting_point: CURRENT set
//   costs_changed         the cost blocks' data or a group's robust parameters were replaced (nlls_set_cost_data, nlls_set_robust_params): no linearisation is held
//   step_replaced         the caller writes x: nothing known of the last solve's step holds
//   backsub_done, mf_backsub_done, step_solved   a solve's back-substitution wrote x (and S or the tiles); the host has read the step's statistics
//   take_mf_tail          a trial's tail finishes the matrix-free step whose sets it retracts, and drops it otherwise (other sets, or a set written since)
//   take / drop           one fact is used up by the work it saves (a memset, a retraction, a finishing launch) / no longer holds
#pragma once

namespace nlls {

[[nodiscard]] inline bool take(bool& fact) { const bool f = fact; fact = false; return f; }
inline void drop(bool& fact) { fact = false; }
inline void upload_started(nlls_ctx* c) { const Lookahead a = c->ahead; c->lin = {}; c->ahead = {}; c->step = {}; c->zero = {}; c->fin = {}; c->lambda = 0; c->ahead.hits = a.hits; c->ahead.misses = a.misses; }

// ---- the linearisation ----------------------------------------------------------------------------------------------
inline void sweep_enqueued(nlls_ctx* c, int which, int level) { c->lin.level = level; c->lin.phys = c->vars_slot[which]; c->step.tE_valid = c->step.cached = c->step.mf = false; }
inline bool lookahead_consume(nlls_ctx* c, bool usable) {      // (`usable`: the caller can take the look-ahead sweep's linearisation)
    if (!c->ahead.pending) return false;
    const bool hit = usable && !c->ahead.stale && c->lin.phys == c->vars_slot[NLLS_VARS_CURRENT]; c->ahead.pending = c->ahead.stale = false;
    if (hit) c->ahead.hits++; else { c->ahead.misses++; c->ahead.armed = false; c->lin.level = 0; }
    return hit;
}
// (a sweep the caller asks for: the look-ahead may try again behind the next trial -- but not behind the FIRST trial from a new starting point: the initial damping
//  (1e-6 of the largest diagonal entry, src/iterators.jl:131-137) is the one guess of the loop that is routinely rejected -- five times in a row at BASELINE config 5 --,
//  and a look-ahead behind it is a sweep thrown away plus the current point swept again.  Returns whether the look-ahead sweep is the linearisation asked for: with the
//  cost wanted it is not.  A miss zeroes lin.level, which the sweep that follows sets again.)
inline bool sweep_asked(nlls_ctx* c, bool want_cost) { const bool hit = lookahead_consume(c, !want_cost); c->ahead.armed = c->ahead.sweeps_since_set++ >= 1; c->lin.stale_point = false; return hit; }
inline void new_linearisation(nlls_ctx* c, bool summed = true, bool reset_lambda = true) { if (reset_lambda) c->lambda = 0.0; c->lin.have = true; c->lin.summed = summed; }
// (matrix-free LM trial: between two iterations nothing is enqueued -- the first call that needs the linearisation says how much of it, and it is formed then, at CURRENT)
inline void defer_linearisation(nlls_ctx* c) { c->lin.level = 0; c->lin.phys = c->vars_slot[NLLS_VARS_CURRENT]; c->step.tE_valid = c->step.cached = false; new_linearisation(c); }
inline void drop_lookahead(nlls_ctx* c, bool fresh_point) { c->ahead.pending = c->ahead.stale = false; if (fresh_point) c->lin.stale_point = false; }
inline int enqueue_lookahead(nlls_ctx* c, int which, int mode) {     // (the small dense system's trial never sets zero.heavy_rows: clearing it there is a no-op)
    const int rc = enqueue_sweep_gradhess(c, false, which, mode); c->zero.heavy_rows = false;
    if (rc == NLLS_OK) { c->ahead.pending = true; c->ahead.stale = false; }
    return rc;
}
// ---- the variables ----------------------------------------------------------------------------------------------------
// A look-ahead sweep of the set written is stale, and so is a linearisation at it that is not (fully) formed yet; a matrix-free trial's point and cost are of the
// sets as they were (its tail is not finished again).  `relaxed`: nothing of the linear system or of a look-ahead sweep of this very set holds.
inline int vars_written(nlls_ctx* c, int which, bool relaxed = false) {
    c->step.mf = false;
    if (relaxed) { c->lin.have = false; c->lin.level = 0; c->ahead.pending = c->ahead.stale = false; c->step.cached = c->step.tE_valid = false; return NLLS_OK; }
    if (c->vars_slot[which] != c->lin.phys) return NLLS_OK;
    if (c->ahead.pending) c->ahead.stale = true;
    else if (which == NLLS_VARS_CURRENT && c->lin.have && c->mf_ok) {
        // CURRENT under the linearisation of the last nlls_sweep_gradhess (include/nlls_amd.h): the trial that follows takes A and b of the values BEFORE this write. What the
        // matrix-free path has not formed yet is formed now, in stream order ahead of the write, and its trial -- the eliminated rows evaluated at CURRENT -- is off until the
        // next sweep.  (No LM loop gets here: it writes NEXT, swaps, and sweeps again.)
        if (c->lin.level < 2) { const int rc = enqueue_sweep_gradhess(c, false, NLLS_VARS_CURRENT, 0); if (rc != NLLS_OK) return rc; }
        c->lin.stale_point = true;
    }
    else if (c->lin.level < 2) c->lin.level = 0;    // (what is formed on demand would be formed at the NEW values: the caller sweeps again after writing CURRENT -- every iterator does)
    return NLLS_OK;
}
// ---- the costs ---------------------------------------------------------------------------------------------------------
// The problem itself changed under the linear system, as vars_written(relaxed) has it for the variables: A and b are of the old costs -- the caller sweeps again before anything
// reads them (NLLS_ERR_NOT_READY until then, as after an upload) --, a pending look-ahead sweep read the old data and is dropped uncounted, the step's cached statistics, E_v s and
// a matrix-free tail are of the old system.  The variables, lambda, the counters, the known-zero scratch and deferred finishing work (none outlives its nlls_lm_trial) stay.
inline void costs_changed(nlls_ctx* c) { c->lin.have = false; c->lin.level = 0; c->ahead.pending = c->ahead.stale = false; c->step.cached = c->step.tE_valid = c->step.mf = false; }
inline void new_starting_point(nlls_ctx* c) { c->ahead.sweeps_since_set = 0; }     // (its first trial gets no look-ahead sweep: sweep_asked)
// ---- the step, and finishing work deferred to the next launch ---------------------------------------------------------------
inline void step_replaced(nlls_ctx* c) { c->step.tE_valid = c->step.cached = c->step.mf = false; }
inline void step_solved(nlls_ctx* c, bool status_read) {     // (status_read: nothing has touched the device's status word since, the next solve need not reset it)
    const double* h = c->h_scalars; StepState& s = c->step; s.cached = true; s.maxabs = h[1]; s.sumsq = h[2]; s.gx = h[5]; s.xAx = h[8]; s.xx = h[9];
    if (status_read) c->zero.status = (int32_t)h[10] == 0;
}
// (the matrix-free back-substitution always retracts; `fast`: the fast back-substitution ran, kept E_v s and zero-filled the tiles -- or S, if `zero_S` -- for the next solve)
inline void mf_backsub_done(nlls_ctx* c, int to, int from) { StepState& s = c->step; s.tE_valid = false; s.mf = s.retract_done = true; s.mf_to_phys = c->vars_slot[to]; s.mf_from_phys = c->vars_slot[from]; c->zero.tiles = true; }
inline void backsub_done(nlls_ctx* c, bool fast, bool tiles_direct, bool zero_S, bool retracted) {
    c->step.mf = false; c->step.retract_done = retracted;
    if (fast) { c->step.tE_valid = true; if (tiles_direct) c->zero.tiles = true; else c->zero.S = zero_S; }
}
inline bool take_mf_tail(nlls_ctx* c, int to, int from) {
    if (c->step.mf) { c->step.retract_done = false; c->step.mf = c->vars_slot[to] == c->step.mf_to_phys && c->vars_slot[from] == c->step.mf_from_phys; }
    return c->step.mf;
}
inline void heavy_rows_zeroed(nlls_ctx* c) { c->zero.heavy_rows = true; }   // (by the trial's finishing launch: the look-ahead sweep behind it skips its zero fill once)
inline void defer_dense_fin(nlls_ctx* c, const DenseFin& f) { c->fin.dense = f; c->fin.dense_pending = true; }
inline void defer_mf_fin(nlls_ctx* c) { c->fin.mf_pending = true; }

}  // namespace nlls
