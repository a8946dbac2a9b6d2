// nlls_switches.hpp -- every environment switch of the library, in one table.  Standard library only: no other file of csrc/ reads the environment.
// All are A/B or parity switches.  Each is read at one of two moments: when a context is created (read_create_env) or at every upload (read_upload_env).
#pragma once

#include <cstdint>
#include <cstdlib>

namespace nlls {

struct Switches {
    // ---- read when the context is created; the run-time options write some of them later, and no upload reads them again -------------------------------
    bool spec_on = true;               // the look-ahead sweep behind an LM trial
    bool mf_on = true;                 // the matrix-free LM trial where the structure qualifies
    bool tiny_dense_on = true;         // the small dense system's own route
    bool post_fuse = true;             // materialised trial: retraction inside the back-substitution launch, step statistics inside the cost sweep's
    bool elim_split = false;           // materialised trial: the assembly of the reduced system in one launch per supernode class
    bool dense_fused_bwd = true;       // dense LDL': the backward substitution in one launch
    int dense_t128_min = 16;           // dense LDL': 128 x 128 trailing-update tiles while at least this many 128-row blocks are left
    int64_t singles_wave_min = 64;     // optimizesingles: cost blocks from which a variable of at most 6 dof gets a wavefront instead of a thread
    // ---- read at every upload: they hold for that upload's structure ------------------------------------------------------------------------------------------
    bool no_arena = false;             // no hot arena (one allocation for the loop's working set)
    int sweep_fold = -1;               // folded sweep: 0 never, 1 for every qualifying group, -1 for groups of three or more slots
    int heavy_max_entries = 1024;      // entries per heavy tile (two wavefronts x 8 pipeline stages); longer rows are split
    int supernode_piece = 0;           // cut runs of eliminated blocks into pieces of this many (0: balanced automatically)
    bool bcr_nt_full = false;          // block cyclic reduction: blocks of 16 ceil(bw / 16) unknowns instead of the smallest size the structure keeps block tridiagonal
    bool bcr_level_backward = false;   // ... one backward launch per level instead of one fused launch
    int bcr_chrows_slots = 256;        // ... workgroup slots a panel launch may fill with one X row per workgroup (0: always three rows)
    int cost_grid_max = 2048;          // workgroups of the cost sweep
    int dense_dch1 = 256;              // dense LDL': one-row panels up to this many tile rows, one round of a 256-CU chip (0: two rows per workgroup everywhere)
    bool no_dense_window = false;      // dense LDL' never windowed
    bool no_tsparse = false;           // tile-sparse solver never ...
    bool force_tsparse = false;        // ... or always, instead of the upload's cost model
    int tsp_leaf = 256;                // tile-sparse: unknowns up to which a part is not cut further (two tiles)
    int tsp_carry = 80;                // ... rows of a part's last tile up to which it is carried up into its separator (0: never)
    int tsp_scheme = 0;                // ... panel scheme 1 / 2 / 3 for every level (0: chosen per level)
    int tsp_slots = 256;               // ... workgroups of one round of the chip
    int tsp_quad_max = 160;            // ... target tiles of a level up to which an update workgroup takes a quarter tile
    int tsp_cap = 0;                   // ... products of one target tile that a workgroup walks at most (0: from the level's size)
    bool tsp_no_masks = false;         // ... every tile product in full
};

// the parse rules.  atoi throughout: text that is not a number reads as 0
namespace env {
inline bool is_set(const char* name) { return std::getenv(name) != nullptr; }                                                  // any value, the empty one included
inline bool starts_with(const char* name, char ch) { const char* e = std::getenv(name); return e && e[0] == ch; }
inline int integer(const char* name, int unset) { const char* e = std::getenv(name); return e ? std::atoi(e) : unset; }        // every integer is a value, 0 and negative ones too
inline int at_least(const char* name, int lowest, int otherwise) { const int v = integer(name, lowest - 1); return v >= lowest ? v : otherwise; }
inline int64_t positive64(const char* name, int64_t otherwise) { const char* e = std::getenv(name); const long long v = e ? std::atoll(e) : 0; return v > 0 ? (int64_t)v : otherwise; }
}  // namespace env

inline void read_create_env(Switches& s) {
    const Switches d;
    s.spec_on          = !env::starts_with("NLLS_NO_LOOKAHEAD_SWEEP", '1');
    s.mf_on            = !env::starts_with("NLLS_MATERIALIZE", '1');
    s.tiny_dense_on    = !env::starts_with("NLLS_TINY_DENSE", '0');
    s.post_fuse        = !env::starts_with("NLLS_POST_SPLIT", '1');
    s.elim_split       =  env::starts_with("NLLS_ELIM_SPLIT", '1');
    s.dense_fused_bwd  = !env::starts_with("NLLS_DENSE_STEP_BACKWARD", '1');
    s.dense_t128_min   =  env::integer("NLLS_DENSE_T128_MIN", d.dense_t128_min);
    s.singles_wave_min =  env::positive64("NLLS_SINGLES_WAVE_MIN", d.singles_wave_min);
}

inline void read_upload_env(Switches& s) {
    const Switches d;
    s.no_arena           = env::is_set("NLLS_NO_ARENA");
    s.sweep_fold         = env::integer("NLLS_SWEEP_FOLD", d.sweep_fold);
    s.heavy_max_entries  = env::at_least("NLLS_HEAVY_MAX_ENTRIES", 128, d.heavy_max_entries);
    s.supernode_piece    = env::integer("NLLS_SUPERNODE_PIECE", d.supernode_piece);
    s.bcr_nt_full        = env::is_set("NLLS_BCR_NT_FULL");
    s.bcr_level_backward = env::starts_with("NLLS_BCR_LEVEL_BACKWARD", '1');
    s.bcr_chrows_slots   = env::integer("NLLS_BCR_CHROWS_SLOTS", d.bcr_chrows_slots);
    s.cost_grid_max      = env::at_least("NLLS_COST_GRID_MAX", 1, d.cost_grid_max);
    s.dense_dch1         = env::integer("NLLS_DENSE_DCH1", d.dense_dch1);
    s.no_dense_window    = env::is_set("NLLS_NO_DENSE_WINDOW");
    s.no_tsparse         = env::is_set("NLLS_NO_TSPARSE");
    s.force_tsparse      = env::is_set("NLLS_FORCE_TSPARSE");
    s.tsp_leaf           = env::at_least("NLLS_TSP_LEAF", 1, d.tsp_leaf);
    s.tsp_carry          = env::integer("NLLS_TSP_CARRY", d.tsp_carry);
    s.tsp_scheme         = env::integer("NLLS_TSP_SCHEME", d.tsp_scheme);
    s.tsp_slots          = env::integer("NLLS_TSP_SLOTS", d.tsp_slots);
    s.tsp_quad_max       = env::integer("NLLS_TSP_QUAD_MAX", d.tsp_quad_max);
    s.tsp_cap            = env::integer("NLLS_TSP_CAP", d.tsp_cap);
    s.tsp_no_masks       = env::is_set("NLLS_TSP_NO_MASKS");
}

}  // namespace nlls
