// msda_knobs.h -- host only, no HIP: the test / measurement knobs and the table of pinned routes (msda_knobs.hip).
#pragma once

#include <string>

#include "msda_params.h"

namespace msda {

// ---- test / measurement knobs -------------------------------------------------------------------------------
// All of them are environment variables that are read ONCE (first call into the library, or msda_reload_knobs())
// and only when MSDA_ENABLE_HOOKS=1: a production process cannot have its results or speed changed by a stray
// variable, and the launch path does not call getenv.  tests/ and bench.py set MSDA_ENABLE_HOOKS=1 and call
// msda_reload_knobs() after changing a knob.  Each knob is one row of kKnobs below.
struct Knobs {
    int fwd_rs = -1, fwd_rs_nt = 0;     // resident-slab forward: -1 auto, 0 off, 1 force; tiles per wave (0 = auto)
    int bwd_rs = -1, bwd_rs_tpw = 0;    // resident-slab gather pass: -1 auto, 0 off, 1 force; tiles per wave (0 = auto)
    int fwd_tile_waves = -1;            // forward tile kernel: waves per tile (-1 auto)
    int bwd_rs_fsplit = -1;             // gather pass with one source frame per workgroup: parts per (clip, head, frame); -1 auto, 0 off
    int fwd_win = -1, bwd_win = -1;     // resident-window kernels (encoder-shaped calls): -1 auto, 0 off, 1 force
    int win_min_halo = 5;               // narrowest halo a window plan may have; one staging phase is preferred from here on (5 holds
                                        // the reference's initial offsets, <= 4 pixels of every level: ms_deform_attn.py:64-76)
    int bwd_atomic = 0;                 // MSDA_BWD_MODE=atomic: one-kernel backward with global atomics
    int bwd_phases = 3;                 // 1 = gather pass only, 2 = scatter pass only, 3 = both
    int bwd_cull = 1;                   // 0: no culling structure, 2: (min, max) intervals instead of per-point records
    int bwd_all_records = 0;            // measurement: the gather pass leaves records for every level (a later scatter-only call may walk them)
    int scatter_lds_kb = 144;
    int scatter_dbg = 0;                // MSDA_SCATTER_DBG without kSdbgOrderMask: the bits the planner and the scatter kernels read (table: msda_params.h)
    int scatter_order = 0;              // owner-computes scatter's item order: 0 = rule, 1 = level order (MSDA_SCATTER_DBG kSdbgLevelOrder),
                                        // 2 = image order wherever the bands can be sorted (kSdbgImageOrder)
    int scatter_own = -1;               // owner-computes scatter: -1 auto, 0 off (the LDS-atomic scatter instead)
    int scatter_mfma = -1;              // matrix-pipe scatter of the coarse levels (msda_mfma.hip): -1 auto, 0 off, 1 wherever it applies
    int scatter_part = 0;               // measurement: 1 = only the owner-computes kernel of a scatter that runs both, 2 = only the matrix-pipe kernel
    int force_generic = 0;
    int det_route = 0;                  // MSDA_GRAD_DETERMINISTIC grad_value: 0 auto, 1 = route (a) (any shape), 2 = route (b) (LDS bands)
    int dbg = 0;                        // MSDA_DBG: tile kernels and launcher (kDbg*, msda_params.h)
    int walk = -1;                      // resident-slab gather pass: -1 = the planner's size rule (msda_params.h, kWalkDownBytes), 0 = every XCD
                                        // takes its workgroups first to last, 1 = last to first.  Results kept
    unsigned forced = 0;                // bit i: the variable of kKnobs[i] was SET in the environment, whatever its value: a knob
                                        // forced to its default (MSDA_FWD_RS=-1 for a rules-only A/B run) still wins over a pin
};

// How a variable's text becomes the knob's value.
enum class Parse { Int, IsOne, IsAtomic, DbgBits, OrderBits };
struct KnobDef {
    const char *env;                    // environment variable
    const char *pin;                    // name in msda_pin_route settings, or null: not pinnable
    int Knobs::*field;
    Parse parse;
};
inline const KnobDef kKnobs[] = {
    {"MSDA_FWD_RS", "fwd_rs", &Knobs::fwd_rs, Parse::Int},
    {"MSDA_FWD_RS_NT", "fwd_rs_nt", &Knobs::fwd_rs_nt, Parse::Int},
    {"MSDA_FWD_WIN", "fwd_win", &Knobs::fwd_win, Parse::Int},
    {"MSDA_FWD_TILE_WAVES", "fwd_tile_waves", &Knobs::fwd_tile_waves, Parse::Int},
    {"MSDA_BWD_RS", "bwd_rs", &Knobs::bwd_rs, Parse::Int},
    {"MSDA_BWD_RS_TPW", "bwd_rs_tpw", &Knobs::bwd_rs_tpw, Parse::Int},
    {"MSDA_BWD_RS_FSPLIT", "bwd_rs_fsplit", &Knobs::bwd_rs_fsplit, Parse::Int},
    {"MSDA_BWD_WIN", "bwd_win", &Knobs::bwd_win, Parse::Int},
    {"MSDA_SCATTER_DBG", "scatter_order", &Knobs::scatter_order, Parse::OrderBits},
    {"MSDA_SCATTER_MFMA", "scatter_mfma", &Knobs::scatter_mfma, Parse::Int},
    {"MSDA_WIN_MIN_HALO", nullptr, &Knobs::win_min_halo, Parse::Int},
    {"MSDA_BWD_MODE", nullptr, &Knobs::bwd_atomic, Parse::IsAtomic},
    {"MSDA_BWD_PHASES", nullptr, &Knobs::bwd_phases, Parse::Int},
    {"MSDA_BWD_CULL", nullptr, &Knobs::bwd_cull, Parse::Int},
    {"MSDA_BWD_ALL_RECORDS", nullptr, &Knobs::bwd_all_records, Parse::Int},
    {"MSDA_SCATTER_LDS_KB", nullptr, &Knobs::scatter_lds_kb, Parse::Int},
    {"MSDA_SCATTER_DBG", nullptr, &Knobs::scatter_dbg, Parse::DbgBits},
    {"MSDA_SCATTER_OWN", nullptr, &Knobs::scatter_own, Parse::Int},
    {"MSDA_SCATTER_PART", nullptr, &Knobs::scatter_part, Parse::Int},
    {"MSDA_FORCE_GENERIC", nullptr, &Knobs::force_generic, Parse::IsOne},
    {"MSDA_DET_ROUTE", nullptr, &Knobs::det_route, Parse::Int},
    {"MSDA_DBG", nullptr, &Knobs::dbg, Parse::Int},
    {"MSDA_WALK", nullptr, &Knobs::walk, Parse::Int},
};
constexpr int kNumKnobs = sizeof(kKnobs) / sizeof(kKnobs[0]);
static_assert(kNumKnobs <= 32, "Knobs::forced has one bit per knob");

int knob_value(Parse parse, const char *text);
void load_knobs();
const Knobs &env_knobs();

// ---- measured route table (ABI v12) ---------------------------------------------------------------------------------
// The rules of the plan_* functions choose a kernel family, tiles per wave, the gather pass's grid and the scatter's item order
// from sizes alone; they were calibrated on three pyramids and a few batch sizes and are the FALLBACK.  A
// caller that has TIMED the alternatives for a call shape (devis_amd.tune, or the audited table shipped as
// devis_amd/routes.json) pins the winner here: key = everything the rules look at (direction, dtype code, clips, frames,
// window, S, M, D, L, Lq, points, the host copy of the shapes), settings = the route knobs.  A knob forced through the
// environment (tests, A/B runs) wins over a pin.  Results never depend on a pin: every route computes the same function.
constexpr int kNotPinned = -2;
struct RoutePin {
    std::string key;
    int value[kNumKnobs];               // per row of kKnobs: the pinned value, or kNotPinned
};

int route_key(char *buf, int len, bool bwd, int dtype, const Params &p);
bool parse_route_settings(const char *text, RoutePin &pin);
Knobs call_knobs(bool bwd, int dtype, const Params &p);
// msda_pin_route / msda_clear_routes / msda_route_count behind their argument checks; pin_route: false = cannot parse the settings
bool pin_route(const char *key, const char *settings);
void clear_routes();
int route_count();

}  // namespace msda
