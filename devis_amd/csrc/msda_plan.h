// msda_plan.h -- host only, no HIP and no call into the HIP runtime: which kernel family takes a call and with what grid
// (msda_plan.hip).  Pure functions of the sizes, the knobs and the CU count: msda_api.hip launches what they return, and they
// run as they are on a CPU.
#pragma once

#include "msda_knobs.h"

namespace msda {
namespace plan {

inline bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

size_t tile_lds_bytes(int rpw, int nvl, bool bwd, bool intervals = false);
int elem_bytes(int dtype);
int storage_dtype(int dtype);
bool scatter_applicable(const Params &p, const Knobs &k);
bool owner_scatter_applicable(const Params &p, int esz, const Knobs &k);
bool rs_fits(const Params &p, int esz);
bool win_plan_cached(const Params &p, int esz, int min_halo, WinPlan &w);
bool storage_typed_grad_value_ok(int dtype, const Params &p, const Knobs &k);
unsigned persistent_grid(int cus);
bool fast_path_takes(int dtype, const Params &p, const Knobs &k, bool bwd);

// What the fast path's rules read of a call, worked out once.
struct Shape {
    int esz;                            // bytes of a value element
    int G, RPW;                         // tile kernels: G = D / (16 / esz) lanes per row, 64 / G rows per wave,
    unsigned blocks;                    // one workgroup per (wave of rows, head)
    size_t tile_lds;                    // ... and its LDS (backward: with the interval records when p.bbox is set)
    int64_t clips;
    int cus;                            // compute units of the device (an input: the planner does not ask the runtime)
    bool rs_ok;                         // rs_fits
    int rs_tiles_per_clip, l0_host;     // resident-slab kernels: 16-row tiles per clip, first slab level
    long long outside, l2_budget;       // bytes of one (clip, head)'s levels below l0_host; see rs_tiles_per_wave
    long long footprint;                // bytes of value + sampling points (locations and weights) + out of the call: walk_down_rule
};

bool shape_of(int dtype, const Params &p, bool bwd, int cus, Shape &s);         // false: the problem is too large for one launch

struct FwdPlan {
    enum { kWindow, kSlab, kTile } family = kTile;
    WinPlan win;                        // kWindow
    int nt = 0, body_l0 = 0, parts = 0; // kSlab: tiles per wave, level the slot body is compiled for, workgroups per (clip, head)
    int waves = 1;                      // kTile: waves per tile
    size_t lds = 0;                     // kTile
};
FwdPlan plan_forward(const Shape &s, const Params &p, const Knobs &k);

struct ScatterPlan {
    enum { kAtomic, kOwner, kLds } route = kAtomic;   // one-kernel backward with global atomics / owner-computes / LDS-atomic scatter
    int l0 = 0;                         // kOwner: the owner-computes kernel walks levels [0, l0), the matrix-pipe kernel [l0, L)
    int mfma_tiles = 0;                 // kOwner: tiles of the matrix-pipe kernel, 0 = it does not run
    bool run_owner = false, run_mfma = false;   // kOwner: which of the two kernels run (MSDA_SCATTER_PART)
    int own_pix = kOwnPix;              // kOwner: pixels per band of the owner kernel for this call (Params::own_pix)
    bool fused_zero = false;            // kOwner: the zero-fill rides in the owner kernel's prologue: the launcher sets the kernel's
                                        // launch flag kOwnFusedZero (msda_params.h) from this and from nothing else
    bool image_order = false;           // kOwner: the owner kernel's items in image order
    unsigned rec_mask = ~0u;            // levels the gather pass leaves culling records for (Params::rec_mask)
    bool interval_records = false;      // the gather pass leaves (min, max) interval records: only the tile kernel writes those
};
ScatterPlan plan_scatter(int dtype, const Shape &s, const Params &p, const Knobs &k, int grads);

struct GatherPlan {
    enum { kRecordsOnly, kWindow, kSlab, kTile } kind = kTile;
    WinPlan win;                        // kWindow
    int parts = 0, frame_split = 0;     // kSlab: workgroups per (clip, head) -- or per (clip, head, frame) with frame_split
    unsigned grid = 0;                  // kSlab
    bool walk_down = false;             // kSlab: every XCD takes its run of workgroups last first, the reverse of the forward's walk (walk_down_rule)
};
GatherPlan plan_gather(const Shape &s, const Params &p, const Knobs &k, int grads, bool interval_records);

// ---- size rules ---------------------------------------------------------------------------------------------------
long long workspace_table_bytes(int batch, int num_query, int num_heads, int virtual_levels);
long long workspace_need(int batch, int num_query, int num_heads, int virtual_levels);
int mfma_scatter_tiles(long long pixels);
long long det_maxima_bytes(long long clips, int num_heads);
long long det_workspace_bytes(long long clips, int frames, int spatial_size, int num_heads, int channels);

}  // namespace plan
}  // namespace msda
