// msda_params.h -- what the kernels and the host-only units (msda_knobs.hip, msda_plan.hip) both need: the kernel parameter
// blocks, the resident-window plan and its tile geometry, and the launch-geometry constants.  Plain C++17, no HIP include: the
// planner compiles with any host compiler.  The kernel units get it through msda_common.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "msda.h"

// `__host__ __device__` in the units that include msda_common.h (which defines it), nothing in the host-only units.
#ifndef MSDA_HD
#define MSDA_HD
#endif

namespace msda {

constexpr int kWave = 64;   // gfx950 wavefront
constexpr int kPch = 16;    // sampling points per LDS chunk (= L*P of the DeVIS configs)
constexpr unsigned kOobBytes = 0xF0000000u;     // byte offset of a corner outside the map: beyond every buffer resource (msda_common.h, gather_load_z)

// ------------------------------------------------------------------------------------------------
// kernel parameters: one struct serves the plain op (frames = 1, window = 0, LB = 0) and the fused
// temporal op (array A = current-frame points, array B = temporal points)
// ------------------------------------------------------------------------------------------------
struct Params {
    const void *value;          // [groups, S, M, D]; groups = clips * frames
    const int64_t *shapes;      // [L, 2] (H, W)
    const int64_t *lsi;         // [L]
    const int32_t *ftab;        // [frames, window] or null
    const void *locA, *awA;     // [groups, Lq, M, LA, PA, 2], [groups, Lq, M, LA, PA]
    const void *locB, *awB;     // [groups, Lq, M, LB, PB, 2], ...      (LB = window * L)
    void *out;                  // fwd: [groups, Lq, M*D]
    const void *grad_out;       // bwd
    void *grad_value;           // bwd: acc type, pre-zeroed
    void *glocA, *gawA, *glocB, *gawB;
    unsigned *workspace;        // bwd: 8 work-ticket counters of the scatter pass (zeroed by the caller) or null
    int *bbox;                  // bwd: [groups, M, LA+LB, Lq, 2] (min, max) top tap row per (row, virtual level) -- or, with
                                // cull_points, the top tap row of each of its <= 4 points as int16 (same 8 bytes) --
                                // written by the gather pass, read by the scatter pass to cull rows; or null
    int groups, frames, window;
    int S, M, D, L, Lq;
    int LA, PA, LB, PB;
    int64_t v_clip, v_head;     // element strides of `value`: between clips (= frames * S pixels), between heads
    int v_pix;                  // ... and between consecutive pixels (standard [S, M, D]: frames*S*M*D, D, M*D)
    int *bsum;                  // bwd: [groups, M, LA+LB, ceil(Lq/64), 2] (min, max) top tap row over blocks of 64 queries
                                // (built from the per-point records; lets long candidate ranges skip dead blocks) or null
    const int64_t *shapes_host; // HOST copy of `shapes` or null: kernel selection only (never dereferenced on the device)
    int cull_points;            // bbox entries are 4 x int16 top tap rows, one per POINT (PA, PB <= 4), not (min, max)
    int wide_stores;            // bwd: the four gradient arrays are 16-byte aligned (resident-slab gather pass: whole-row stores)
    int wide_loads;             // loc / attn arrays are 16-byte aligned (resident-slab kernels: whole-row loads)
    int dbg;                    // measurement hooks (MSDA_DBG env: the kDbg* bits below), 0 in production
    int gv_storage;             // bwd: grad_value is in the STORAGE type (16-bit), not the arithmetic type (owner-computes scatter only)
    int own_levels;             // bwd: the owner-computes scatter handles levels [0, own_levels); the trailing (coarse) levels are
                                // the matrix-pipe scatter's (msda_mfma.hip).  = L when that kernel does not run
    int own_pix;                // bwd: pixels per band of the owner-computes scatter for THIS call (ScatterPlan::own_pix: 1280 or 1024);
                                // selects the kernel's slot count at the launch, the planner counted the bands with it
    unsigned rec_mask;          // bwd: bit l = the gather pass leaves culling records for level l and the owner-computes scatter reads
                                // them; clear for the matrix-pipe levels and for levels that are ONE band (every group a candidate)
    int walk_down;              // bwd: the resident-slab gather pass takes its workgroups in the reverse of the forward's order
                                // (GatherPlan::walk_down, kWalkDownBytes below): speed only, every workgroup computes what it did
};

// The gather pass of a call too large for the last-level cache walks its work DOWNWARDS.  Forward and gather pass give every
// XCD the same clips in the same ascending order, so between the two uses of a `value` line lies the forward's whole footprint,
// and a 256 MiB memory-side cache (LRU-like) keeps nothing for the second use.  In the reverse order the maps the forward read
// last are the first the gather pass reads.  A call whose footprint (value + sampling points + out) stays below this size fits
// the cache either way and keeps the ascending order.
constexpr long long kWalkDownBytes = 256ll << 20;

struct Level { int H, W, start, pad; };   // start = first pixel of the level inside the CLIP slab

constexpr int kNoRow16 = -32768;            // culling record of a point that touches no row (see the gather passes)
constexpr int kSlabMaxLevels = 32;          // levels the resident-slab kernels keep tables for
constexpr int kScatterMaxLevels = 32;
constexpr int kOwnMaxSorted = 256;            // (level, band) pairs the owner-computes scatter sorts by position (more: level order)
constexpr int kScatterMaxSources = 64;      // 1 + frames * window must fit
constexpr int kCullBlock = 64;              // queries per block summary of the culling records
constexpr int kLiveWords = 64;              // up to 2048 cull batches per item take the block-summary pre-pass
// gradient groups of a backward call (include/msda.h, msda_backward_grads)
constexpr int kGradValue = MSDA_GRAD_VALUE, kGradSampling = MSDA_GRAD_SAMPLING, kGradAll = kGradValue | kGradSampling;
constexpr int kGradDet = MSDA_GRAD_DETERMINISTIC;
constexpr int mfma_rows(int MT) { return MT * 32 - 16; }                 // pixel rows per k-chunk of a tile: pixels + 1 trash row <= this

// ------------------------------------------------------------------------------------------------
// the measurement bits: MSDA_SCATTER_DBG and MSDA_DBG (read only with MSDA_ENABLE_HOOKS=1, msda_knobs.h)
// ------------------------------------------------------------------------------------------------
// THE table of both words: every reader tests these names, devis_amd/tuning.py carries the same names and values for tests and
// scripts (tests/test_plan_cpu.py compares the two), INTEGRATION.md prints it.  A ROUTE bit sends the call another way and keeps
// its results: tests may set it.  An ABLATION bit cuts work out of a kernel to time the rest: the results are WRONG by
// construction.  "owner" = msda_bwd_value_grp_kernel, "LDS" = msda_bwd_value_lds_kernel (msda_scatter.hip); the two kernels
// give some ablation bits different meanings, hence two names for one value.
//
// MSDA_SCATTER_DBG, route bits (results kept)
constexpr int kSdbgStaticStride = 16;       // owner + LDS: items by static stride, never by work tickets.  Results kept
constexpr int kSdbgLevelOrder = 256;        // knob parser: Knobs::scatter_order = 1, the planner keeps the owner kernel's level-by-level item order.  Results kept
constexpr int kSdbgSeparateZero = 1024;     // planner: the zero-fill stays a launch of its own (ScatterPlan::fused_zero = false).  Results kept
constexpr int kSdbgImageOrder = 2048;       // knob parser: Knobs::scatter_order = 2, image order wherever the planner can count the bands.  Results kept
constexpr int kSdbgNoBandRotation = 4096;   // owner: the static stride never rotates the bands by the (clip, frame) index.  Results kept
constexpr int kSdbgNoFourSlotRule = 8192;   // planner: few-item calls keep five pixels per owner quad as well.  Results kept
constexpr int kSdbgOrderMask = kSdbgLevelOrder | kSdbgImageOrder;   // the parser takes these out of Knobs::scatter_dbg (256 wins over 2048)
constexpr int kSdbgRouteMask = kSdbgStaticStride | kSdbgOrderMask | kSdbgSeparateZero | kSdbgNoBandRotation | kSdbgNoFourSlotRule;
// MSDA_SCATTER_DBG, ablation bits (timing only: WRONG results)
constexpr int kSdbgOwnNoWalk = 1;           // owner: lists are built and never walked.  Results WRONG
constexpr int kSdbgOwnNoLink = 2;           // owner: rows are staged, no corner is linked into a list.  Results WRONG
constexpr int kSdbgLdsScanOnly = 2;         // LDS: the survivors are listed and never scanned.  Results WRONG
constexpr int kSdbgOwnNoStage = 4;          // owner: no grad_out row is staged, the walk reads whatever the rows hold.  Results WRONG
constexpr int kSdbgLdsNoSources = 4;        // LDS: an item has no source frames, only its zero band is flushed.  Results WRONG
constexpr int kSdbgOwnCullOnly = 8;         // owner: the culling pass runs, its survivor list is dropped.  Results WRONG
constexpr int kSdbgLdsNoAdds = 8;           // LDS: everything but the LDS adds.  Results WRONG
constexpr int kSdbgOwnLevelShift = 5, kSdbgOwnLevelMask = 7;    // owner: field (word >> 5) & 7 = level + 1: the items of that level only (0: all).  Results WRONG
constexpr int kSdbgOwnLevelField = kSdbgOwnLevelMask << kSdbgOwnLevelShift;
constexpr int kSdbgAblationMask = kSdbgOwnNoWalk | kSdbgOwnNoLink | kSdbgOwnNoStage | kSdbgOwnCullOnly | kSdbgOwnLevelField;
// what of Knobs::scatter_dbg each kernel reads: the launcher (msda_api.hip) passes nothing else
constexpr int kSdbgOwnMask = kSdbgStaticStride | kSdbgNoBandRotation | kSdbgAblationMask;
constexpr int kSdbgLdsMask = kSdbgStaticStride | kSdbgLdsScanOnly | kSdbgLdsNoSources | kSdbgLdsNoAdds;
// Not an environment bit: the owner kernel's second argument is a word of launch FLAGS, kSdbgOwnMask of the environment's bits
// and this one, which the launcher sets from ScatterPlan::fused_zero and from nothing else -- the zero-fill of the pixels outside
// every level runs in the kernel's prologue.  (Value 512: above the kernel's environment bits 0..7, never parsed into them.)
constexpr int kOwnFusedZero = 512;
static_assert((kSdbgRouteMask & kSdbgAblationMask) == 0 && ((kSdbgRouteMask | kSdbgAblationMask) & kOwnFusedZero) == 0,
              "MSDA_SCATTER_DBG: a bit is a route bit, an ablation bit or the launch flag");
//
// MSDA_DBG (Knobs::dbg; the tile kernels see it as Params::dbg), route bits (results kept)
constexpr int kDbgTileRotateHeads = 32;     // tile kernels: heads rotate over the workgroups, breaks the head <-> XCD affinity.  Results kept
constexpr int kDbgNarrowStores = 64;        // launcher: Params::wide_stores = 0 whatever the alignment of the gradient arrays.  Results kept
constexpr int kDbgNarrowLoads = 128;        // launcher: Params::wide_loads = 0 whatever the alignment of loc / attn.  Results kept
constexpr int kDbgRouteMask = kDbgTileRotateHeads | kDbgNarrowStores | kDbgNarrowLoads;
// MSDA_DBG, ablation bits (timing only: WRONG results)
constexpr int kDbgTileNoWriteOut = 8;       // backward tile kernel: grad_loc / grad_attn are computed and not stored.  Results WRONG
constexpr int kDbgTileNoRowSum = 16;        // backward tile kernel: no cross-lane sum of the four corner dots.  Results WRONG
constexpr int kDbgAblationMask = kDbgTileNoWriteOut | kDbgTileNoRowSum;

// ------------------------------------------------------------------------------------------------
// launch geometry shared by kernels and dispatcher
// ------------------------------------------------------------------------------------------------
constexpr int kRowSlots = kPch + 1;         // tile kernels: 16-byte record slots per row (odd: LDS banks)
constexpr int kTileMaxWaves = 8;            // forward tile kernel: waves of one workgroup that share a tile (small calls)
// owner-computes scatter
constexpr int kOwnThreads = 1024;                   // (512: two workgroups per CU out of phase with each other)
constexpr int kOwnQuads = kOwnThreads / 4;
constexpr int kOwnSlots = 4;                        // pixels per owner quad: the least of own_slots (few-item calls, 16-bit types with float grad_value)
constexpr int kOwnPix = kOwnQuads * kOwnSlots;      // pixels per band
// The group-granular owner kernel (msda_bwd_value_grp_kernel) keeps FIVE pixels per owner quad where its instantiation has the
// registers for them at 4 workgroups' worth of waves per SIMD (no VGPR spill, no scratch: profiles/own5_resource_usage.txt):
// fp32, and the 16-bit types when grad_value is written in the storage type.  A 16-bit type with FLOAT grad_value is at 123
// VGPRs with four slots and stays there.  The 360x640 pyramid's 45 x 80 level is then 3 bands of 15 rows instead of 4.
// own_slots is the MOST an instantiation takes: dtype = an msda_dtype code, gv_storage = Params::gv_storage.  Both slot counts are
// compiled where five fit, and the planner picks one per call (msda_plan.hip, plan_scatter: few-item calls stay on four); the
// choice travels as ScatterPlan::own_pix / Params::own_pix, so that the kernel launched and every band count agree.
constexpr int own_slots(int dtype, bool gv_storage) { return (dtype == MSDA_F32 || gv_storage) ? 5 : kOwnSlots; }
constexpr int own_band_pixels(int dtype, bool gv_storage) { return kOwnQuads * own_slots(dtype, gv_storage); }
// Bands of a level of H x W pixels at `pix` pixels per band: nb = ceil(H / floor(pix / W)) bands of equal height to within one
// row -- the first H % nb bands have H / nb + 1 rows, the others H / nb (45 rows in 4 bands: 12, 11, 11, 11) -- instead of runs
// of floor(pix / W) rows and a short last band.  0 = a "direct" level (no rows, or a row wider than kOwnRowPix = 1024 pixels, own_row_fits: one
// item, float atomics).  That limit is the same for every slot count, as it was: the fifth slot buys taller bands, not wider rows
// (a row of 1025-1280 pixels would be a band of ONE row per item), so which levels are "direct", which calls may have a
// storage-typed grad_value and which need a zero-fill launch of their own does not depend on the instantiation.  Host (planner: band counts, the one-band rule of rec_mask) and device (items, row ranges) evaluate the same integers.
constexpr int kOwnRowPix = kOwnPix;                 // the widest row a band takes, whatever its slots (also the zero-fill's cap)
template <typename I> MSDA_HD inline bool own_row_fits(I W) { return W <= (I)kOwnRowPix; }
template <typename I> MSDA_HD inline I own_band_count(I H, I W, I pix)
{
    const I rows = pix / (W > 0 ? W : 1);           // whole rows a band holds
    return (H <= 0 || rows <= 0 || !own_row_fits(W)) ? 0 : (rows >= H ? 1 : (H + rows - 1) / rows);
}
// first and last row of band b of a level cut into nb > 0 bands: q = H / nb, rem = H % nb (no division per band)
template <typename I> MSDA_HD inline void own_band_rows(I q, I rem, I b, I &r0, I &r1)
{
    r0 = b * q + (b < rem ? b : rem);
    r1 = r0 + q - (b < rem ? 0 : 1);
}
// resident-slab kernels
constexpr int kRsThreads = 1024, kRsWaves = kRsThreads / kWave;     // (512: 8 waves with a 256-VGPR budget each -- measured slower)
constexpr int kRsRows = kWave / 4;       // rows per wave tile: one quad per row
constexpr int kRsSlack = 1024;          // bytes: the last LDS-DMA piece may overrun the slab's pixels
constexpr int kRsLdsBytes = 160 * 1024;
constexpr int kRsMaxFrames = 32;        // frames x frames slot masks live in LDS
constexpr int kRsRowB = 128;            // bytes of one pixel of one head in a 4-byte type (D = 32); 64 in a 2-byte type
constexpr int kRsTailBytes = kRsRowB + kRsMaxFrames * kRsMaxFrames * 4 + 4 * kSlabMaxLevels * 4 + 16;   // after the slab
constexpr int kRsSlabBytes = ((kRsLdsBytes - 256 - kRsTailBytes) / 128) * 128;

// ---- resident-window kernels (msda_win.hip): encoder-shaped calls, where query i IS pixel i of the pyramid and samples round
// its own position.  A workgroup owns the queries of one spatial TILE (By x Bx level-0 pixels and the pixels of the other
// levels whose centres fall into it) and stages, per source frame, a WINDOW of every level -- the tile's footprint on that
// level plus `halo` pixels on every side -- in LDS; taps outside the window are read from memory (any input is computed
// exactly; only speed depends on locality).  When all windows do not fit at a useful halo the levels are staged in two
// phases per source frame: levels < split, then levels >= split (split = 0: one phase).
constexpr int kWinMaxLevels = 8;
struct WinPlan {
    int By, Bx, tiles_y, tiles_x;       // tile size in level-0 pixels; tiles of one map
    int split;                          // first level of the second staging phase (0 = one phase)
    int halo[2];                        // pixels round the footprint, per phase
    int wbase[kWinMaxLevels];           // first LDS pixel of level l's window (inside its phase's layout)
    int tpg;                            // wave tiles (16 rows) per query frame: ceil(most queries of a tile / 16)
    int nt;                             // wave tiles per wave: ceil(frames * tpg / 16 waves) <= 3
};

// One axis of a tile's geometry on a level with n_l pixels (n_0 on level 0): the level's own pixels the tile OWNS
// [q0, q1) -- pixel y belongs to the tile its centre falls into, i.e. floor((2y + 1) n_0 / (2 n_l) / B) -- and the window
// [w0, w1) that holds every tap of a point within `halo` pixels of the tile's extent (floor(y n_l - 0.5) and the row below).
// Host (planning: maxima over the tiles) and device (the tile's own tables) evaluate the same integers.
MSDA_HD inline int win_fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
MSDA_HD inline void win_axis(int n_l, int n_0, int t, int B, int halo, int &q0, int &q1, int &w0, int &w1)
{
    const int a = 2 * n_l * t * B - n_0, b = 2 * n_l * (t + 1) * B - n_0, d = 2 * n_0;
    auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
    q0 = clampi(-win_fdiv(-a, d), 0, n_l);          // ceil
    q1 = clampi(-win_fdiv(-b, d), 0, n_l);
    w0 = clampi(win_fdiv(a, d) - halo, 0, n_l);
    w1 = clampi(win_fdiv(b, d) + 2 + halo, 0, n_l);
}

constexpr int kWinTailBytes = 128 + kRsMaxFrames * kRsMaxFrames * 4 + 14 * kWinMaxLevels * 4 + 64;    // zero row, slot masks, level tables
constexpr int kWinSlabBytes = ((160 * 1024 - 256 - kWinTailBytes) / 128) * 128;

struct PrepParams {
    const void *off_c, *off_t;        // [rows, M, L, Pc, 2], [rows, M, W*L, Pt, 2]   raw sampling offsets
    const void *logit_c, *logit_t;    // [rows, M, L*Pc], [rows, M, W*L*Pt]           raw attention logits
    const void *ref_c, *ref_t;        // [rows, L, d], [rows, W*L, d]                 reference points (d = 2 | 4)
    const int64_t *shapes;            // [L, 2] (H, W)
    void *loc_c, *loc_t, *aw_c, *aw_t;            // forward outputs (backward: aw_* are inputs)
    const void *gloc_c, *gloc_t, *gaw_c, *gaw_t;  // backward inputs
    void *goff_c, *goff_t, *glogit_c, *glogit_t;  // backward outputs
    int64_t rows;
    int64_t ld;                       // row stride of the Linear-side tensors (offsets / logits forward, their grads
                                      // backward) when they are column slices of one fused matrix; 0 = each dense
    int M, L, W, Pc, Pt, d;
};

constexpr int kMaxDevices = 64;

}  // namespace msda
