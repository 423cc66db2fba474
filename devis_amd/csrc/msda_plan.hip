// msda_plan.hip -- kernel selection of libmsda_hip.so (which family takes a shape: resident-slab / resident-window / tile /
// generic kernels; owner-computes / LDS / atomic scatter) and the size rules of its workspaces.  Host only, no HIP: see msda_plan.h.
#include "msda_plan.h"
#include <algorithm>
#include <string.h>

namespace msda {
namespace plan {

size_t tile_lds_bytes(int rpw, int nvl, bool bwd, bool intervals)
{
    return (size_t)rpw * kRowSlots * 16 * (bwd ? 3 : 2) + (size_t)nvl * sizeof(Level) +
           (intervals ? (size_t)rpw * nvl * 8 : 0);     // + the per-(row, level) tap-row intervals
}

int elem_bytes(int dtype) { return dtype == MSDA_F32 ? 4 : dtype == MSDA_F64 ? 8 : 2; }        // of value / out / grad_out
// the storage type of value / out / grad_out behind a dtype code (MSDA_*_LOC32: the 16-bit type)
int storage_dtype(int dtype) { return dtype == MSDA_BF16_LOC32 ? MSDA_BF16 : dtype == MSDA_F16_LOC32 ? MSDA_F16 : dtype; }

// How many of the LAST pyramid levels fit `cap_pixels` pixels of LDS slab (the device-side rule of first_slab_level,
// evaluated on the host copy of spatial_shapes when the caller passed one; otherwise guessed from the pixel count:
// with the usual stride-2 pyramids level 0 holds ~3/4 of the S pixels).  Returns the first slab level l0.
static int host_first_slab_level(const Params &p, long long cap_pixels)
{
    if (p.shapes_host) {
        int l0 = p.L;
        long long acc = 0;
        for (int l = p.L - 1; l >= 0; --l) {
            acc += (long long)p.shapes_host[2 * l] * p.shapes_host[2 * l + 1];
            if (acc > cap_pixels) break;
            l0 = l;
        }
        return l0;
    }
    if (p.L == 1) return (long long)p.S <= cap_pixels ? 0 : 1;
    return (long long)p.S <= cap_pixels ? 0 : ((double)p.S * 0.2551 <= (double)cap_pixels ? 1 : 2);
}

// Pixels of the levels below l0 (the ones the resident-slab kernels gather through the L2), from the host copy of the
// shapes or, without one, from the usual stride-2 pyramid proportions.
static long long host_pixels_below(const Params &p, int l0)
{
    if (l0 <= 0) return 0;
    if (p.shapes_host) {
        long long acc = 0;
        for (int l = 0; l < l0 && l < p.L; ++l) acc += (long long)p.shapes_host[2 * l] * p.shapes_host[2 * l + 1];
        return acc;
    }
    return l0 >= p.L ? p.S : (long long)((double)p.S * (l0 == 1 ? 0.75 : 0.94));
}

// Tiles per wave of the resident-slab kernels = how many workgroups share one (clip, head).  Every workgroup of a
// pair gathers the non-resident levels from the same maps, and both kernels are bound by how fast a CU's vector-memory
// path returns those scattered lines, i.e. by what an XCD's 4 MiB L2 keeps of the maps: take the
// LARGEST workgroups (least slab staging) whose pairs in flight per XCD keep the non-resident levels within
// `l2_budget`, else the smallest.  Measured on the round-3 kernels, 16 clips of the DeVIS decoder shape (same box),
// 1 / 2 / 4 tiles per wave: fp32 (460 KiB per level-0 map) forward 0.337 / 0.364 / -- ms, gather pass 0.423 / 0.471 /
// 0.560; bf16 (230 KiB, two heads per 128-byte line) forward -- / 0.246 / 0.238, gather pass 0.363 / 0.326 / 0.312.
// Hence a budget of 2 MiB for 4-byte types and 4 MiB for 2-byte types.
static int rs_tiles_per_wave(const Params &p, int tiles_per_clip, long long outside_bytes, bool force, long long l2_budget, int max_tiles, int cus)
{
    // Among the candidates that (nearly) fill the chip and keep the non-resident levels of the (clip, head) pairs in flight per XCD
    // within `l2_budget` -- or the smallest one if none does -- the one with the least (rounds of workgroups over the CUs) x (tiles
    // per wave), larger workgroups on a tie: 360 workgroups of 4 tiles are two rounds of 4, 720 of 2 are three rounds of 2 (round
    // 4 audit, 1-clip encoder call on the SwinL pyramid in bf16: forward 0.455 -> 0.373 ms, gather pass 0.634 -> 0.534).
    const int64_t clips = p.groups / p.frames;
    const int cus_per_xcd = cus / 8 > 0 ? cus / 8 : 1;
    int pick = 0, fallback = 0;
    long long best = 0;
    for (int cand : {4, 2, 1}) {
        if (cand > max_tiles) continue;
        const int parts = (tiles_per_clip + kRsWaves * cand - 1) / (kRsWaves * cand);
        const long long wgs = clips * p.M * parts;
        // must fill the chip -- nearly, for workgroups of several tiles per wave: 232 workgroups of 4 tiles (1-clip encoder call,
        // bf16 forward 0.263 -> 0.227 ms) do; 240 of 1 tile (1-image SwinL encoder call) are 7 % behind the tile kernels
        if (!force && (cand > 1 ? 4 * wgs < 3LL * cus : wgs < cus)) continue;
        fallback = cand;                                              // (ends as the smallest admissible candidate)
        const long long pairs = (cus_per_xcd + parts - 1) / parts;
        // (encoder-shaped calls -- one query per pixel, sampling round its own position -- find their non-resident lines in the L2
        // whatever the pairs in flight: single-frame fp32 encoder call on the SwinL pyramid, 6 images, 0.134 -> 0.089 ms)
        if (p.Lq != p.S && pairs * outside_bytes > l2_budget) continue;
        // (x2, + 1: half a tile's worth of fixed cost per workgroup -- slab staging, set-up; 8-image encoder call 0.072 -> 0.064 ms)
        const long long cost = ((wgs + cus - 1) / cus) * (2 * cand + 1);
        if (!pick || cost < best) { pick = cand; best = cost; }
    }
    return pick ? pick : fallback;
}

static bool standard_value_layout(const Params &p)
{
    return p.v_clip == (int64_t)p.frames * p.S * p.M * p.D && p.v_head == p.D && p.v_pix == p.M * p.D;
}

// Can grad_value go through a scatter kernel (owner-computes or LDS atomics)?  MSDA_BWD_MODE=atomic forces the
// one-kernel backward with global atomics (kept for A/B measurements and as the any-shape path).
bool scatter_applicable(const Params &p, const Knobs &k)
{
    if (k.bwd_atomic) return false;
    if (p.L > kScatterMaxLevels || (p.D % 4) != 0 || p.D / 4 > kWave || ((p.D / 4) & (p.D / 4 - 1)) != 0) return false;   // D / 4 lanes per hit
    if (1 + p.frames * p.window > kScatterMaxSources || p.Lq >= (1 << 24)) return false;   // survivor-list entry fields
    if (p.window == 0 && p.LA != p.L) return false;
    if ((int64_t)p.groups * p.Lq >= 0x7fffffffLL) return false;       // query rows are 32-bit in the hit records
    return true;
}

// The owner-computes scatter (msda_bwd_value_grp_kernel) takes D = 32 with <= 4 points per level and the per-point
// culling records (or no records at all).
bool owner_scatter_applicable(const Params &p, int esz, const Knobs &k)
{
    // (work items -- (clip, frame, head, band) with at most one band per pixel row -- are counted in 32 bits)
    return p.D == 32 && (esz == 4 || esz == 2) && p.PA <= 4 && p.PB <= 4 && p.Lq < (1 << 22) && k.scatter_own != 0 &&
           k.scatter_lds_kb == 144 && (int64_t)p.groups * p.M * ((int64_t)p.S + p.L) < 0x7fffffffLL && scatter_applicable(p, k);
}

// The resident-slab kernels take D = 32 in 2- / 4-byte types when the index arithmetic fits and at least the last
// pyramid level fits the slab.  One predicate for forward and gather pass: a forward / backward pair never splits
// between kernel families on a shape limit.
bool rs_fits(const Params &p, int esz)
{
    const int64_t pixB = (int64_t)p.v_pix * esz;
    const int64_t pmax = p.PA > p.PB ? p.PA : p.PB;
    return p.D == 32 && (esz == 4 || esz == 2) && p.LA == p.L && p.L <= kSlabMaxLevels &&
           (int64_t)p.frames * p.S < (1 << 24) && pixB < (1 << 24) && (int64_t)p.frames * p.S * pixB < 0x7fffffffLL &&
           p.frames <= kRsMaxFrames && p.window <= 31 &&
           pmax * pmax * p.L < 65536;         // the kernels take a point's level as (k * ceil(2^16 / P)) >> 16
}

// Plan of the resident-window kernels (msda_win.hip; WinPlan in msda_params.h) for an encoder-shaped call: the largest tile
// whose rows fit a workgroup (frames * ceil(queries / 16) wave tiles <= 3 per wave), then the widest halo whose windows fit
// the LDS -- all levels at once when that halo reaches 6 pixels, else level 0 and the other levels in two staging phases.
// `min_halo`: MSDA_WIN_MIN_HALO.  (Its preconditions and the grid count of the call: win_plan_cached, its only caller.)
static bool win_plan(const Params &p, int esz, int min_halo, WinPlan &w)
{
    long long pixels = 0;
    for (int l = 0; l < p.L; ++l) {
        if (p.shapes_host[2 * l] <= 0 || p.shapes_host[2 * l + 1] <= 0 || p.shapes_host[2 * l] > 16000 || p.shapes_host[2 * l + 1] > 16000) return false;       // (win_axis: 2 * n_l * n_0 in 32 bits)
        pixels += p.shapes_host[2 * l] * p.shapes_host[2 * l + 1];
    }
    if (pixels != p.Lq) return false;                 // the tiles enumerate the queries as the pixels of the pyramid
    const int cap_px = kWinSlabBytes / (32 * esz), H0 = (int)p.shapes_host[0], W0 = (int)p.shapes_host[1];
    auto H = [&](int l) { return (int)p.shapes_host[2 * l]; };
    auto W = [&](int l) { return (int)p.shapes_host[2 * l + 1]; };
    // most pixels of level l a tile owns / needs in its window, per axis (maxima over the tiles)
    auto extent = [&](int n_l, int n_0, int B, int halo, bool window) {
        int best = 0;
        for (int t = 0; t < (n_0 + B - 1) / B; ++t) {
            int q0, q1, w0, w1;
            win_axis(n_l, n_0, t, B, halo, q0, q1, w0, w1);
            best = std::max(best, window ? w1 - w0 : q1 - q0);
        }
        return best;
    };
    // Tile sizes are tried from large to small; a size is taken when its rows fill the workgroup's wave tiles (16 waves x nt x
    // 16 rows) best -- rows of tiles at the map's edge and the idle tail of the last wave tiles cost as much as full ones.
    double best_score = 0.0;
    bool found = false;
    static const int kEdges[] = {24, 20, 16, 12, 10, 8, 6, 4};
    for (int By : kEdges) for (int Bx : kEdges) {
        if (By > 2 * Bx || Bx > 2 * By) continue;
        const int tiles_y = (H0 + By - 1) / By, tiles_x = (W0 + Bx - 1) / Bx;
        int nq = 0;
        for (int l = 0; l < p.L; ++l) nq += extent(H(l), H0, By, 0, false) * extent(W(l), W0, Bx, 0, false);
        const int tpg = (nq + kRsRows - 1) / kRsRows, nt = (p.frames * tpg + kRsWaves - 1) / kRsWaves;
        if (nq <= 0 || nt > 3) continue;                // (the forward keeps nt accumulator sets in registers)
        auto need = [&](int la, int lb, int halo) {       // LDS pixels of the windows of levels [la, lb) (each rounded to a DMA piece)
            int acc = 0;
            for (int l = la; l < lb; ++l)
                acc += (extent(H(l), H0, By, halo, true) * extent(W(l), W0, Bx, halo, true) + 15) / 16 * 16;
            return acc;
        };
        auto widest = [&](int la, int lb) {
            int h = -1;
            while (h < 16 && need(la, lb, h + 1) <= cap_px) ++h;
            return h;
        };
        int split = 0, h0 = widest(0, p.L), h1 = h0;
        if (h0 < min_halo && p.L > 1) {
            int best = h0;
            for (int sp = 1; sp < p.L; ++sp) {
                const int a = widest(0, sp), b = widest(sp, p.L);
                if (std::min(a, b) > best) { best = std::min(a, b); split = sp; h0 = a; h1 = b; }
            }
        }
        if (std::min(h0, h1) < min_halo) continue;      // (a corner outside its window costs a memory round trip of the whole wave)
        // useful rows per row slot of a workgroup, less the share of a source frame's time spent staging (estimated as the
        // window pixels per row served, one pixel ~ the LDS time of a sixth of a row's slot)
        const double rows = (double)p.Lq / ((double)tiles_y * tiles_x) * p.frames;
        const double staged = (split ? need(0, split, h0) + need(split, p.L, h1) : need(0, p.L, h0));
        const double score = rows / (nt * kRsWaves * kRsRows) / (1.0 + staged / (6.0 * rows)) / (split ? 1.08 : 1.0);
        if (score <= best_score) continue;
        best_score = score; found = true;
        w.By = By; w.Bx = Bx; w.tiles_y = tiles_y; w.tiles_x = tiles_x; w.split = split; w.halo[0] = h0; w.halo[1] = h1;
        w.tpg = tpg; w.nt = nt;
        int acc = 0;
        for (int l = 0; l < kWinMaxLevels; ++l) {
            if (l == split && split > 0) acc = 0;
            w.wbase[l] = acc;
            if (l < p.L) {
                const int halo = (split > 0 && l >= split) ? h1 : h0;
                acc += (extent(H(l), H0, By, halo, true) * extent(W(l), W0, Bx, halo, true) + 15) / 16 * 16;
            }
        }
    }
    return found;
}

// win_plan searches tile sizes and halos (~10^5 integer operations): the last plan is kept, keyed by everything it depends on.
bool win_plan_cached(const Params &p, int esz, int min_halo, WinPlan &w)
{
    struct Key { int L, frames, esz, Lq, min_halo; int64_t shapes[2 * kWinMaxLevels]; };
    static thread_local Key last_key;
    static thread_local WinPlan last_plan;
    static thread_local int last_state = -1;           // -1 nothing cached, 0 no plan, 1 plan
    if (!p.shapes_host || p.L < 1 || p.L > kWinMaxLevels || !rs_fits(p, esz)) return false;
    Key k;
    memset(&k, 0, sizeof k);
    k.L = p.L; k.frames = p.frames; k.esz = esz; k.Lq = p.Lq; k.min_halo = min_halo;
    for (int i = 0; i < 2 * p.L; ++i) k.shapes[i] = p.shapes_host[i];
    if (last_state < 0 || memcmp(&k, &last_key, sizeof k) != 0) {
        // (the remaining inputs of win_plan -- D, M, strides, window -- only gate it through rs_fits, checked above)
        last_state = win_plan(p, esz, min_halo, last_plan) ? 1 : 0;
        last_key = k;
    }
    if (last_state != 1) return false;
    w = last_plan;
    return (long long)(p.groups / p.frames) * p.M * w.tiles_y * w.tiles_x <= 0x7fffffffLL;
}

// grad_value may be written in the 16-bit STORAGE type (include/msda.h, msda_grad_value_dtype) when the owner-computes
// scatter will produce it: that kernel overwrites every pixel exactly once from fp32 registers.  Every other route
// accumulates into grad_value (LDS-atomic flush aside, float atomics) and needs the arithmetic type.  Levels wider than a
// band take that kernel's float-atomic branch, so the host copy of the shapes must be there and say they do not occur.
// Its callers pass the unpinned knobs: no pinnable knob changes the answer.
bool storage_typed_grad_value_ok(int dtype, const Params &p, const Knobs &k)
{
    if (storage_dtype(dtype) != MSDA_BF16 && storage_dtype(dtype) != MSDA_F16) return false;
    if (k.force_generic || k.bwd_cull == 2) return false;
    if (!owner_scatter_applicable(p, 2, k) || !p.shapes_host) return false;
    for (int l = 0; l < p.L; ++l)
        if (!own_row_fits(p.shapes_host[2 * l + 1]) || p.shapes_host[2 * l + 1] <= 0) return false;
    // the shape conditions of fast_path_takes (pointer alignment is checked at the call: a mismatch is an error there)
    if (p.D % 8 || (int64_t)p.frames * p.S * p.M * p.D >= 0x7fffffffLL) return false;
    if (tile_lds_bytes(kWave / (p.D / 8), p.LA + p.LB, true) > 60 * 1024) return false;
    return true;
}

// Grid of the persistent scatter kernels: one 1024-thread workgroup per CU, a multiple of the XCD count (item % M stays put).
unsigned persistent_grid(int cus)
{
    return (unsigned)cus - (unsigned)cus % 8;
}

bool shape_of(int dtype, const Params &p, bool bwd, int cus, Shape &s)
{
    s.esz = elem_bytes(dtype);
    s.G = p.D / (16 / s.esz);
    s.RPW = kWave / s.G;
    const int64_t blocks = (int64_t)p.groups * (((int64_t)p.Lq + s.RPW - 1) / s.RPW) * p.M;
    if (blocks > 0x7fffffffLL) return false;
    s.blocks = (unsigned)blocks;
    s.tile_lds = tile_lds_bytes(s.RPW, p.LA + p.LB, bwd, bwd && p.bbox != nullptr);
    s.clips = p.groups / p.frames;
    s.cus = cus;
    s.rs_ok = rs_fits(p, s.esz);
    s.rs_tiles_per_clip = p.frames * (int)(((int64_t)p.Lq + kRsRows - 1) / kRsRows);    // (<= blocks)
    const int rs_row = 32 * s.esz;                                // bytes of one pixel of one head
    s.l0_host = s.rs_ok ? host_first_slab_level(p, (kRsSlabBytes - kRsSlack) / rs_row) : p.L;
    s.outside = host_pixels_below(p, s.l0_host) * rs_row;
    s.l2_budget = s.esz == 4 ? (2ll << 20) : (4ll << 20);         // see rs_tiles_per_wave
    const long long lesz = (dtype == MSDA_BF16_LOC32 || dtype == MSDA_F16_LOC32) ? 4 : s.esz;      // bytes of a location / weight element
    const long long points = (long long)p.LA * p.PA + (long long)p.LB * p.PB;
    s.footprint = (long long)p.groups * p.M * ((long long)p.S * p.D * s.esz + (long long)p.Lq * (3 * points * lesz + (long long)p.D * s.esz));
    return true;
}

// Does the resident-slab gather pass take its work last first (msda_params.h, kWalkDownBytes)?  From sizes alone: a call whose
// footprint fits the last-level cache keeps the ascending order -- its lines survive from the forward to the gather pass whatever
// the order.  Measured on one box, 16 clips of the 360x640 decoder call, up / down (profiles/walk_order_ab.log): fp32 gather pass
// 0.3985 -> 0.3878 ms, step 1.188 -> 1.174; 64 clips 4.63 -> 4.59; bf16 and fp16 level (0.970 / 0.971, 0.944 / 0.941).
// Encoder-shaped calls (one query per pixel) stay as they are: their points are nine times their maps, so that one clip is past
// the limit, and nothing was measured there.  MSDA_WALK (Knobs::walk): 0 = up, 1 = down, whatever the size.
static bool walk_down_rule(const Shape &s, const Params &p, const Knobs &k)
{
    if (k.walk >= 0) return k.walk != 0;
    return s.footprint > kWalkDownBytes && p.Lq != p.S;
}

// Encoder-shaped calls (one query per pixel) take the resident-window kernels when the slab of the resident-slab kernels
// would hold the last level at most (fp32 at 800x1333: 273 of 22223 pixels) -- measured forward 2.38 -> 1.07 ms, gather pass 2.85 -> 1.60 ms there; where
// more levels fit the slab (16-bit types, the 360x640 pyramid) the two families are on a par and the slab kernels stay.
// `mode`: MSDA_FWD_WIN / MSDA_BWD_WIN.
static bool window_route(const Shape &s, const Params &p, const Knobs &k, int mode, WinPlan &w)
{
    // (round 4 audit: also when a 4-byte slab holds only the last TWO levels -- SwinL 480x768 in fp32: forward 0.49 -> 0.37 ms,
    // gather pass 0.66 -> 0.55; 2-byte slabs of that kind -- 800x1333 bf16 -- are on a par and stay)
    // (temporal calls only: single-frame encoder calls on that pyramid are 6-26 % faster on the slab kernels)
    const bool few_levels = s.l0_host >= p.L - 1 || (s.esz == 4 && p.frames > 1 && p.L > 2 && s.l0_host >= p.L - 2);
    if (mode == 0 || (mode != 1 && !(p.Lq == p.S && p.L > 1 && few_levels))) return false;     // (cheap tests first)
    return win_plan_cached(p, s.esz, k.win_min_halo, w);
}

// ---- forward ------------------------------------------------------------------------------------------------
FwdPlan plan_forward(const Shape &s, const Params &p, const Knobs &k)
{
    FwdPlan f;
    if (window_route(s, p, k, k.fwd_win, f.win)) { f.family = FwdPlan::kWindow; return f; }
    if (s.rs_ok) {
        // resident-slab forward: up to NT * 16 tiles of 16 rows per workgroup, so that the per-frame slab staging is
        // amortised; tiles per wave (NT) and workgroups per (clip, head) (parts): see rs_tiles_per_wave
        const int mode = k.fwd_rs;                                     // -1 auto, 0 off, 1 force
        // at most 2 tiles per wave for slabs that start at level 2 (large pyramids) and for fp32: the 4-tile instantiations of
        // those slot bodies spill 10-40 VGPRs (profiles/r04_resource_usage.txt); BASELINE configs[1] forward 0.306 -> 0.290 ms,
        // SwinL 0.088 -> 0.082, 2-clip fp32 encoder call 0.52 -> 0.46
        const int max_nt = (s.l0_host >= 2 || s.esz == 4) ? 2 : 4;
        int nt = rs_tiles_per_wave(p, s.rs_tiles_per_clip, s.outside, mode == 1, s.l2_budget, max_nt, s.cus);
        // the slab must hold at least the last level.  (Since the whole-row loads / stores of the points and gradients
        // the kernel wins for every dtype as soon as ANY level fits -- 800x1333, levels 2-3 resident.)
        if (mode != 1 && s.l0_host > p.L - 1) nt = 0;
        if (k.fwd_rs_nt == 1 || k.fwd_rs_nt == 2 || k.fwd_rs_nt == 4) nt = k.fwd_rs_nt;
        const int parts = nt ? (s.rs_tiles_per_clip + kRsWaves * nt - 1) / (kRsWaves * nt) : 0;
        // few tiles per (clip, head) leave waves of the workgroups without one: 19 tiles (300 queries of a single-frame call)
        // on 2 x 16 waves -- 36-image decoder-like call in fp32 on the SwinL pyramid 0.078 ms here, 0.055 on the tile kernels
        // (only where the slab starts at level 2 in a 4-byte type, i.e. saves the least: elsewhere, and in the gather pass, the slab
        // kernels stay ahead by 4-19 %)
        if (mode != 1 && nt && s.esz == 4 && s.l0_host >= 2 && 10LL * s.rs_tiles_per_clip < 7LL * parts * kRsWaves * nt) nt = 0;
        if (mode != 0 && nt && s.clips * p.M * parts <= 0x7fffffffLL) {
            f.family = FwdPlan::kSlab;
            f.nt = nt;
            f.parts = parts;
            // fp32, one tile per wave, slab from level 2 on: the software-pipelined slot body of that instantiation spills 31 VGPRs
            // and its plain loop (the kernel compiled for a level-1 slab falls back to it) is 16-27 % faster on the SwinL pyramid
            // (decoder call, 4 / 16 / 32 clips: 0.175 -> 0.137, 0.644 -> 0.540, 1.178 -> 0.973 ms; 800x1333: the same)
            f.body_l0 = (s.esz == 4 && nt == 1 && s.l0_host >= 2) ? 1 : s.l0_host;
            return f;
        }
    }
    // SMALL forwards -- one clip at the 60 / 180 queries per frame of DeVIS's shipped configs is 192-1104 single-wave workgroups on
    // 1024 SIMDs, each walking its rows' 96 points as a chain of dependent gather batches -- put THREE waves on a tile, each with
    // a share of the tile's 16-point chunks, partial rows added through LDS in wave order (msda_fwd_tile_kernel, MW): 60 queries
    // fp32 0.020 -> 0.013 ms, fp16 0.034 -> 0.015; 180 queries fp16 0.041 -> 0.027; 300 queries bf16 0.043 -> 0.031.  With more
    // workgroups than SIMDs (fp32 from 180 queries on) the chip is busy anyway and the split only adds the exchange
    // (profiles/r04_logs/small_batch_tile_waves.log: no gain at 1824 workgroups).
    const int G = s.G, RPW = s.RPW, VEC = 16 / s.esz;
    const int chunks = (p.LA * p.PA + kPch - 1) / kPch + (p.LB * p.PB + kPch - 1) / kPch;
    int waves = k.fwd_tile_waves;
    // (fewer single-wave workgroups than SIMDs -- 4 per CU; 4-byte types: than three quarters of them)
    if (waves < 0) waves = s.blocks <= (long long)s.cus * (s.esz == 4 ? 3 : 4) ? 3 : 1;
    waves = std::max(1, std::min(std::min(waves, chunks), kTileMaxWaves));
    if (!(G == 4 || G == 8)) waves = 1;
    auto lds_of = [&](int w) { return (size_t)w * RPW * kRowSlots * 32 + (size_t)(p.LA + p.LB) * sizeof(Level) + (size_t)w * kWave * VEC * 4; };
    while (waves > 1 && lds_of(waves) > 48 * 1024) --waves;
    f.waves = waves;
    f.lds = waves > 1 ? lds_of(waves) : s.tile_lds;
    return f;
}

// ---- backward: scatter plan -----------------------------------------------------------------------------------
// The coarse levels -- the last one or two of the pyramid, together at most ~300 pixels -- on the matrix pipe (msda_mfma.hip):
// the owner-computes kernel then runs on levels [0, l0).  Needs the host copy of the shapes (a true copy: include/msda.h)
// and at least 16 queries (a step is 16 groups).  Automatic for decoder-shaped batches: an item walks (1 + sources) x Lq
// groups in 8 waves, so a handful of items of encoder length would be the kernel's whole duration.
static void plan_matrix_pipe(int dtype, const Shape &s, const Params &p, const Knobs &k, ScatterPlan &sc)
{
    // (its loads are buffer loads with 32-bit byte offsets inside one clip: grad_out and the point arrays of a clip below 2 GiB)
    const long long lesz = (dtype == MSDA_BF16_LOC32 || dtype == MSDA_F16_LOC32) ? 4 : s.esz;
    const long long clip_rows = (long long)p.frames * p.Lq;
    const bool mfma_fits = clip_rows * p.M * p.D * s.esz < 0x7fffffffLL &&
                           clip_rows * p.M * std::max((long long)p.LA * p.PA, (long long)p.LB * p.PB) * 2 * lesz < 0x7fffffffLL;
    if (k.scatter_mfma == 0 || !mfma_fits || !p.shapes_host || p.Lq < 16 || p.L < 2) return;
    long long px = 0;
    for (int l = p.L - 1; l >= 1 && l >= p.L - 2; --l) {
        const long long hw = p.shapes_host[2 * l] * p.shapes_host[2 * l + 1];
        if (p.shapes_host[2 * l] <= 0 || p.shapes_host[2 * l + 1] <= 0 || !mfma_scatter_tiles(px + hw)) break;
        px += hw; sc.l0 = l; sc.mfma_tiles = mfma_scatter_tiles(px);
    }
    const long long items = (long long)p.groups * p.M, per_item = (long long)p.Lq * (1 + p.window);
    // Automatic rule (profiles/r06_logs/mfma_check.log; scatter pass, owner kernel alone -> with this kernel, ms): the two coarse
    // levels of the 360x640 pyramid cost the owner kernel 0.19 ms at 16 clips of 300 queries and this one 0.12 (0.563 -> 0.502;
    // bf16 0.564 -> 0.473; 4 / 8 / 32 clips 0.159 -> 0.148 / 0.289 -> 0.265 / 1.096 -> 1.064); the single 273-pixel level of the
    // 800x1333 pyramid 0.553 -> 0.512 (with the owner kernel's bands rotated unconditionally; see below).
    // It needs items to fill the chip -- 2 clips (96 items) 0.089 -> 0.110, one clip 0.053 -> 0.088 -- and items long enough to
    // pay for their zero-fill and reduction: the plain op on 48 images x 300 queries (19 steps per item) 0.100 -> 0.109.  Encoder-
    // shaped calls (one query per pixel: tens of thousands of groups per item) win once there are enough items -- 4 clips at
    // 360x640: 1.924 -> 1.733 -- and lose with one clip's 48 (0.556 -> 0.987; BASELINE configs[1], 64 items: 0.644 -> 0.688).
    const bool enough = items >= 128 && per_item >= 512 && (per_item <= 8192 || items >= 192);
    // (after the owner kernel's band rotation became conditional -- msda_scatter.hip -- the 96-pixel last level of the SwinL
    // pyramid pays as well: 16 clips 0.679 -> 0.636; the 273-pixel one of 800x1333 is level: 0.514 -> 0.510)
    if (sc.mfma_tiles && k.scatter_mfma < 0 && !(enough && (p.L - sc.l0 == 2 || px >= 64))) { sc.l0 = p.L; sc.mfma_tiles = 0; }
}

// Items of the owner-computes scatter in image order for long candidate ranges of a TEMPORAL call (the encoder's fused call: the
// frames of one band run side by side and share the rows and points of the queries near it), when the host knows the band count
// (scatter_order 1, MSDA_SCATTER_DBG kSdbgLevelOrder: the level-by-level order).  Plain calls keep the heaviest-first order: measured on one box,
// image order / level order: 800x1333 T = 6 one clip 2.76 / 2.86 ms, 360x640 T = 6 0.54 / 0.55, but the single-frame
// encoder call of BASELINE configs[1] (N = 8, bf16) 0.92 / 0.63 and the SwinL one (N = 6, fp16) 0.23 / 0.17 -- with
// `clip` outermost the batch is 8 serial tails.
// (round 4, after the per-item fixed costs shrank: at 360x640, Lq = 4820, image order is now the slower one, 0.555 / 0.529)
// (a pinned route, msda_pin_route scatter_order: 1 = level order, 2 = image order wherever the bands can be sorted)
static bool owner_image_order(const Params &p, const Knobs &k, int own_levels, long long pix)
{
    if (!((p.Lq >= 8192 && p.frames > 1) || k.scatter_order == 2) || !p.shapes_host || k.scatter_order == 1) return false;
    int bands = 0;
    for (int l = 0; l < own_levels; ++l) {
        const long long H = p.shapes_host[2 * l], W = p.shapes_host[2 * l + 1];
        if (H <= 0 || W <= 0) return false;         // (degenerate level: the device counts its bands differently)
        const long long nb = own_band_count(H, W, pix);       // (0: a "direct" level is one item)
        bands += nb > 0 ? (int)nb : 1;
    }
    return bands <= kOwnMaxSorted;
}

// Which scatter produces grad_value, and (since the gather pass leaves culling records only for the levels the owner kernel
// will walk band by band -- 16 clips: 0.400 -> 0.394 ms, 22 MB of stores less) which records the gather pass leaves: settled
// BEFORE the gather pass.  `grads` without kGradValue: no scatter follows, rec_mask = 0.
ScatterPlan plan_scatter(int dtype, const Shape &s, const Params &p, const Knobs &k, int grads)
{
    ScatterPlan sc;
    if (!scatter_applicable(p, k)) return sc;
    const bool want_value = (grads & kGradValue) != 0;
    const bool owner = owner_scatter_applicable(p, s.esz, k) && (p.cull_points || !p.bbox);
    sc.route = owner ? ScatterPlan::kOwner : ScatterPlan::kLds;
    sc.l0 = p.L;
    if (owner) plan_matrix_pipe(dtype, s, p, k, sc);
    // pixels per band of the owner kernel's instantiation for this call (msda_params.h): the kernel and the rules below count
    // bands with own_band_count at this size (a row wider than kOwnPix is "direct" at every size)
    long long pix = own_band_pixels(dtype, p.gv_storage != 0);
    // FEW-ITEM calls stay on four slots: with about one item per workgroup (at most two per workgroup of the persistent grid,
    // counted at five slots) a launch lasts as long as its heaviest item, and a band of 15 rows is heavier than one of 12 -- one
    // clip of the 360x640 decoder call replayed from a graph, 288 items for 256 workgroups: 0.124 -> 0.130 ms at five slots,
    // with 60 queries 0.0573 -> 0.0606; the SwinL fp16 encoder call image by image + 1.2 % (profiles/own5_ab.log, section 4b).
    // From 16 clips on (3072 items) five slots win; between 2 and 16 clips nothing was measured.  Without the host copy of the
    // shapes the items cannot be counted and the call keeps the larger bands.  (MSDA_SCATTER_DBG kSdbgNoFourSlotRule: never -- tests)
    if (owner && pix > kOwnPix && p.shapes_host && (k.scatter_dbg & kSdbgNoFourSlotRule) == 0) {
        long long bands = 0;
        for (int l = 0; l < sc.l0; ++l) {
            const long long nb = own_band_count<long long>(p.shapes_host[2 * l], p.shapes_host[2 * l + 1], pix);
            bands += nb > 0 ? nb : 1;
        }
        if ((long long)p.groups * p.M * bands <= 2LL * persistent_grid(s.cus)) pix = kOwnPix;
    }
    sc.own_pix = (int)pix;
    // Culling records: not for the matrix-pipe levels, and not for levels of ONE band (the host copy of the shapes says so: every
    // group is a candidate of the only band, the owner kernel takes all its points) -- the 23x40 level of the 360x640 pyramid; at
    // five pixels per owner quad the 25x42 level of the 800x1333 one as well.  The device counts the bands with the same function
    // at the same size (Params::own_pix picks its instantiation): a level it cut in two where the host saw one would take every
    // group as a candidate of both bands (correct, and slower); the other way round records would be written and never read.
    if (owner && !k.bwd_all_records) {
        for (int l = sc.l0; l < p.L && l < 32; ++l) sc.rec_mask &= ~(1u << l);
        for (int l = 0; p.shapes_host && l < sc.l0 && l < 32; ++l) {
            const long long H = p.shapes_host[2 * l], W = p.shapes_host[2 * l + 1];
            if (H > 0 && W > 0 && own_band_count(H, W, pix) == 1) sc.rec_mask &= ~(1u << l);
        }
    }
    if (!want_value) sc.rec_mask = 0;
    // Does the full call's gather pass leave (min, max) interval records?  A call without kGradValue leaves no records and needs
    // no workspace, but takes the full call's kernel: the one a full call with a workspace of msda_backward_workspace_bytes()
    // takes (what the Python binding always passes).
    sc.interval_records = want_value ? (p.bbox != nullptr && !p.cull_points)
                                     : (k.bwd_cull != 0 && !(k.bwd_cull != 2 && owner_scatter_applicable(p, s.esz, k)));
    if (!owner) return sc;
    // When every level's row fits a band (the host copy of the shapes says so) no pixel takes the float-atomic branch, and the
    // zero-fill of the pixels outside the levels -- normally none -- rides in the scatter kernel's prologue (launch flag kOwnFusedZero) instead of
    // a launch of its own in front of it: one dependent dispatch less per backward (one clip from a HIP graph 0.127 -> see r04 logs)
    sc.fused_zero = p.shapes_host != nullptr && (k.scatter_dbg & kSdbgSeparateZero) == 0;
    for (int l = 0; sc.fused_zero && l < p.L; ++l) sc.fused_zero = p.shapes_host[2 * l + 1] > 0 && own_row_fits(p.shapes_host[2 * l + 1]);
    sc.image_order = owner_image_order(p, k, sc.l0, pix);
    sc.run_owner = !(sc.mfma_tiles && k.scatter_part == 2);
    sc.run_mfma = sc.mfma_tiles && k.scatter_part != 1;
    return sc;
}

// ---- backward: gather pass --------------------------------------------------------------------------------------
// Workgroups per (clip, head, frame) of the resident-slab gather pass with one source frame per workgroup, 0 = not that grid.
// One source frame per workgroup (round 4): the gather pass carries nothing from frame to frame, so (clip, head, frame,
// half of the clip's tiles) workgroups stage ONE slab each and meet at no barrier afterwards -- a quarter of the staging
// traffic of (clip, head, part) workgroups walking the frames.  Pays from ~8 clips on (same box, fp32:
// 8 / 16 / 32 clips 0.245 -> 0.229 / 0.48 -> 0.44 / 0.881 -> 0.874 ms; 4 clips with TWO workgroups per frame
// 0.100 -> 0.122 -- with four it pays there too, see below).
// SMALL batches -- the one clip per GPU DeVIS itself issues (main.py:85) -- cannot fill the chip with (clip, head, part)
// workgroups at all (tpw = 0) and used to fall to the tile kernels: with the frames as a workgroup index 1 / 2 clips make
// 192 / 384 workgroups of <= 2 tiles per wave (same box, gather pass of 1 clip fp32 0.058 -> 0.040 ms, bf16 0.074 -> 0.037;
// 2 clips 0.088 -> 0.063, 0.094 -> 0.065; profiles/r04_logs/small_batch_sweep.log).  `small`: set when that rule chose it.
static int gather_frame_parts(const Shape &s, const Params &p, const Knobs &k, int tpw, int parts, bool &small)
{
    small = false;
    if (k.bwd_rs_fsplit >= 0) return k.bwd_rs_fsplit;
    const int mode = k.bwd_rs, esz = s.esz, cus = s.cus;
    // (round 4, second sweep, profiles/r04_logs/gather_fsplit_sweep.log: 2-byte types gain 5-10 % at 8 / 16 / 32 / 64 clips;
    // fp32 gains 4-11 % up to 32 clips and loses 3 % at 64)
    // Only while the levels outside the slab are small: the frame-split grid keeps 16 frame maps per XCD in flight instead
    // of 4 -- fine for the 360x640 pyramid's level 0 (460 KB in fp32), 12-16 % SLOWER on the 800x1333 one (levels 0-1
    // outside: 2.7 MB per map; 16 clips bf16 0.531 -> 0.618 ms, fp32 0.906 -> 1.012).
    const long long wgs = s.clips * p.M * p.frames * 2;
    // (route audit, profiles/r04_logs/route_audit_*.log: SwinL pyramid in fp32, 737 KB outside, 8-32 clips 14-20 % slower)
    const bool small_outside = s.outside <= (512ll << 10);
    // (encoder-shaped batches: 8 clips at 360x640 in fp32 2.50 -> 2.80 ms on this grid, in bf16 2.49 -> 2.13)
    if (p.frames > 1 && small_outside && wgs >= 3LL * cus && (esz == 2 || (wgs < 24LL * cus && p.Lq != p.S))) return 2;
    // (2-byte encoder-shaped batches one size below that: four workgroups per frame at 4 clips, 1.23 -> 1.13 ms at 360x640,
    // 1.94 -> 1.80 on the SwinL pyramid)
    if (esz == 2 && p.frames > 1 && p.Lq == p.S && small_outside && 2 * wgs >= 3LL * cus) return 4;
    // fp32 batches whose (clip, head, part) workgroups are a single round over the CUs (4 clips): four workgroups per (clip,
    // head, frame) balance better -- 0.103 -> 0.099 / 0.177 -> 0.149 / 0.259 -> 0.242 ms on the three audited pyramids;
    // 2-byte types lose 2-14 % there and stay, and so do encoder-shaped calls (one clip is 232 workgroups of 4 tiles: 0.36 vs
    // 0.47 ms on the frame-split grid)
    if (tpw && esz == 4 && mode == -1 && p.frames > 1 && p.Lq != p.S && s.l0_host <= p.L - 1 && s.clips * p.M * parts <= cus) return 4;
    if (!tpw && mode == -1 && p.frames > 1 && s.l0_host <= p.L - 1 && s.clips * p.M * p.frames * 4 >= cus / 2) {
        // (2-byte types with two clips: 2 workgroups per (clip, head, frame) -- 0.067 -> 0.056 ms; fp32 the other way round)
        // Whatever the query count -- DeVIS's shipped configs run 60 queries per frame (YouTube-VIS) and 180 (OVIS), 24 / 72
        // tiles per clip: one clip of 60 queries 0.050 -> 0.020 ms in fp32, 0.065 -> 0.020 in fp16, 10 queries 0.042 -> 0.018
        // (the tile kernels walk a chain of 24 dependent gather batches per wave however few rows there are)
        small = true;
        return (esz == 2 && s.clips * p.M * p.frames * 2 >= 3LL * cus / 4) ? 2 : 4;
    }
    return 0;
}

GatherPlan plan_gather(const Shape &s, const Params &p, const Knobs &k, int grads, bool interval_records)
{
    GatherPlan g;
    // grad_value alone: the records (and zeroed tickets) the gather pass would have left, from the sampling locations only
    if (!(grads & kGradSampling)) { g.kind = GatherPlan::kRecordsOnly; return g; }
    if (interval_records) return g;                 // (only the tile kernel writes interval records)
    if (window_route(s, p, k, k.bwd_win, g.win)) { g.kind = GatherPlan::kWindow; return g; }
    if (!s.rs_ok) return g;
    // resident-slab gather pass: same applicability rule as the forward
    const int mode = k.bwd_rs;
    int tpw = rs_tiles_per_wave(p, s.rs_tiles_per_clip, s.outside, mode == 1, s.l2_budget,
                                s.l0_host >= 2 ? 2 : 4, s.cus);      // (as in the forward: configs[1] gather pass 0.407 -> 0.395 ms)
    if (k.bwd_rs_tpw > 0) tpw = k.bwd_rs_tpw;
    const int parts = tpw ? (s.rs_tiles_per_clip + tpw * kRsWaves - 1) / (tpw * kRsWaves) : 1;       // (L2: see the forward)
    const bool want = mode == 1 || (mode == -1 && tpw && s.l0_host <= p.L - 1);
    bool want_small = false;
    const int fparts = gather_frame_parts(s, p, k, tpw, parts, want_small);
    const long long frame_grid = s.clips * p.M * p.frames * fparts, grid = s.clips * p.M * parts;
    if ((want || want_small) && fparts > 0 && p.frames > 1 && frame_grid <= 0x7fffffffLL) {
        g.kind = GatherPlan::kSlab; g.parts = fparts; g.frame_split = 1; g.grid = (unsigned)frame_grid;
    } else if (want && grid <= 0x7fffffffLL) {
        g.kind = GatherPlan::kSlab; g.parts = parts; g.grid = (unsigned)grid;
    }
    g.walk_down = g.kind == GatherPlan::kSlab && walk_down_rule(s, p, k);
    return g;
}

// Shapes the 16-byte-lane kernels take: D a multiple of the lane vector with 64 / G rows per wave, aligned bases,
// 32-bit element offsets inside a clip.
bool fast_path_takes(int dtype, const Params &p, const Knobs &k, bool bwd)
{
    if (dtype == MSDA_F64) return false;
    const int esz = elem_bytes(dtype), VEC = 16 / esz;
    if (p.D % VEC) return false;
    const int G = p.D / VEC;
    if (G != 1 && G != 2 && G != 4 && G != 8 && G != 16 && G != 32 && G != 64) return false;
    // every 16-B lane vector must be aligned: bases 16-B aligned and D a multiple of VEC
    if (!aligned16(p.value) || (!bwd && !aligned16(p.out)) || (bwd && (!aligned16(p.grad_out) || !aligned16(p.grad_value))))
        return false;
    // element offsets inside one clip slab are 32-bit in the tap records
    if ((int64_t)p.frames * p.S * p.M * p.D >= 0x7fffffffLL || (int64_t)p.frames * p.S * p.v_pix >= 0x7fffffffLL ||
        (int64_t)p.frames * p.S * p.v_pix * (int64_t)esz >= (int64_t)kOobBytes)  // gather_load: 32-bit byte offsets < kOobBytes
        return false;
    if (p.v_clip % VEC || p.v_head % VEC || p.v_pix % VEC) return false;
    // the one-kernel backward scatters grad_value (always dense) at value's offsets
    if (bwd && !scatter_applicable(p, k) && !standard_value_layout(p)) return false;
    if (tile_lds_bytes(kWave / G, p.LA + p.LB, bwd) > 60 * 1024) return false;
    return true;
}

long long workspace_table_bytes(int batch, int num_query, int num_heads, int virtual_levels)
{
    return (long long)batch * num_query * num_heads * virtual_levels * 8;
}

// ticket counters + per-point culling records + their 64-query block summaries
long long workspace_need(int batch, int num_query, int num_heads, int virtual_levels)
{
    const long long nblk = (num_query + kCullBlock - 1) / kCullBlock;
    return MSDA_BWD_WORKSPACE_BYTES + workspace_table_bytes(batch, num_query, num_heads, virtual_levels) +
           (long long)batch * num_heads * virtual_levels * nblk * 8;
}

// Pixel tiles (of 32) the matrix-pipe scatter needs for `pixels` coarse pixels, or 0 when they do not fit its largest kernel.
int mfma_scatter_tiles(long long pixels)
{
    for (int mt : {2, 4, 6, 8, 10})
        if (pixels + 1 <= mfma_rows(mt)) return mt;
    return 0;
}

long long det_maxima_bytes(long long clips, int num_heads)
{
    return (clips * num_heads * 16 + 255) / 256 * 256;
}

long long det_workspace_bytes(long long clips, int frames, int spatial_size, int num_heads, int channels)
{
    const long long elems = clips * frames * spatial_size * (long long)num_heads * channels;
    return det_maxima_bytes(clips, num_heads) + elems * 8 + (elems + 7) / 8 * 4;
}

}  // namespace plan
}  // namespace msda
