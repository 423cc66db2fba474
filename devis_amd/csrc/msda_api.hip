// msda_api.hip -- host side of libmsda_hip.so: the extern "C" ABI of include/msda.h, argument checks, workspace layout, the
// per-device caches, and the launching of what the planner chose (msda_plan.hip: which kernel family takes a shape; msda_knobs.hip:
// the test knobs and the pinned routes).  The kernels live in the other translation units of this directory.
#include "msda_common.h"
#include "msda_det.h"
#include "msda_plan.h"

namespace msda {

using namespace plan;

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, const char *detail)
{
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

thread_local char g_route[512] = "";     // kernels launched by the last entry-point call of this thread (msda_last_route)

int check_launch(const char *what)
{
    const size_t used = strlen(g_route);
    if (used + 3 < sizeof(g_route)) snprintf(g_route + used, sizeof(g_route) - used, "%s%s", used ? "; " : "", what);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return MSDA_ERR_HIP;
    }
    return MSDA_OK;
}

namespace {

int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
    return dev;
}

}  // namespace

// ---- per-device caches --------------------------------------------------------------------------------------
int device_cus()
{
    static int cus[kMaxDevices];        // 0 = not asked yet; benign race: every thread computes the same value
    const int dev = current_device();
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

int grant_lds(const void *kernel, size_t bytes, LdsGrant &granted, const char *what)
{
    const int dev = current_device();
    if (bytes <= granted.bytes[dev]) return MSDA_OK;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        return fail(MSDA_ERR_HIP, "msda: cannot reserve the LDS budget of %s", what);
    granted.bytes[dev] = bytes;
    return MSDA_OK;
}

namespace {

int zero_grad_value(int grad_value_dtype, void *grad_value, int groups, int S, int M, int D, void *stream)
{
    if (grad_value_dtype < MSDA_F32 || grad_value_dtype > MSDA_F16) return fail(MSDA_ERR_DTYPE, "msda: unknown dtype code%s");
    if (!grad_value) return fail(MSDA_ERR_ARG, "msda backward: null grad_value%s");
    const size_t bytes = (size_t)groups * S * M * D * (size_t)elem_bytes(grad_value_dtype);
    if (hipMemsetAsync(grad_value, 0, bytes, static_cast<hipStream_t>(stream)) != hipSuccess)
        return fail(MSDA_ERR_HIP, "msda backward: hipMemsetAsync(grad_value) failed%s");
    return MSDA_OK;
}

int launch_forward(int dtype, const Params &p, const Knobs &k, const Shape &s, hipStream_t stream)
{
    const FwdPlan f = plan_forward(s, p, k);
    switch (f.family) {
        case FwdPlan::kWindow: return launch_fwd_win(dtype, p, f.win, stream);
        case FwdPlan::kSlab: return launch_fwd_rs(dtype, f.nt, f.body_l0, p, f.parts, (unsigned)(s.clips * p.M * f.parts), stream);
        default: return launch_fwd_tile(dtype, s.G, p, s.blocks, f.lds, stream, f.waves);
    }
}

// The backward's gather pass + scatter on the tile / resident-slab / resident-window / scatter kernels.  `grads`: the gradient
// groups asked for (msda_backward_grads) -- without kGradValue the gather pass runs as in the full call but leaves no culling
// records and nothing follows it; without kGradSampling the culling-records kernel stands in for the gather pass in front of
// the full call's scatter.
int launch_backward(int dtype, const Params &p, const Knobs &k, const Shape &s, hipStream_t stream, int grads)
{
    const bool want_value = (grads & kGradValue) != 0, want_sampling = (grads & kGradSampling) != 0;
    const ScatterPlan sc = plan_scatter(dtype, s, p, k, grads);
    Params pq = p;                                 // the gather pass's view
    pq.rec_mask = sc.rec_mask;
    if (!want_value) { pq.bbox = nullptr; pq.bsum = nullptr; pq.workspace = nullptr; }      // no scatter follows: no records, no tickets
    if (p.gv_storage && sc.route != ScatterPlan::kOwner)      // (only the owner-computes scatter writes the storage type)
        return fail(MSDA_ERR_ARG, "msda backward: this call needs grad_value in the arithmetic type (see msda_grad_value_dtype)%s");
    if (sc.route == ScatterPlan::kAtomic) {
        // the one-kernel backward; without grad_value without its atomics: no records, no tickets, nothing to zero-fill
        if (!want_value) return launch_bwd_tile(dtype, s.G, false, pq, s.blocks, tile_lds_bytes(s.RPW, p.LA + p.LB, true), stream);
        if (const int rc = zero_grad_value(MSDA_F32, p.grad_value, p.groups, p.S, p.M, p.D, stream)) return rc;
        return launch_bwd_tile(dtype, s.G, true, p, s.blocks, s.tile_lds, stream, !want_sampling);
    }
    // MSDA_BWD_PHASES (measurement hook for bench.py): 1 = gather pass only, 2 = scatter pass only
    // (needs the workspace a previous gather pass filled), 3 = both (default)
    int rc = MSDA_OK;
    if (k.bwd_phases & 1) {
        const GatherPlan g = plan_gather(s, p, k, grads, sc.interval_records);
        switch (g.kind) {
            case GatherPlan::kRecordsOnly: rc = pq.workspace ? launch_cull_records(dtype, pq, stream) : MSDA_OK; break;
            case GatherPlan::kWindow: rc = launch_bwd_win(dtype, pq, g.win, stream); break;
            case GatherPlan::kSlab:
                pq.walk_down = g.walk_down ? 1 : 0;
                rc = launch_bwd_rs(dtype, s.l0_host, pq, g.parts, g.grid, stream, g.frame_split);
                break;
            default: rc = launch_bwd_tile(dtype, s.G, false, pq, s.blocks, s.tile_lds, stream);
        }
        if (!rc && pq.cull_points && pq.bsum) rc = launch_cull_summary(pq, stream);      // block summaries of the records just written
        if (rc) return rc;
    }
    if (!(k.bwd_phases & 2) || !want_value) return rc;
    const unsigned grid = persistent_grid(s.cus);
    if (sc.route == ScatterPlan::kOwner) {
        // owner-computes scatter: no float atomics; pixels outside its bands are zero-filled first
        if (!sc.fused_zero) {
            rc = launch_zero_unowned(p, kOwnRowPix * p.D, p.gv_storage ? 2 : 4, stream);      // (rows own_row_fits takes are the scatter's)
            if (rc) return rc;
        }
        Params pg = p;
        pg.own_levels = sc.l0;
        pg.rec_mask = sc.rec_mask;
        pg.own_pix = sc.own_pix;
        if (sc.run_owner)
            rc = launch_scatter_grp(dtype, p.gv_storage != 0, pg, grid * (1024 / kOwnThreads), (k.scatter_dbg & kSdbgOwnMask) | (sc.fused_zero ? kOwnFusedZero : 0),
                                    sc.image_order, stream);
        if (rc || !sc.run_mfma) return rc;
        return launch_scatter_mfma(dtype, p.gv_storage != 0, p, sc.l0, sc.mfma_tiles, stream);
    }
    // LDS-atomic scatter: 144 KiB of 8-byte accumulators per workgroup
    const int cap_bytes = k.scatter_lds_kb * 1024;
    rc = launch_zero_unowned(p, cap_bytes / 8, 4, stream);
    if (rc) return rc;
    return launch_scatter_lds(dtype, p.D / 4, p, grid, cap_bytes, k.scatter_dbg & kSdbgLdsMask, stream);      // 4 channels per lane
}

int run(int dtype, const Params &p_in, const Knobs &k, bool bwd, hipStream_t stream, int grads = kGradAll)
{
    if (dtype < MSDA_F32 || dtype > MSDA_F16_LOC32) return fail(MSDA_ERR_DTYPE, "msda: unknown dtype code%s");
    Params p = p_in;
    p.own_levels = p.L;
    p.rec_mask = ~0u;
    p.own_pix = kOwnPix;
    p.walk_down = 0;
    p.dbg = k.dbg;
    // culling records per point (4 x int16) when the owner-computes scatter will read them; (min, max) intervals for the
    // LDS-atomic scatter (MSDA_BWD_CULL=2 forces them)
    p.cull_points = bwd && p.bbox && k.bwd_cull != 2 && owner_scatter_applicable(p, elem_bytes(dtype), k);
    if (!p.cull_points) p.bsum = nullptr;
    p.wide_stores = bwd && aligned16(p.glocA) && aligned16(p.gawA) && (p.LB == 0 || (aligned16(p.glocB) && aligned16(p.gawB))) &&
                    (k.dbg & kDbgNarrowStores) == 0;          // (measurement: keeps the narrow stores)
    p.wide_loads = aligned16(p.locA) && aligned16(p.awA) && (p.LB == 0 || (aligned16(p.locB) && aligned16(p.awB))) &&
                   (k.dbg & kDbgNarrowLoads) == 0;           // (measurement: keeps the narrow loads)
    if (p.groups == 0 || p.Lq == 0) return MSDA_OK;
    if (!k.force_generic && fast_path_takes(dtype, p, k, bwd)) {
        Shape s;
        if (!shape_of(dtype, p, bwd, device_cus(), s)) return fail(MSDA_ERR_ARG, "msda: problem too large for one launch%s");
        return bwd ? launch_backward(dtype, p, k, s, stream, grads) : launch_forward(dtype, p, k, s, stream);
    }
    if (p.gv_storage) return fail(MSDA_ERR_ARG, "msda backward: this call needs grad_value in the arithmetic type (see msda_grad_value_dtype)%s");
    return launch_generic(dtype, p, bwd, stream, grads);
}

// `grad_value_dtype` of the backward entry points: the arithmetic type, or the 16-bit storage type where allowed.
int set_grad_value_dtype(int dtype, int grad_value_dtype, Params &p)
{
    const int arith = dtype == MSDA_F64 ? MSDA_F64 : MSDA_F32;
    p.gv_storage = 0;
    if (grad_value_dtype == arith) return MSDA_OK;
    if (grad_value_dtype != storage_dtype(dtype) || !storage_typed_grad_value_ok(dtype, p, env_knobs()))
        return fail(MSDA_ERR_ARG, "msda backward: grad_value_dtype must be what msda_grad_value_dtype returns for this call%s");
    p.gv_storage = 1;
    return MSDA_OK;
}

// The operator's inputs and sizes as Params.  The plain entry points are the temporal ones with frames = 1, window = 0 and no
// frame table or temporal arrays (hence LB = 0, PB = 1).
Params op_params(const void *value, const int64_t *shapes, const int64_t *lsi, const int32_t *ftab, const void *locA,
                 const void *awA, const void *locB, const void *awB, int clips, int frames, int window, int S, int M, int D,
                 int L, int Lq, int Pc, int Pt, const int64_t *shapes_host)
{
    Params p;
    memset(&p, 0, sizeof(p));
    p.value = value; p.shapes = shapes; p.lsi = lsi; p.ftab = ftab;
    p.locA = locA; p.awA = awA; p.locB = locB; p.awB = awB;
    p.groups = clips * frames; p.frames = frames; p.window = window;
    p.S = S; p.M = M; p.D = D; p.L = L; p.Lq = Lq;
    p.LA = L; p.PA = Pc; p.LB = window * L; p.PB = window > 0 ? Pt : 1;
    p.shapes_host = shapes_host;
    return p;
}

// The checks of the forward and backward entry points in front of their empty-call test.  `fn` names the entry point in the
// messages; the plain ones take any frames / window / points here (theirs are fixed, num_point is checked with the pointers).
int check_sizes(const char *fn, bool temporal, const Params &p, int clips)
{
    if (!p.value || !p.shapes || !p.lsi) return fail(MSDA_ERR_ARG, "msda: null pointer argument%s");
    if (clips < 0 || p.Lq < 0 || p.S <= 0 || p.M <= 0 || p.D <= 0 || p.L <= 0)
        return fail(MSDA_ERR_ARG, "msda: sizes must be positive%s");
    if (temporal && (p.frames <= 0 || p.window < 0 || p.PA <= 0 || (p.window > 0 && p.PB <= 0)))
        return fail(MSDA_ERR_ARG, "%s: bad frames/window/points", fn);
    return MSDA_OK;
}

// `value_strides` (host pointer, may be null): element strides {between clips, between heads, between pixels}
// of `value`; null = the standard dense [groups, S, M, D].
int set_value_strides(Params &p, const int64_t *vs)
{
    p.v_clip = (int64_t)p.frames * p.S * p.M * p.D; p.v_head = p.D; p.v_pix = p.M * p.D;
    if (!vs) return MSDA_OK;
    if (vs[0] < 0 || vs[1] < 0 || vs[2] <= 0 || vs[2] > 0x7fffffffLL)
        return fail(MSDA_ERR_ARG, "msda: bad value_strides%s");
    p.v_clip = vs[0]; p.v_head = vs[1]; p.v_pix = (int)vs[2];
    return MSDA_OK;
}

void attach_workspace(Params &p, const Knobs &k, void *workspace, long long bytes)
{
    const int batch = p.groups, num_query = p.Lq, num_heads = p.M, vl = p.LA + p.LB;
    p.workspace = (workspace && bytes >= MSDA_BWD_WORKSPACE_BYTES) ? static_cast<unsigned *>(workspace) : nullptr;
    p.bbox = nullptr;
    p.bsum = nullptr;
    if (p.workspace && bytes >= workspace_need(batch, num_query, num_heads, vl) && k.bwd_cull != 0) {
        p.bbox = reinterpret_cast<int *>(p.workspace) + MSDA_BWD_WORKSPACE_BYTES / 4;
        // block summaries only pay for long candidate ranges (and index (group, head, level) rows with 32 bits)
        if (num_query >= 2048 && (long long)batch * num_heads * vl < 0x7fffffffLL)
            p.bsum = p.bbox + workspace_table_bytes(batch, num_query, num_heads, vl) / 4;
    }
}

// MSDA_GRAD_DETERMINISTIC.  grad_loc / grad_attn: a gather pass whose sums do not depend on a row's place in the batch --
// the tile kernel (G lanes per row, the same lanes and order for every row) where the fast path takes the call, else the
// generic kernel (one wave per row); the resident-slab and resident-window passes are repeatable but not that (their
// grad_loc differs in the last bits when the queries are permuted).  grad_value: maxima, then route (b) -- the LDS-band
// scatter with int64 bands, for fp32 / 16-bit calls the LDS scatter takes -- or route (a), the any-shape int64-atomic
// scatter; both give the same bits (msda_det.h).  MSDA_DET_ROUTE (hooks) forces one: 1 = (a), 2 = (b).
int run_det(int dtype, const Params &p_in, const Knobs &k, void *workspace, long long workspace_bytes, hipStream_t stream, int grads)
{
    if (dtype < MSDA_F32 || dtype > MSDA_F16_LOC32) return fail(MSDA_ERR_DTYPE, "msda: unknown dtype code%s");
    const long long need = det_workspace_bytes(p_in.groups / p_in.frames, p_in.frames, p_in.S, p_in.M, p_in.D);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return fail(MSDA_ERR_ARG, "msda backward: MSDA_GRAD_DETERMINISTIC needs a 256-byte aligned workspace of msda_backward_workspace_bytes_det() bytes%s");
    Params p = p_in;
    p.workspace = nullptr; p.bbox = nullptr; p.bsum = nullptr;          // no tickets (static item stride), no culling records
    p.own_levels = p.L; p.rec_mask = 0; p.cull_points = 0;
    if (p.groups == 0 || p.Lq == 0) return MSDA_OK;
    const bool band_ok = dtype != MSDA_F64 && scatter_applicable(p, k);
    if (k.det_route == 2 && !band_ok) return fail(MSDA_ERR_ARG, "msda backward: MSDA_DET_ROUTE=2 (LDS bands) does not take this call%s");
    int rc = MSDA_OK;
    if (grads & kGradSampling) {
        Params ps = p;
        ps.grad_value = nullptr; ps.gv_storage = 0;
        if (!k.force_generic && fast_path_takes(dtype, ps, k, true)) {
            Shape s;                    // (p.bbox is null: the tile kernel's LDS without interval records)
            if (!shape_of(dtype, p, true, device_cus(), s)) return fail(MSDA_ERR_ARG, "msda: problem too large for one launch%s");
            rc = launch_bwd_tile(dtype, s.G, false, ps, s.blocks, s.tile_lds, stream);
        } else {
            rc = launch_generic(dtype, ps, true, stream, kGradSampling);
        }
        if (rc) return rc;
    }
    DetArgs d;
    rc = launch_det_prepare(dtype, p, workspace, d, stream);
    if (rc) return rc;
    if (band_ok && k.det_route != 1) {
        rc = launch_scatter_lds_det(dtype, p.D / 4, p, persistent_grid(device_cus()), k.scatter_lds_kb * 1024, d, stream);
    } else {
        rc = launch_det_scatter_any(dtype, p, d, stream);
    }
    if (rc) return rc;
    return launch_det_convert(dtype, p, d, stream);
}

// The forward entry points; `temporal`: msda_temporal_forward (see check_sizes).
int forward(const char *fn, bool temporal, int dtype, Params p, int clips, void *out, const int64_t *value_strides, void *stream)
{
    g_err[0] = 0; g_route[0] = 0;
    int rc = check_sizes(fn, temporal, p, clips);
    if (rc) return rc;
    if (clips == 0 || p.Lq == 0) return MSDA_OK;
    if (!p.locA || !p.awA || !out || p.PA <= 0 || (p.window > 0 && (!p.ftab || !p.locB || !p.awB)))
        return fail(MSDA_ERR_ARG, temporal ? "%s: null pointer argument" : "%s: null pointer or non-positive num_point", fn);
    p.out = out;
    rc = set_value_strides(p, value_strides);
    if (rc) return rc;
    return run(dtype, p, call_knobs(false, dtype, p), false, static_cast<hipStream_t>(stream));
}

// The backward entry points; `grad_locB` / `grad_awB`: the temporal arrays' gradients (null for the plain ones).
int backward(const char *fn, bool temporal, int grads, int dtype, Params p, int clips, const void *grad_out, void *grad_value,
             int grad_value_dtype, void *grad_locA, void *grad_awA, void *grad_locB, void *grad_awB, void *workspace,
             long long workspace_bytes, const int64_t *value_strides, void *stream)
{
    g_err[0] = 0; g_route[0] = 0;
    if ((grads & ~(kGradAll | kGradDet)) || ((grads & kGradDet) && !(grads & kGradValue)))
        return fail(MSDA_ERR_ARG, "msda backward: grads must be a mask of MSDA_GRAD_VALUE and MSDA_GRAD_SAMPLING (MSDA_GRAD_DETERMINISTIC only with MSDA_GRAD_VALUE)%s");
    const bool det = (grads & kGradDet) != 0;
    grads &= kGradAll;
    if (grads == 0) return MSDA_OK;
    const bool want_value = (grads & kGradValue) != 0, want_sampling = (grads & kGradSampling) != 0;
    int rc = check_sizes(fn, temporal, p, clips);
    if (rc) return rc;
    if (clips == 0) return MSDA_OK;
    if (p.Lq == 0) return want_value ? zero_grad_value(grad_value_dtype, grad_value, p.groups, p.S, p.M, p.D, stream) : MSDA_OK;
    if (!p.locA || !p.awA || !grad_out || (want_value && !grad_value) || (want_sampling && (!grad_locA || !grad_awA)) || p.PA <= 0 ||
        (p.window > 0 && (!p.ftab || !p.locB || !p.awB || (want_sampling && (!grad_locB || !grad_awB)))))
        return fail(MSDA_ERR_ARG, temporal ? "%s: null pointer argument" : "%s: null pointer or non-positive num_point", fn);
    p.grad_out = grad_out; p.grad_value = grad_value;
    p.glocA = grad_locA; p.gawA = grad_awA; p.glocB = grad_locB; p.gawB = grad_awB;
    const Knobs k = call_knobs(true, dtype, p);
    attach_workspace(p, k, workspace, workspace_bytes);
    rc = set_value_strides(p, value_strides);
    if (rc) return rc;
    rc = want_value ? set_grad_value_dtype(dtype, grad_value_dtype, p) : MSDA_OK;
    if (rc) return rc;
    if (det) return run_det(dtype, p, k, workspace, workspace_bytes, static_cast<hipStream_t>(stream), grads);
    return run(dtype, p, k, true, static_cast<hipStream_t>(stream), grads);
}

int run_prep(int dtype, const PrepParams &p, bool bwd, void *stream)
{
    if (p.rows < 0 || p.M <= 0 || p.L <= 0 || p.W < 0 || p.Pc <= 0 || (p.W > 0 && p.Pt <= 0) || (p.d != 2 && p.d != 4))
        return fail(MSDA_ERR_ARG, "msda prep: bad sizes (rows, heads, levels, window, points, reference dim)%s");
    if (!p.shapes || !p.ref_c || (p.W > 0 && !p.ref_t)) return fail(MSDA_ERR_ARG, "msda prep: null pointer argument%s");
    if (p.rows == 0) return MSDA_OK;
    return launch_prep(dtype, p, bwd, static_cast<hipStream_t>(stream));
}

}  // namespace
}  // namespace msda

using namespace msda;

extern "C" {

int msda_version(void) { return MSDA_ABI_VERSION; }

const char *msda_build_info(void)
{
    return "abi=14 arch=gfx950";
}

void msda_reload_knobs(void) { load_knobs(); }

int msda_route_key(int backward, int dtype, int clips, int frames, int window, int spatial_size, int num_heads, int channels,
                   int num_levels, int num_query, int num_curr_point, int num_temp_point, const int64_t *spatial_shapes_host,
                   char *buf, int buf_len)
{
    if (!buf || buf_len <= 0 || !spatial_shapes_host || clips <= 0 || frames <= 0) return fail(MSDA_ERR_ARG, "msda_route_key: bad arguments%s");
    const Params p = op_params(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, clips, frames, window, spatial_size,
                               num_heads, channels, num_levels, num_query, num_curr_point, num_temp_point, spatial_shapes_host);
    const int n = route_key(buf, buf_len, backward != 0, dtype, p);
    return n < 0 ? fail(MSDA_ERR_ARG, "msda_route_key: the key does not fit the buffer (or more than 16 levels)%s") : n;
}

int msda_pin_route(const char *key, const char *settings)
{
    if (!key || !key[0]) return fail(MSDA_ERR_ARG, "msda_pin_route: empty key%s");
    if (!pin_route(key, settings)) return fail(MSDA_ERR_ARG, "msda_pin_route: cannot parse the settings (name=value ...)%s");
    return MSDA_OK;
}

void msda_clear_routes(void) { clear_routes(); }

int msda_route_count(void) { return route_count(); }

const char *msda_last_route(void) { return g_route; }

long long msda_backward_workspace_bytes(int batch, int num_query, int num_heads, int virtual_levels)
{
    return workspace_need(batch, num_query, num_heads, virtual_levels);
}

long long msda_backward_workspace_bytes_det(int clips, int frames, int spatial_size, int num_heads, int channels)
{
    if (clips < 0 || frames <= 0 || spatial_size <= 0 || num_heads <= 0 || channels <= 0) return 0;
    return det_workspace_bytes(clips, frames, spatial_size, num_heads, channels);
}

const char *msda_last_error(void) { return g_err; }

int msda_grad_value_dtype(int dtype, int clips, int frames, int window, int spatial_size, int num_heads, int channels,
                          int num_levels, int num_query, int num_curr_point, int num_temp_point,
                          const int64_t *spatial_shapes_host)
{
    const int arith = dtype == MSDA_F64 ? MSDA_F64 : MSDA_F32;
    if (clips <= 0 || frames <= 0 || window < 0 || spatial_size <= 0 || num_heads <= 0 || channels <= 0 || num_levels <= 0 ||
        num_query <= 0 || num_curr_point <= 0)
        return arith;
    const Params p = op_params(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, clips, frames, window, spatial_size,
                               num_heads, channels, num_levels, num_query, num_curr_point, num_temp_point, spatial_shapes_host);
    return storage_typed_grad_value_ok(dtype, p, env_knobs()) ? storage_dtype(dtype) : arith;
}

int msda_forward(int dtype, const void *value, const int64_t *spatial_shapes,
                 const int64_t *level_start_index, const void *sampling_loc, const void *attn_weight,
                 int batch, int spatial_size, int num_heads, int channels, int num_levels,
                 int num_query, int num_point, void *out, const int64_t *value_strides,
                 const int64_t *spatial_shapes_host, void *stream)
{
    return forward("msda_forward", false, dtype,
                   op_params(value, spatial_shapes, level_start_index, nullptr, sampling_loc, attn_weight, nullptr, nullptr, batch, 1,
                             0, spatial_size, num_heads, channels, num_levels, num_query, num_point, 1, spatial_shapes_host),
                   batch, out, value_strides, stream);
}

int msda_backward(int dtype, const void *value, const int64_t *spatial_shapes,
                  const int64_t *level_start_index, const void *sampling_loc,
                  const void *attn_weight, const void *grad_out,
                  int batch, int spatial_size, int num_heads, int channels, int num_levels,
                  int num_query, int num_point,
                  void *grad_value, int grad_value_dtype, void *grad_sampling_loc, void *grad_attn_weight,
                  void *workspace, long long workspace_bytes, const int64_t *value_strides,
                  const int64_t *spatial_shapes_host, void *stream)
{
    return msda_backward_grads(kGradAll, dtype, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_out,
                               batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, grad_value,
                               grad_value_dtype, grad_sampling_loc, grad_attn_weight, workspace, workspace_bytes, value_strides,
                               spatial_shapes_host, stream);
}

int msda_backward_grads(int grads, int dtype, const void *value, const int64_t *spatial_shapes,
                        const int64_t *level_start_index, const void *sampling_loc,
                        const void *attn_weight, const void *grad_out,
                        int batch, int spatial_size, int num_heads, int channels, int num_levels,
                        int num_query, int num_point,
                        void *grad_value, int grad_value_dtype, void *grad_sampling_loc, void *grad_attn_weight,
                        void *workspace, long long workspace_bytes, const int64_t *value_strides,
                        const int64_t *spatial_shapes_host, void *stream)
{
    return backward("msda_backward", false, grads, dtype,
                    op_params(value, spatial_shapes, level_start_index, nullptr, sampling_loc, attn_weight, nullptr, nullptr, batch, 1,
                              0, spatial_size, num_heads, channels, num_levels, num_query, num_point, 1, spatial_shapes_host),
                    batch, grad_out, grad_value, grad_value_dtype, grad_sampling_loc, grad_attn_weight, nullptr, nullptr, workspace,
                    workspace_bytes, value_strides, stream);
}

int msda_temporal_forward(int dtype, const void *value, const int64_t *spatial_shapes,
                          const int64_t *level_start_index, const int32_t *frame_table,
                          const void *loc_curr, const void *aw_curr,
                          const void *loc_temp, const void *aw_temp,
                          int clips, int frames, int window, int spatial_size, int num_heads,
                          int channels, int num_levels, int num_query,
                          int num_curr_point, int num_temp_point, void *out, const int64_t *value_strides,
                          const int64_t *spatial_shapes_host, void *stream)
{
    return forward("msda_temporal_forward", true, dtype,
                   op_params(value, spatial_shapes, level_start_index, frame_table, loc_curr, aw_curr, loc_temp, aw_temp, clips, frames,
                             window, spatial_size, num_heads, channels, num_levels, num_query, num_curr_point, num_temp_point,
                             spatial_shapes_host),
                   clips, out, value_strides, stream);
}

int msda_temporal_backward(int dtype, const void *value, const int64_t *spatial_shapes,
                           const int64_t *level_start_index, const int32_t *frame_table,
                           const void *loc_curr, const void *aw_curr,
                           const void *loc_temp, const void *aw_temp, const void *grad_out,
                           int clips, int frames, int window, int spatial_size, int num_heads,
                           int channels, int num_levels, int num_query,
                           int num_curr_point, int num_temp_point,
                           void *grad_value, int grad_value_dtype, void *grad_loc_curr, void *grad_aw_curr,
                           void *grad_loc_temp, void *grad_aw_temp, void *workspace, long long workspace_bytes,
                           const int64_t *value_strides, const int64_t *spatial_shapes_host, void *stream)
{
    return msda_temporal_backward_grads(kGradAll, dtype, value, spatial_shapes, level_start_index, frame_table, loc_curr, aw_curr,
                                        loc_temp, aw_temp, grad_out, clips, frames, window, spatial_size, num_heads, channels,
                                        num_levels, num_query, num_curr_point, num_temp_point, grad_value, grad_value_dtype,
                                        grad_loc_curr, grad_aw_curr, grad_loc_temp, grad_aw_temp, workspace, workspace_bytes,
                                        value_strides, spatial_shapes_host, stream);
}

int msda_temporal_backward_grads(int grads, int dtype, const void *value, const int64_t *spatial_shapes,
                                 const int64_t *level_start_index, const int32_t *frame_table,
                                 const void *loc_curr, const void *aw_curr,
                                 const void *loc_temp, const void *aw_temp, const void *grad_out,
                                 int clips, int frames, int window, int spatial_size, int num_heads,
                                 int channels, int num_levels, int num_query,
                                 int num_curr_point, int num_temp_point,
                                 void *grad_value, int grad_value_dtype, void *grad_loc_curr, void *grad_aw_curr,
                                 void *grad_loc_temp, void *grad_aw_temp, void *workspace, long long workspace_bytes,
                                 const int64_t *value_strides, const int64_t *spatial_shapes_host, void *stream)
{
    return backward("msda_temporal_backward", true, grads, dtype,
                    op_params(value, spatial_shapes, level_start_index, frame_table, loc_curr, aw_curr, loc_temp, aw_temp, clips, frames,
                              window, spatial_size, num_heads, channels, num_levels, num_query, num_curr_point, num_temp_point,
                              spatial_shapes_host),
                    clips, grad_out, grad_value, grad_value_dtype, grad_loc_curr, grad_aw_curr, grad_loc_temp, grad_aw_temp, workspace,
                    workspace_bytes, value_strides, stream);
}

int msda_prep_forward(int dtype, const void *offsets_curr, const void *offsets_temp, const void *logits_curr,
                      const void *logits_temp, const void *ref_curr, const void *ref_temp,
                      const int64_t *spatial_shapes, long long rows, int num_heads, int num_levels, int window,
                      int num_curr_point, int num_temp_point, int ref_dim, long long raw_row_stride,
                      void *loc_curr, void *loc_temp, void *aw_curr, void *aw_temp, void *stream)
{
    g_err[0] = 0; g_route[0] = 0;
    PrepParams p;
    memset(&p, 0, sizeof(p));
    p.off_c = offsets_curr; p.off_t = offsets_temp; p.logit_c = logits_curr; p.logit_t = logits_temp;
    p.ref_c = ref_curr; p.ref_t = ref_temp; p.shapes = spatial_shapes;
    p.loc_c = loc_curr; p.loc_t = loc_temp; p.aw_c = aw_curr; p.aw_t = aw_temp;
    p.rows = rows; p.M = num_heads; p.L = num_levels; p.W = window; p.Pc = num_curr_point;
    p.Pt = window > 0 ? num_temp_point : 1; p.d = ref_dim; p.ld = raw_row_stride;
    if (rows > 0 && (!offsets_curr || !logits_curr || !loc_curr || !aw_curr ||
                     (window > 0 && (!offsets_temp || !logits_temp || !loc_temp || !aw_temp))))
        return fail(MSDA_ERR_ARG, "msda_prep_forward: null pointer argument%s");
    return run_prep(dtype, p, false, stream);
}

int msda_prep_backward(int dtype, const void *grad_loc_curr, const void *grad_loc_temp, const void *grad_aw_curr,
                       const void *grad_aw_temp, const void *aw_curr, const void *aw_temp, const void *ref_curr,
                       const void *ref_temp, const int64_t *spatial_shapes, long long rows, int num_heads,
                       int num_levels, int window, int num_curr_point, int num_temp_point, int ref_dim,
                       long long raw_row_stride, void *grad_offsets_curr, void *grad_offsets_temp,
                       void *grad_logits_curr, void *grad_logits_temp, void *stream)
{
    g_err[0] = 0; g_route[0] = 0;
    PrepParams p;
    memset(&p, 0, sizeof(p));
    p.gloc_c = grad_loc_curr; p.gloc_t = grad_loc_temp; p.gaw_c = grad_aw_curr; p.gaw_t = grad_aw_temp;
    p.aw_c = const_cast<void *>(aw_curr); p.aw_t = const_cast<void *>(aw_temp);
    p.ref_c = ref_curr; p.ref_t = ref_temp; p.shapes = spatial_shapes;
    p.goff_c = grad_offsets_curr; p.goff_t = grad_offsets_temp; p.glogit_c = grad_logits_curr; p.glogit_t = grad_logits_temp;
    p.rows = rows; p.M = num_heads; p.L = num_levels; p.W = window; p.Pc = num_curr_point;
    p.Pt = window > 0 ? num_temp_point : 1; p.d = ref_dim; p.ld = raw_row_stride;
    if (rows > 0 && (!grad_loc_curr || !grad_aw_curr || !aw_curr || !grad_offsets_curr || !grad_logits_curr ||
                     (window > 0 && (!grad_loc_temp || !grad_aw_temp || !aw_temp || !grad_offsets_temp || !grad_logits_temp))))
        return fail(MSDA_ERR_ARG, "msda_prep_backward: null pointer argument%s");
    return run_prep(dtype, p, true, stream);
}

int msda_mask_rows(int dtype, void *rows, const void *padding_mask, long long pixels, long long row_elems,
                   long long row_stride, void *stream)
{
    g_err[0] = 0; g_route[0] = 0;
    const int e = dtype == MSDA_F32 ? 4 : dtype == MSDA_F64 ? 8 : (dtype == MSDA_BF16 || dtype == MSDA_F16) ? 2 : 0;
    if (!e) return fail(MSDA_ERR_DTYPE, "msda: unknown dtype code%s");
    if (pixels < 0 || row_elems <= 0 || row_stride < row_elems)
        return fail(MSDA_ERR_ARG, "msda_mask_rows: bad sizes (pixels, row elements, row stride)%s");
    if (pixels == 0) return MSDA_OK;
    if (!rows || !padding_mask) return fail(MSDA_ERR_ARG, "msda_mask_rows: null pointer argument%s");
    const long long rb = row_elems * e, sb = row_stride * e;
    const int g = (rb % 16 == 0 && sb % 16 == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0) ? 16 : e;
    const long long chunks = rb / g, threads = pixels * chunks;
    if (chunks > 0x7fffffffLL || (threads + 255) / 256 > 0x7fffffffLL)
        return fail(MSDA_ERR_ARG, "msda_mask_rows: tensor too large for one launch%s");
    return launch_mask_rows(g, static_cast<char *>(rows), static_cast<const uint8_t *>(padding_mask), pixels, (int)chunks, sb,
                            (unsigned)((threads + 255) / 256), static_cast<hipStream_t>(stream));
}

}  // extern "C"
