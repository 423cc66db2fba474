// plan_probe.cpp -- the route planner of libmsda_hip.so (devis_amd/csrc/msda_plan.hip, msda_knobs.hip) as a stand-alone host
// program: tests/test_plan_cpu.py builds it with the host compiler under ASan + UBSan, without any ROCm header, and reads the plans
// it prints.  One command per line of stdin, one line of `name=value` fields per command:
//   shape DIR DTYPE CLIPS FRAMES WINDOW S M D L LQ PC PT CUS HxW,HxW,...|- GRADS [vs=CLIP,HEAD,PIX]
//       the plan of one call (DIR f | b; DTYPE an msda_dtype code; `-`: no host copy of the shapes; vs: value_strides), made from
//       the knobs of the environment and the pins, as msda_api.hip makes it for a caller that passes a full workspace
//   pin SETTINGS|- <the fields of shape>      msda_pin_route for that call's key (`-`: remove the pin)
//   parse SETTINGS                            parse_route_settings alone
// The pointers of the Params are fakes (16-byte aligned, never dereferenced); only the host copy of the shapes is real.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "msda_plan.h"

using namespace msda;
using namespace msda::plan;

namespace {

struct Call {
    bool bwd = false;
    int dtype = 0, cus = 0, grads = 0;
    std::vector<int64_t> shapes;
    Params p;
};

void *fake(uintptr_t n) { return reinterpret_cast<void *>(n << 12); }

bool read_call(std::istringstream &in, Call &c)
{
    std::string dir, shapes, extra;
    long long clips, frames, window, S, M, D, L, Lq, Pc, Pt;
    if (!(in >> dir >> c.dtype >> clips >> frames >> window >> S >> M >> D >> L >> Lq >> Pc >> Pt >> c.cus >> shapes >> c.grads)) return false;
    for (long long v : {clips * frames, window * L, S, M, D, L, Lq, Pc, Pt, M * D})
        if (v < 0 || v > INT_MAX) return false;        // (the entry points take ints)
    c.bwd = dir == "b";
    Params &p = c.p;
    memset(&p, 0, sizeof p);
    p.value = fake(1); p.shapes = static_cast<const int64_t *>(fake(2)); p.lsi = static_cast<const int64_t *>(fake(3));
    p.ftab = window > 0 ? static_cast<const int32_t *>(fake(4)) : nullptr;
    p.locA = fake(5); p.awA = fake(6);
    if (window > 0) { p.locB = fake(7); p.awB = fake(8); }
    p.groups = (int)(clips * frames); p.frames = (int)frames; p.window = (int)window;
    p.S = (int)S; p.M = (int)M; p.D = (int)D; p.L = (int)L; p.Lq = (int)Lq;
    p.LA = (int)L; p.PA = (int)Pc; p.LB = (int)(window * L); p.PB = window > 0 ? (int)Pt : 1;
    if (shapes != "-") {
        std::istringstream ss(shapes);
        std::string hw;
        while (std::getline(ss, hw, ',')) {
            const size_t x = hw.find('x');
            if (x == std::string::npos) return false;
            c.shapes.push_back(atoll(hw.substr(0, x).c_str()));
            c.shapes.push_back(atoll(hw.substr(x + 1).c_str()));
        }
        if ((long long)c.shapes.size() != 2 * L) return false;
        p.shapes_host = c.shapes.data();
    }
    p.v_clip = frames * S * M * D; p.v_head = D; p.v_pix = (int)(M * D);
    while (in >> extra) {
        long long a, b, v;
        if (sscanf(extra.c_str(), "vs=%lld,%lld,%lld", &a, &b, &v) != 3 || v <= 0 || v > INT_MAX) return false;
        p.v_clip = a; p.v_head = b; p.v_pix = (int)v;
    }
    if (c.bwd) {
        p.grad_out = fake(9); p.grad_value = fake(10); p.glocA = fake(11); p.gawA = fake(12);
        if (window > 0) { p.glocB = fake(13); p.gawB = fake(14); }
    } else {
        p.out = fake(9);
    }
    return true;
}

void print_shape(Call &c)
{
    Params &p = c.p;
    const Knobs k = call_knobs(c.bwd, c.dtype, p);
    if (c.bwd) {
        // a workspace of msda_backward_workspace_bytes(), as attach_workspace lays it out
        p.workspace = static_cast<unsigned *>(fake(15));
        if (k.bwd_cull != 0) {
            p.bbox = static_cast<int *>(fake(16));
            if (p.Lq >= 2048 && (long long)p.groups * p.M * (p.LA + p.LB) < 0x7fffffffLL) p.bsum = static_cast<int *>(fake(17));
        }
        // grad_value in the type msda_grad_value_dtype names
        p.gv_storage = (c.grads & kGradValue) && storage_typed_grad_value_ok(c.dtype, p, env_knobs());
    }
    // as run() completes the Params
    p.own_levels = p.L; p.rec_mask = ~0u; p.dbg = k.dbg;
    const int esz = elem_bytes(c.dtype);
    p.cull_points = c.bwd && p.bbox && k.bwd_cull != 2 && owner_scatter_applicable(p, esz, k);
    if (!p.cull_points) p.bsum = nullptr;
    p.wide_stores = c.bwd; p.wide_loads = 1;

    WinPlan w;
    memset(&w, 0, sizeof w);
    const bool win = win_plan_cached(p, esz, k.win_min_halo, w);
    printf("knob_fwd_rs=%d knob_scatter_order=%d knob_scatter_dbg=%d knob_forced=%u", k.fwd_rs, k.scatter_order, k.scatter_dbg, k.forced);
    printf(" rs_fits=%d scatter_ok=%d owner_ok=%d gv_storage=%d win=%d win_tiles=%dx%d", (int)rs_fits(p, esz), (int)scatter_applicable(p, k),
           (int)owner_scatter_applicable(p, esz, k), p.gv_storage, (int)win, win ? w.tiles_y : 0, win ? w.tiles_x : 0);
    const bool fast = !k.force_generic && fast_path_takes(c.dtype, p, k, c.bwd);
    printf(" fast=%d", (int)fast);
    Shape s;
    if (!fast || p.groups == 0 || p.Lq == 0) { printf("\n"); return; }
    const bool fits = shape_of(c.dtype, p, c.bwd, c.cus, s);
    printf(" too_large=%d", (int)!fits);
    if (!fits) { printf("\n"); return; }
    printf(" blocks=%u l0_host=%d persistent_grid=%u", s.blocks, s.l0_host, persistent_grid(s.cus));
    if (!c.bwd) {
        const FwdPlan f = plan_forward(s, p, k);
        static const char *const family[] = {"window", "slab", "tile"};
        printf(" family=%s nt=%d parts=%d body_l0=%d waves=%d lds=%zu\n", family[f.family], f.nt, f.parts, f.body_l0, f.waves, f.lds);
        return;
    }
    const ScatterPlan sc = plan_scatter(c.dtype, s, p, k, c.grads);
    static const char *const route[] = {"atomic", "owner", "lds"}, *const kind[] = {"records", "window", "slab", "tile"};
    if (sc.route == ScatterPlan::kAtomic) { printf(" scatter=atomic gather=none\n"); return; }      // (the one-kernel backward)
    const GatherPlan g = plan_gather(s, p, k, c.grads, sc.interval_records);
    printf(" scatter=%s sc_l0=%d mfma_tiles=%d run_owner=%d run_mfma=%d fused_zero=%d image_order=%d rec_mask=%u interval_records=%d",
           route[sc.route], sc.l0, sc.mfma_tiles, (int)sc.run_owner, (int)sc.run_mfma, (int)sc.fused_zero, (int)sc.image_order, sc.rec_mask,
           (int)sc.interval_records);
    printf(" gather=%s g_parts=%d frame_split=%d g_grid=%u\n", kind[g.kind], g.parts, g.frame_split, g.grid);
}

}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, settings;
        if (!(in >> cmd)) continue;
        Call c;
        if (cmd == "shape" && read_call(in, c)) {
            print_shape(c);
        } else if (cmd == "pin" && (in >> settings) && read_call(in, c)) {
            char key[512];
            const bool ok = route_key(key, (int)sizeof key, c.bwd, c.dtype, c.p) > 0 && pin_route(key, settings == "-" ? "" : settings.c_str());
            printf("pinned=%d routes=%d\n", (int)ok, route_count());
        } else if (cmd == "parse" && (in >> settings)) {
            RoutePin pin;
            printf("parsed=%d\n", (int)parse_route_settings(settings.c_str(), pin));
        } else {
            printf("error=bad-line\n");
        }
    }
    return 0;
}
