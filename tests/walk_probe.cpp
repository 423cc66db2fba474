// walk_probe.cpp -- the backward plans of the route planner (devis_amd/csrc/msda_plan.hip, msda_knobs.hip) with the direction in
// which the gather pass takes its work (GatherPlan::walk_down), as a stand-alone host program:
// tests/test_walk_order_cpu.py builds it with the host compiler under ASan + UBSan and reads what it prints.  The twin of
// tests/plan_probe.cpp for the backward of one call; one line of stdin per call, one line of `name=value` fields per line:
//   DTYPE CLIPS FRAMES WINDOW LQ CUS HxW,HxW,...
// (DTYPE an msda_dtype code; 8 heads of 32 channels, 4 points per level, all gradients, the standard value layout; the plans are
// made from the knobs of the environment, as msda_api.hip makes them for a caller that passes a full workspace).  Every field of
// both plans is printed: a test that compares two lines field by field sees whatever else a rule changed.
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

void *fake(uintptr_t n) { return reinterpret_cast<void *>(n << 12); }     // 16-byte aligned, never dereferenced

bool print_call(std::istringstream &in)
{
    int dtype, cus;
    long long clips, frames, window, Lq;
    std::string text;
    if (!(in >> dtype >> clips >> frames >> window >> Lq >> cus >> text)) return false;
    std::vector<int64_t> shapes;
    std::istringstream ss(text);
    std::string hw;
    long long S = 0;
    while (std::getline(ss, hw, ',')) {
        const size_t x = hw.find('x');
        if (x == std::string::npos) return false;
        shapes.push_back(atoll(hw.substr(0, x).c_str()));
        shapes.push_back(atoll(hw.substr(x + 1).c_str()));
        S += shapes[shapes.size() - 2] * shapes.back();
    }
    const long long L = (long long)shapes.size() / 2;
    if (L < 1 || clips < 1 || frames < 1 || window < 0 || Lq < 1 || clips * frames > 1 << 20 || S > 1 << 24 || Lq > 1 << 24) return false;
    Params p;
    memset(&p, 0, sizeof p);
    p.value = fake(1); p.shapes = static_cast<const int64_t *>(fake(2)); p.lsi = static_cast<const int64_t *>(fake(3));
    p.ftab = window > 0 ? static_cast<const int32_t *>(fake(4)) : nullptr;
    p.locA = fake(5); p.awA = fake(6);
    if (window > 0) { p.locB = fake(7); p.awB = fake(8); }
    p.groups = (int)(clips * frames); p.frames = (int)frames; p.window = (int)window;
    p.S = (int)S; p.M = 8; p.D = 32; p.L = (int)L; p.Lq = (int)Lq;
    p.LA = (int)L; p.PA = 4; p.LB = (int)(window * L); p.PB = window > 0 ? 4 : 1;
    p.shapes_host = shapes.data();
    p.v_clip = frames * S * p.M * p.D; p.v_head = p.D; p.v_pix = p.M * p.D;
    p.grad_out = fake(9); p.grad_value = fake(10); p.glocA = fake(11); p.gawA = fake(12);
    if (window > 0) { p.glocB = fake(13); p.gawB = fake(14); }
    const Knobs k = call_knobs(true, dtype, p);
    p.workspace = static_cast<unsigned *>(fake(15));
    if (k.bwd_cull != 0) {
        p.bbox = static_cast<int *>(fake(16));
        if (p.Lq >= 2048 && (long long)p.groups * p.M * (p.LA + p.LB) < 0x7fffffffLL) p.bsum = static_cast<int *>(fake(17));
    }
    p.gv_storage = storage_typed_grad_value_ok(dtype, p, env_knobs());
    p.own_levels = p.L; p.rec_mask = ~0u; p.own_pix = kOwnPix; p.dbg = k.dbg;
    const int esz = elem_bytes(dtype);
    p.cull_points = p.bbox && k.bwd_cull != 2 && owner_scatter_applicable(p, esz, k);
    if (!p.cull_points) p.bsum = nullptr;
    p.wide_stores = 1; p.wide_loads = 1;
    Shape s;
    if (k.force_generic || !fast_path_takes(dtype, p, k, true) || !shape_of(dtype, p, true, cus, s)) { printf("fast=0\n"); return true; }
    const ScatterPlan sc = plan_scatter(dtype, s, p, k, kGradAll);
    const GatherPlan g = plan_gather(s, p, k, kGradAll, sc.interval_records);
    printf("fast=1 footprint=%lld limit=%lld knob_walk=%d", s.footprint, kWalkDownBytes, k.walk);
    printf(" scatter=%d sc_l0=%d mfma_tiles=%d run_owner=%d run_mfma=%d own_pix=%d fused_zero=%d image_order=%d rec_mask=%u interval_records=%d",
           (int)sc.route, sc.l0, sc.mfma_tiles, (int)sc.run_owner, (int)sc.run_mfma, sc.own_pix, (int)sc.fused_zero, (int)sc.image_order,
           sc.rec_mask, (int)sc.interval_records);
    printf(" gather=%d g_parts=%d frame_split=%d g_grid=%u", (int)g.kind, g.parts, g.frame_split, g.grid);
    if (g.kind == GatherPlan::kWindow)
        printf(" win=%d,%d,%d,%d,%d,%d,%d,%d,%d", g.win.By, g.win.Bx, g.win.tiles_y, g.win.tiles_x, g.win.split, g.win.halo[0], g.win.halo[1], g.win.tpg, g.win.nt);
    printf(" walk=%s\n", g.walk_down ? "down" : "up");
    return true;
}

}  // namespace

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!print_call(in)) printf("error=bad-line\n");
    }
    return 0;
}
