// band_probe.cpp -- the band arithmetic of the owner-computes scatter (devis_amd/csrc/msda_params.h: own_slots, own_band_pixels,
// own_band_count, own_band_rows) and what the planner (msda_plan.hip) makes of it, as a stand-alone host program beside
// tests/plan_probe.cpp.  That probe takes grad_value in the type msda_grad_value_dtype names; this one takes Params::gv_storage
// as an input, so that the four-slot instantiations (a 16-bit type with float grad_value) are reached as well.
// One backward call of the fused temporal op per line of stdin:
//   DTYPE GV_STORAGE CLIPS FRAMES WINDOW LQ HxW,HxW,...
// and one line of `name=value` fields per call: slots, pix (the most the instantiation takes), per level the band count (0 = "direct") and the bands' row ranges as
// the device forms them at that size, and the planner's own_pix (its choice for the call) / rec_mask / fused_zero / image_order /
// own levels.
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

static void *fake(uintptr_t n) { return reinterpret_cast<void *>(n << 12); }

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int dtype, gv, clips, frames, window, Lq;
        std::string text;
        if (!(in >> dtype >> gv >> clips >> frames >> window >> Lq >> text)) { printf("error=bad-line\n"); continue; }
        std::vector<int64_t> shapes;
        std::istringstream ss(text);
        std::string hw;
        long long S = 0;
        while (std::getline(ss, hw, ',')) {
            const size_t x = hw.find('x');
            if (x == std::string::npos) break;
            shapes.push_back(atoll(hw.substr(0, x).c_str()));
            shapes.push_back(atoll(hw.substr(x + 1).c_str()));
            S += shapes[shapes.size() - 2] * shapes.back();
        }
        const int L = (int)shapes.size() / 2;
        if (L < 1 || S <= 0) { printf("error=bad-shapes\n"); continue; }
        Params p;
        memset(&p, 0, sizeof p);
        p.value = fake(1); p.shapes = static_cast<const int64_t *>(fake(2)); p.lsi = static_cast<const int64_t *>(fake(3));
        p.ftab = window > 0 ? static_cast<const int32_t *>(fake(4)) : nullptr;
        p.locA = fake(5); p.awA = fake(6);
        if (window > 0) { p.locB = fake(7); p.awB = fake(8); }
        p.groups = clips * frames; p.frames = frames; p.window = window;
        p.S = (int)S; p.M = 8; p.D = 32; p.L = L; p.Lq = Lq;
        p.LA = L; p.PA = 4; p.LB = window * L; p.PB = window > 0 ? 4 : 1;
        p.shapes_host = shapes.data();
        p.v_clip = (int64_t)frames * S * p.M * p.D; p.v_head = p.D; p.v_pix = p.M * p.D;
        p.grad_out = fake(9); p.grad_value = fake(10); p.glocA = fake(11); p.gawA = fake(12);
        if (window > 0) { p.glocB = fake(13); p.gawB = fake(14); }
        const Knobs k = call_knobs(true, dtype, p);
        p.workspace = static_cast<unsigned *>(fake(15));
        p.bbox = static_cast<int *>(fake(16));
        p.gv_storage = gv;
        p.own_levels = L; p.rec_mask = ~0u;
        const int esz = elem_bytes(dtype);
        p.cull_points = owner_scatter_applicable(p, esz, k);
        p.wide_stores = 1; p.wide_loads = 1;

        const int pix = own_band_pixels(dtype, gv != 0);
        printf("slots=%d pix=%d gv_ok=%d bands=", own_slots(dtype, gv != 0), pix, (int)storage_typed_grad_value_ok(dtype, p, env_knobs()));
        std::string rows;
        for (int l = 0; l < L; ++l) {
            // as msda_bwd_value_grp_kernel's prologue and item loop form them: 32-bit, q = H / nb, rem = H % nb
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
            const int nb = own_band_count(H, W, pix);
            printf("%s%d", l ? "," : "", nb);
            // ... and as the planner counts them, in 64 bits: the two must agree
            if ((long long)nb != own_band_count<long long>(shapes[2 * l], shapes[2 * l + 1], pix)) { printf(" error=host-device-mismatch"); }
            if (l) rows += "|";
            for (int b = 0; b < nb; ++b) {
                int r0 = 0, r1 = 0;
                own_band_rows(H / nb, H % nb, b, r0, r1);
                rows += (b ? ";" : "") + std::to_string(r0) + "-" + std::to_string(r1);
            }
            if (nb == 0) rows += "direct";
        }
        printf(" rows=%s", rows.c_str());
        Shape s;
        if (!fast_path_takes(dtype, p, k, true) || !shape_of(dtype, p, true, 256, s)) { printf(" error=no-fast-path\n"); continue; }
        const ScatterPlan sc = plan_scatter(dtype, s, p, k, kGradAll);
        printf(" owner=%d sc_l0=%d own_pix=%d rec_mask=%u fused_zero=%d image_order=%d\n", (int)(sc.route == ScatterPlan::kOwner), sc.l0,
               sc.own_pix, sc.rec_mask, (int)sc.fused_zero, (int)sc.image_order);
    }
    return 0;
}
