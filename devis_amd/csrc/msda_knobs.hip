// msda_knobs.hip -- host only, no HIP: reads the knobs from the environment and keeps the pinned routes (msda_knobs.h).
#include "msda_knobs.h"
#include <algorithm>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace msda {

namespace {
Knobs g_knobs;
int g_knobs_loaded = 0;
std::mutex g_routes_mutex;
std::vector<RoutePin> g_routes;
int g_routes_n = 0;                     // (read without the lock on the launch path: 0 = nothing pinned, skip the key)
}  // namespace

int knob_value(Parse parse, const char *text)
{
    const int v = atoi(text);
    switch (parse) {
        case Parse::IsOne: return v == 1;
        case Parse::IsAtomic: return strcmp(text, "atomic") == 0;
        case Parse::DbgBits: return v & ~kSdbgOrderMask;
        case Parse::OrderBits: return (v & kSdbgLevelOrder) ? 1 : (v & kSdbgImageOrder) ? 2 : 0;
        default: return v;
    }
}

void load_knobs()
{
    Knobs k;
    const char *hooks = getenv("MSDA_ENABLE_HOOKS");
    if (hooks && atoi(hooks) == 1)
        for (int i = 0; i < kNumKnobs; ++i) {
            const char *e = getenv(kKnobs[i].env);
            if (!e || !e[0]) continue;
            k.*kKnobs[i].field = knob_value(kKnobs[i].parse, e);
            k.forced |= 1u << i;
        }
    g_knobs = k;
    __atomic_store_n(&g_knobs_loaded, 1, __ATOMIC_RELEASE);
}

// The knobs of the environment, without any pin.
const Knobs &env_knobs()
{
    if (!__atomic_load_n(&g_knobs_loaded, __ATOMIC_ACQUIRE)) load_knobs();      // benign race: every thread reads the same environment
    return g_knobs;
}

int route_key(char *buf, int len, bool bwd, int dtype, const Params &p)
{
    if (!p.shapes_host || p.L > 16) return -1;
    int n = snprintf(buf, len, "%c|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|%d|", bwd ? 'b' : 'f', dtype, p.groups / (p.frames > 0 ? p.frames : 1),
                     p.frames, p.window, p.S, p.M, p.D, p.L, p.Lq, p.PA, p.PB);
    for (int l = 0; l < p.L && n > 0 && n < len; ++l)
        n += snprintf(buf + n, len - n, "%s%lldx%lld", l ? "," : "", (long long)p.shapes_host[2 * l], (long long)p.shapes_host[2 * l + 1]);
    return (n > 0 && n < len) ? n : -1;
}

bool parse_route_settings(const char *text, RoutePin &pin)
{
    std::fill(pin.value, pin.value + kNumKnobs, kNotPinned);
    std::string t(text ? text : "");
    size_t i = 0;
    while (i < t.size()) {
        while (i < t.size() && (t[i] == ' ' || t[i] == ',')) ++i;
        if (i >= t.size()) break;
        const size_t eq = t.find('=', i);
        if (eq == std::string::npos) return false;
        size_t end = t.find_first_of(" ,", eq);
        if (end == std::string::npos) end = t.size();
        const std::string name = t.substr(i, eq - i);
        int row = 0;
        while (row < kNumKnobs && !(kKnobs[row].pin && name == kKnobs[row].pin)) ++row;
        if (row == kNumKnobs) return false;
        pin.value[row] = atoi(t.substr(eq + 1, end - eq - 1).c_str());
        i = end;
    }
    return true;
}

// The knobs of one entry-point call: the pinned settings of its shape (if any) laid over the environment's.
Knobs call_knobs(bool bwd, int dtype, const Params &p)
{
    Knobs k = env_knobs();
    if (__atomic_load_n(&g_routes_n, __ATOMIC_ACQUIRE) == 0) return k;
    char key[512];
    if (route_key(key, (int)sizeof key, bwd, dtype, p) < 0) return k;
    std::lock_guard<std::mutex> lock(g_routes_mutex);
    for (const RoutePin &r : g_routes) {
        if (r.key != key) continue;
        for (int i = 0; i < kNumKnobs; ++i)
            if (r.value[i] != kNotPinned && !(k.forced & (1u << i))) k.*kKnobs[i].field = r.value[i];
        break;
    }
    return k;
}

bool pin_route(const char *key, const char *settings)
{
    RoutePin pin;
    pin.key = key;
    if (!parse_route_settings(settings, pin)) return false;
    const bool remove = !settings || !settings[0];
    std::lock_guard<std::mutex> lock(g_routes_mutex);
    for (size_t i = 0; i < g_routes.size(); ++i)
        if (g_routes[i].key == pin.key) {
            if (remove) g_routes.erase(g_routes.begin() + (long)i); else g_routes[i] = pin;
            __atomic_store_n(&g_routes_n, (int)g_routes.size(), __ATOMIC_RELEASE);
            return true;
        }
    if (!remove) g_routes.push_back(pin);
    __atomic_store_n(&g_routes_n, (int)g_routes.size(), __ATOMIC_RELEASE);
    return true;
}

void clear_routes()
{
    std::lock_guard<std::mutex> lock(g_routes_mutex);
    g_routes.clear();
    __atomic_store_n(&g_routes_n, 0, __ATOMIC_RELEASE);
}

int route_count() { return __atomic_load_n(&g_routes_n, __ATOMIC_ACQUIRE); }

}  // namespace msda
