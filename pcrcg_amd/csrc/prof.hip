// prof.hip -- optional HIP-event timing of single launches (bench.py roofline): KpProfScope (common.h), which kpconv.hip,
// gemm_x6.hip and radius.hip put around the kernels they time, and the two C entries that switch it on and read it back.
#include <mutex>
#include <vector>

#include "common.h"

namespace pcrcg {

struct ProfRec { hipEvent_t a, b; int nq, h, cin, cout, kind; };
static int g_prof_on = 0;         // bit 0: KPConv kernels (kinds 0-2), bit 1: the GEMM family (kind 3)
static std::vector<ProfRec> g_prof;
static std::mutex g_prof_mu;   // forwards may be enqueued from several host threads

KpProfScope::KpProfScope(hipStream_t s, int nq_, int h_, int cin_, int cout_, int kind_)
    : st(s), a(nullptr), b(nullptr), nq(nq_), h(h_), cin(cin_), cout(cout_), kind(kind_),
      on((g_prof_on & (kind_ == 3 ? 2 : kind_ == 4 ? 4 : 1)) != 0) {
    if (!on) return;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
}
KpProfScope::~KpProfScope() {
    if (!on) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof.push_back({a, b, nq, h, cin, cout, kind});
}

}  // namespace pcrcg

using namespace pcrcg;

extern "C" {

void pcrcg_profile_kpconv(int enable) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    for (auto& r : g_prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof.clear();
    g_prof_on = enable;
}

int pcrcg_profile_kpconv_read(float* ms, int* nq, int* h, int* cin, int* cout, int* kind, int cap) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    int n = 0;
    for (auto& r : g_prof) {
        if (n >= cap) break;
        if (hipEventSynchronize(r.b) != hipSuccess) return -1;
        float t = 0.f;
        if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) return -1;
        ms[n] = t; nq[n] = r.nq; h[n] = r.h; cin[n] = r.cin; cout[n] = r.cout; kind[n] = r.kind;
        ++n;
    }
    return n;
}
}
