// Process-global timing hooks for bench.py (HIP events on the launch streams), serialised by a mutex.
// Nothing on the data path reads them.
#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

#include "sf_prof.h"

static struct {
    int on = 0;
    std::vector<ProfSpan> spans;
    std::vector<hipEvent_t> pool;
    double gemm_flops = 0.0;
    long gemm_launches = 0;
    long calls = 0;
    hipEvent_t ref = nullptr;  // common time origin for merging overlapping launch intervals
} g_prof;
static std::mutex g_prof_mu;

static hipEvent_t prof_event() {
    hipEvent_t e;
    if (!g_prof.pool.empty()) {
        e = g_prof.pool.back();
        g_prof.pool.pop_back();
    } else {
        (void)hipEventCreate(&e);
    }
    return e;
}
ProfScope::ProfScope(hipStream_t st, int stage) : s(st), live(g_prof.on != 0) {
    if (!live) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    sp.stage = stage;
    sp.a = prof_event();
    sp.b = prof_event();
    (void)hipEventRecord(sp.a, s);
}
ProfScope::~ProfScope() {
    if (!live) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    (void)hipEventRecord(sp.b, s);
    g_prof.spans.push_back(sp);
}
// called from sf_chol.hip around every k_gemm_nt launch
void sf_prof_gemm_begin(hipStream_t s, double flops, void** tok) {
    *tok = nullptr;
    if (!g_prof.on) return;
    ProfScope* p = new ProfScope(s, PS_GEMM);
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof.gemm_flops += flops;
        g_prof.gemm_launches += 1;
    }
    *tok = p;
}
void sf_prof_gemm_end(void* tok) {
    if (tok) delete (ProfScope*)tok;
}

void prof_count_call() {
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.calls += 1;
}

extern "C" int sf_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.on = on;
    if (on) {
        if (!g_prof.ref) SF_HIP(hipEventCreate(&g_prof.ref));
        SF_HIP(hipEventRecord(g_prof.ref, 0));
    }
    return SF_OK;
}
extern "C" int sf_profile_read(double* ms_by_stage, double* gemm_flops, long* gemm_launches, long* calls) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    double acc[PS_COUNT + 1] = {0, 0, 0, 0, 0, 0};
    std::vector<std::pair<double, double>> gemm_iv;  // [start, end) of every MFMA launch, ms since ref
    for (auto& sp : g_prof.spans) {
        float ms = 0.f;
        SF_HIP(hipEventSynchronize(sp.b));
        SF_HIP(hipEventElapsedTime(&ms, sp.a, sp.b));
        acc[sp.stage] += ms;
        if (sp.stage == PS_GEMM && g_prof.ref) {
            float ta = 0.f;
            if (hipEventElapsedTime(&ta, g_prof.ref, sp.a) == hipSuccess) gemm_iv.emplace_back(ta, ta + ms);
        }
        g_prof.pool.push_back(sp.a);
        g_prof.pool.push_back(sp.b);
    }
    g_prof.spans.clear();
    // launches on the two streams of the Cholesky overlap: merge the intervals so that concurrent
    // launches are not counted twice (slot 2 = union, slot 5 = plain sum of launch durations)
    acc[PS_COUNT] = acc[PS_GEMM];
    if (!gemm_iv.empty()) {
        std::sort(gemm_iv.begin(), gemm_iv.end());
        double uni = 0.0, lo = gemm_iv[0].first, hi = gemm_iv[0].second;
        for (size_t i = 1; i < gemm_iv.size(); ++i) {
            if (gemm_iv[i].first <= hi) {
                if (gemm_iv[i].second > hi) hi = gemm_iv[i].second;
            } else {
                uni += hi - lo;
                lo = gemm_iv[i].first;
                hi = gemm_iv[i].second;
            }
        }
        uni += hi - lo;
        acc[PS_GEMM] = uni;
    }
    if (ms_by_stage)
        for (int i = 0; i < PS_COUNT + 1; ++i) ms_by_stage[i] = acc[i];
    if (gemm_flops) *gemm_flops = g_prof.gemm_flops;
    if (gemm_launches) *gemm_launches = g_prof.gemm_launches;
    if (calls) *calls = g_prof.calls;
    g_prof.gemm_flops = 0.0;
    g_prof.gemm_launches = 0;
    g_prof.calls = 0;
    return SF_OK;
}
