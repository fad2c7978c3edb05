// Process-global timing hooks for bench.py (HIP events on the launch streams), serialised by a mutex (internal).
// Nothing on the data path reads them.
#pragma once
#include "sf_common.h"

enum { PS_TRANSFORM = 0, PS_FILL, PS_GEMM, PS_POTRF, PS_SOLVE, PS_COUNT };
struct ProfSpan {
    hipEvent_t a, b;
    int stage;
};
// the launches enqueued on `st` during the scope's life count as one span of `stage` (nothing happens while profiling is off)
struct ProfScope {
    hipStream_t s;
    ProfSpan sp;
    bool live;
    ProfScope(hipStream_t st, int stage);
    ~ProfScope();
};
#pragma GCC visibility push(hidden)
void prof_count_call();  // one likelihood / covariance call
#pragma GCC visibility pop
