// sf_exec: the streams and the event pool a launch sequence needs besides the caller's stream (sf_common.h).
#include <cstdlib>

#include "sf_common.h"

int sf_exec_prepare(sf_exec* ex) {
    int dev = 0;
    SF_HIP(hipGetDevice(&dev));
    if (ex->side == nullptr || ex->device != dev) {
        if (ex->side) sf_exec_release(ex);
        // highest priority: the small launches of the diagonal-block chain must win freed CU slots against
        // the thousands of pending MFMA workgroups of the caller's stream, otherwise the chain starves
        int prio_lo = 0, prio_hi = 0;
        SF_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        SF_HIP(hipStreamCreateWithPriority(&ex->side, hipStreamNonBlocking, prio_hi));
        // (high priority too: in a multi-order call the next chunk's transform chains and fills -- dozens of small launches
        // per order -- run on it beside the factorisation, whose workgroups take a CU's whole register file; at normal
        // priority they only got CUs when a big launch drained: 16 of the 21 orders of cfg 3's second chunk were filled
        // AFTER the first chunk's factorisation, 16.7 ms of a 276 ms step with nothing else running)
        SF_HIP(hipStreamCreateWithPriority(&ex->aux, hipStreamNonBlocking, prio_hi));
        for (int g = 0; g < SF_EXEC_GROUPS - 1; ++g) SF_HIP(hipStreamCreateWithFlags(&ex->grp[g], hipStreamNonBlocking));
        SF_HIP(hipEventCreateWithFlags(&ex->fork, hipEventDisableTiming));
        SF_HIP(hipEventCreateWithFlags(&ex->join, hipEventDisableTiming));
        ex->device = dev;
    }
    ex->used = 0;
    return SF_OK;
}
int sf_exec_event(sf_exec* ex, hipEvent_t* e) {
    if (ex->used == ex->pool_size) {
        if (ex->pool_size == ex->pool_cap) {
            const size_t cap = ex->pool_cap ? 2 * ex->pool_cap : 256;
            hipEvent_t* np = (hipEvent_t*)realloc(ex->pool, cap * sizeof(hipEvent_t));
            if (!np) {
                sf_set_error("out of host memory (event pool)");
                return SF_ENOMEM;
            }
            ex->pool = np;
            ex->pool_cap = cap;
        }
        hipEvent_t ne;
        SF_HIP(hipEventCreateWithFlags(&ne, hipEventDisableTiming));
        ex->pool[ex->pool_size++] = ne;
    }
    *e = ex->pool[ex->used++];
    return SF_OK;
}
void sf_exec_release(sf_exec* ex) {
    if (!ex) return;
    for (size_t i = 0; i < ex->pool_size; ++i) (void)hipEventDestroy(ex->pool[i]);
    free(ex->pool);
    ex->pool = nullptr;
    ex->pool_size = ex->pool_cap = ex->used = 0;
    if (ex->fork) (void)hipEventDestroy(ex->fork);
    if (ex->join) (void)hipEventDestroy(ex->join);
    if (ex->side) (void)hipStreamDestroy(ex->side);
    if (ex->aux) (void)hipStreamDestroy(ex->aux);
    for (int g = 0; g < SF_EXEC_GROUPS - 1; ++g) {
        if (ex->grp[g]) (void)hipStreamDestroy(ex->grp[g]);
        ex->grp[g] = nullptr;
    }
    ex->fork = ex->join = nullptr;
    ex->side = ex->aux = nullptr;
    ex->device = -1;
}
// context-free entry points (sf_potrf_batch, ...): one sf_exec per calling thread and device
sf_exec* sf_exec_thread_local(void) {
    static thread_local sf_exec per_device[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    return &per_device[(dev >= 0 && dev < 64) ? dev : 0];
}
