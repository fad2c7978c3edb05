// Dependencies between the workgroups of one launch: counters, bounded waits, the stall watch, the abort record and the
// rescue of unclaimed chain tasks.  Used by the persistent kernel k_potrf_dataflow (and by the panel body's in-task waits).
#pragma once
#include "sf_common.h"

// ---- dataflow sequence (k_potrf_dataflow): dependencies between workgroups of ONE launch ------------------------
// A producer finishes its global stores, __syncthreads(), then ONE lane: agent-scope release (write-back of the XCD's L2),
// s_waitcnt by hand (the compiler may drop its own when the wave's scoreboard is provably empty), relaxed agent-scope
// store / add on a monotone counter.  A consumer: ONE lane polls the counter with relaxed agent-scope loads (L2-served,
// s_sleep between polls), then ONE agent-scope acquire (invalidates this CU's L1), __syncthreads(), plain loads.
// Every wait is bounded: after SF_DF_TIMEOUT_TICKS of the 100 MHz wall clock the waiter raises the launch's abort flag,
// which every other wait and the task dispenser observe.
#define SF_DF_TIMEOUT_TICKS 400000000LL  // 4 s
// ... and the launch is also aborted when NO task of the launch has completed for SF_DF_STALL_TICKS while a workgroup was
// waiting (round 6): every task end bumps a progress counter (abort_flag[5]); the longest task of the largest matrix the tables
// hold (N = 16384: one slab's 1024 K slabs) runs ~5 ms, so 25 ms without a single completion chip-wide means the workgroups
// that hold the claimed tasks are not running -- a device shared with other processes (profiles/r05_g_shared_gpu_abort.txt: the
// stall begins mid-launch, an arrival gate at the head of the kernel would not see it).  The caller's fall-back then costs
// ~25 ms + one factorisation on the launch sequences instead of 4 s.  abort_flag[6] counts the workgroups that started (a
// diagnostic: grid not co-resident), abort_flag[7] != 0 replaces the bound (units of 2^16 ticks; tuning builds).
#define SF_DF_STALL_TICKS 2500000LL  // 25 ms
#define SF_DF_ABORT_TIMEOUT 1
#define SF_DF_ABORT_STALL 2
__device__ __forceinline__ int sf_df_load(const int* flag) {
    return __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the waiter that raises the abort flag leaves what it was waiting for behind it: abort_flag[1..] = {counter (offset from the abort
// flag, in ints), target, value} of the first counter that had not arrived (tuning builds print it)
// (abort_flag[8..9]: address of the process's abort record in host memory, sf_df_diag -- what the caller's warning quotes:
// {aborted launches, reason, workgroups that had started, grid, ticks the reporting wait had lasted, tasks completed})
__device__ __forceinline__ void sf_df_report(int* abort_flag, const int* f, int target, int reason = SF_DF_ABORT_TIMEOUT,
                                             long long waited = 0) {
    if (__hip_atomic_exchange(abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        if (f) {
            abort_flag[1] = (int)(f - abort_flag);
            abort_flag[2] = target;
            abort_flag[3] = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        long long* diag = (long long*)__hip_atomic_load((long long*)(abort_flag + 8), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (diag) {
            diag[1] = reason;
            diag[2] = sf_df_load(abort_flag + 6);
            diag[3] = gridDim.x;
            diag[4] = waited;
            diag[5] = sf_df_load(abort_flag + 5);
            __hip_atomic_fetch_add(diag, 1LL, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
__device__ __forceinline__ long long sf_df_stall_ticks(const int* abort_flag) {
    const int o = abort_flag[7];
    return o ? (long long)o << 16 : SF_DF_STALL_TICKS;
}
// Waits until *f1 >= t1 and *f2 >= t2 and *f3 >= t3 (NULL flags are skipped), then ONE acquire for all of them.  `probe`
// (optional) is only looked at, before the acquire: *probe_ok tells whether it had reached its target -- the data it guards
// is then covered by this acquire and needs no wait of its own later.  Returns false when the launch is being aborted.
// (s_okp: one int of LDS -- the kernels keep their LDS image at offset 0 of the workgroup's allocation, so no static __shared__
// variable may exist beside the dynamic buffer: with sm at offset 16 the direct-to-LDS operand loads lose their alignment)
// `rescue` (queued tasks' waits BEFORE their bodies only): a callable that looks for a ready chain / front task nobody has
// claimed and claims it; after SF_DF_RESCUE_TICKS inside one wait the polling lane calls it every ~50 us.  When it returns
// true the wait ends with SF_DF_DEFERRED: the workgroup sets its task aside, runs the chain task it has just claimed and
// comes back (k_potrf_dataflow).  This is what makes the schedule live BY CONSTRUCTION: chain and front tasks are claimed by
// whoever finds them ready at the dispenser, and a claim can be missed (see there); a workgroup that waits before a body
// holds nothing but its task number, and in-body waits only ever depend on tasks that are already running.  The normal path
// never gets here: waits that long mean the chip is starved of chain progress anyway.
#define SF_DF_RESCUE_TICKS 50000LL  // 500 us of the 100 MHz wall clock
#define SF_DF_DEFERRED 4
struct sf_df_no_rescue {
    __device__ __forceinline__ bool operator()() const { return false; }
};
// The rare part of a wait (every 32nd poll), out of line: the waits are inlined at a dozen sites of a kernel whose task loop is
// 100 KB of code -- with the abort record and the stall bound inlined as well every site grew, and launches of 32-64 matrices
// ran 1.2 % slower (same-box A/B, both orders: profiles/r06_b_dataflow_wait_code_size_ab.txt).
// Returns 0: keep polling; 1: give up (the launch is being aborted, by somebody else or by this call); 2: keep polling, and
// the wait has lasted long enough for the caller to look for an unclaimed chain task (SF_DF_RESCUE_TICKS).
struct sf_df_watch {
    long long t0, tp;  // start of the wait; when the launch's progress counter last moved, as seen from this wait
    int pg0;
};
__device__ __attribute__((noinline)) int sf_df_wait_slow(sf_df_watch& w, int* abort_flag, const int* f1, int t1, const int* f2, int t2,
                                                         const int* f3, int t3, const bool look_at_progress) {
    if (sf_df_load(abort_flag) != 0) return 1;
    const long long now = wall_clock64();
    const long long waited = now - w.t0;
    int reason = 0;
    if (look_at_progress) {  // (every ~0.3 ms: one more L2 round trip in the polling loop)
        const int pg = sf_df_load(abort_flag + 5);
        if (pg != w.pg0) {
            w.pg0 = pg;
            w.tp = now;
        } else if (now - w.tp > sf_df_stall_ticks(abort_flag)) {  // nothing completes any more: see SF_DF_STALL_TICKS
            reason = SF_DF_ABORT_STALL;
        }
    }
    // (abort_flag[4]: the bound in units of 2^20 ticks when the host asked for another one -- tuning builds)
    if (!reason && waited > SF_DF_TIMEOUT_TICKS && (abort_flag[4] == 0 || (waited >> 20) > abort_flag[4])) reason = SF_DF_ABORT_TIMEOUT;
    if (reason) {
        const bool m1 = f1 && sf_df_load(f1) < t1, m2 = f2 && sf_df_load(f2) < t2;
        sf_df_report(abort_flag, m1 ? f1 : (m2 ? f2 : f3), m1 ? t1 : (m2 ? t2 : t3), reason, waited);
        return 1;
    }
    return waited > SF_DF_RESCUE_TICKS ? 2 : 0;
}
template <class RESCUE>
__device__ __forceinline__ int sf_df_wait_r(const int* f1, int t1, const int* f2, int t2, const int* f3, int t3,
                                            const int* probe, int tprobe, bool* probe_ok, int* abort_flag, const int tid,
                                            int* s_okp, RESCUE&& rescue, const bool can_rescue) {
    if (tid == 0) {
        int ok = 1;
        // (short-circuit on purpose: a poller asks for the first counter that is missing only -- polls of all three, every
        // time, from a few hundred waiting workgroups slowed the launch by 2 %)
        auto ready = [&]() {
            return (!f1 || sf_df_load(f1) >= t1) && (!f2 || sf_df_load(f2) >= t2) && (!f3 || sf_df_load(f3) >= t3);
        };
        if (!ready()) {
            sf_df_watch w;
            w.t0 = w.tp = wall_clock64();
            w.pg0 = sf_df_load(abort_flag + 5);
            unsigned it = 0;
            for (;;) {
                __builtin_amdgcn_s_sleep(4);
                if (ready()) break;
                if ((++it & 31) == 0) {
                    const int r = sf_df_wait_slow(w, abort_flag, f1, t1, f2, t2, f3, t3, (it & 255) == 0);
                    if (r == 1) {
                        ok = 0;
                        break;
                    }
                    if (r == 2 && can_rescue && rescue()) {
                        ok = SF_DF_DEFERRED;
                        break;
                    }
                }
            }
        }
        if (probe && sf_df_load(probe) >= tprobe) ok |= 2;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        *s_okp = ok;
    }
    __syncthreads();
    const int ok = __builtin_amdgcn_readfirstlane(*s_okp);
    __syncthreads();  // (s_ok is rewritten by the next wait)
    if (probe_ok) *probe_ok = (ok & 2) != 0;
    return ok & (1 | SF_DF_DEFERRED);
}
__device__ __forceinline__ bool sf_df_wait(const int* f1, int t1, const int* f2, int t2, const int* f3, int t3,
                                           const int* probe, int tprobe, bool* probe_ok, int* abort_flag, const int tid,
                                           int* s_okp) {
    return sf_df_wait_r(f1, t1, f2, t2, f3, t3, probe, tprobe, probe_ok, abort_flag, tid, s_okp, sf_df_no_rescue(), false) == 1;
}
__device__ __forceinline__ bool sf_df_wait(const int* flag, int target, int* abort_flag, const int tid, int* s_okp) {
    return sf_df_wait(flag, target, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, abort_flag, tid, s_okp);
}
// call after __syncthreads(): every wave's stores have been issued and waited for
__device__ __forceinline__ void sf_df_release() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void sf_df_set(int* flag, int value) {
    __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sf_df_add(int* flag, int value) {
    __hip_atomic_fetch_add(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
