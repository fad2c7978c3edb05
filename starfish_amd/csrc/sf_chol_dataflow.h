// The dataflow sequence: the task tables, the dispenser and the persistent kernel k_potrf_dataflow (the bodies of the panel
// step and of the diagonal tile as tasks ordered by counters), then its host side: the counter layout, the abort record, the
// enable flag, what fits, and the launcher sf_launch_potrf_v4.  Used by sf_launch_potrf and the recovery calls of the ABI.
#pragma once
#include "sf_chol_host.h"
#include "sf_chol_diag.h"
#include "sf_chol_sync.h"
#include "sf_chol_panel.h"

// =====================================================================================================================
// DATAFLOW sequence (round 4): the whole factorisation of a batch as ONE persistent launch.
//
// The launch sequences above are bound by their panel boundaries once the batch no longer fills the chip many times over
// (cfg 2 split over 2 / 4 / 8 GPUs: 64 / 32 / 16 matrices): the chain D(k) -> top(k) -> D(k+1) waits for workgroup slots
// behind bulk workgroups that start and end together, the bulk launches wait for the chain's events, every launch fills
// and drains the chip on its own (timelines in profiles/r04_*: the three streams 85-90 % busy, the matrix cores 0.49-0.74).
// Here 512 workgroups (two per CU) stay resident and draw TASKS; a task waits for exactly the tasks whose results it reads
// (monotone counters in global memory, agent scope) -- nothing else orders the work.  Per panel k and matrix b:
//   C(b,k)      chain task: the step of slab k for panel k-1 -- the partial sums FP(b,k-1,1,.) added in split order, then the K
//               tail over the last 128 columns, solve, L in place, tile (k,k) parked -- and the diagonal tile D(b,k) right
//               behind it in the SAME workgroup.  The K work needs the FIRST half of the previous chain task (row k-1
//               final), only the solve its second half (D(b,k-1)): it runs beside that diagonal tile, in another workgroup.
//               Chain tasks are not queued: whichever workgroup finds one READY at the dispenser claims it (compare-and-swap
//               on the matrix's chain counter) -- in a queue it waited until a workgroup had worked its way to it.
//   FP(b,k,d,s) partial sums of the FRONT slabs k+d, d = 1..3, for panel k over the columns LEFT of panel k-1: they depend on
//               tasks two stages back, so they run long before row k is final
//   FR(b,k,d)   d = 2, 3: partial sums added + K tail + solve + L in place + own diagonal tile for slab k+d.  With the front
//               three slabs wide the rows the chain needs next are one reduce-and-epilogue behind it (~150 us), not one
//               long-K task: a lead slab as an ordinary task held the chain of 16 matrices at ~400 us per panel
//   R(b,i,k)    the fused panel step of the slabs i >= k+4 (MODE 0: the K loop starts as soon as row k is final, only the
//               triangular solve waits for D(b,k)), or, while a stage has fewer tasks than its XCD has workgroup slots,
//               RP(b,i,k,s) partial sums + RR(b,i,k) reduce + epilogue
// Queued tasks are drawn in an order in which every dependency precedes its dependants (stage k: FP(.,k+1,.,.), FR(.,k,.),
// R / RP(.,.,k), RR(.,.,k)); a workgroup holds at most one task, only claimed tasks are waited for, a chain task is claimed
// only when its K work can start: the schedule cannot deadlock whatever the residency or placement of the workgroups.  The
// inverse tiles W_k of ALL panels are kept (one per panel, in the scratch the unfused sequence uses for its panel): no
// buffer of the chain is ever recycled.  Same arithmetic as the fused sequence (the same kernels' bodies); the summation
// order differs where the split differs.
struct sf_df_stage {
    int off;      // first task of the stage's segment
    int St;       // split of FP(., k+1, ., .): 0 = the front tasks of panel k+1 run their whole K loops themselves
    int Sr;       // split of the ordinary rest tasks (1 = unsplit MODE 0)
    int thr_pt;   // FP(b, k+1, d, .) arrivals the front task of (b, k+1, d) waits for (cumulative over the panels of that parity)
    int thr_rp;   // RP(b, i, k, .) arrivals RR(b, i, k) waits for (cumulative)
    int dep;      // RP of this stage re-uses the partial-sum region of stage `dep` (same parity, split): wait for its reduces
    int fw;       // front width of this panel (slabs k+1 .. k+F are front slabs) | front slabs of panel k+1 that exist << 8
};
// ... and as it travels in the kernel arguments (12 bytes: two tables of 128 stages stay below the 4 KB of a kernel's arguments;
// N = 16384 has 127 stages)
struct sf_df_stage_packed {
    int off;
    unsigned short thr_pt, thr_rp, fw;
    unsigned char split;  // St | Sr << 4
    signed char dep;
};
static_assert(sizeof(sf_df_stage_packed) == 12, "sf_df_stage_packed");
template <class S>
__host__ __device__ __forceinline__ sf_df_stage sf_df_stage_of(S& x) {  // (copy out of the constant address space)
    sf_df_stage r;
    r.off = x.off;
    const int sp = x.split;
    r.St = sp & 15;
    r.Sr = sp >> 4;
    r.thr_pt = x.thr_pt;
    r.thr_rp = x.thr_rp;
    r.dep = x.dep;
    r.fw = x.fw;
    return r;
}
static inline sf_df_stage_packed sf_df_pack(const sf_df_stage& x) {
    sf_df_stage_packed r;
    r.off = x.off;
    r.thr_pt = (unsigned short)x.thr_pt;
    r.thr_rp = (unsigned short)x.thr_rp;
    r.fw = (unsigned short)x.fw;
    r.split = (unsigned char)(x.St | (x.Sr << 4));
    r.dep = (signed char)x.dep;
    return r;
}
// One task queue per XCD: matrix b belongs to queue b % 8 (its slabs share the B operand L[panel rows, :k0] through that
// XCD's L2 -- with ONE queue for the chip the operand was fetched by every XCD: L2 hit rate 0.14 instead of 0.38, 1.5 x the
// HBM reads); a workgroup serves the queue of the XCD it runs on and, once that is exhausted, the others in turn.  Queues
// with the same number of matrices share a task table (at most two sizes).
#define SF_DF_QUEUES 8
#define SF_DF_MAX_STAGES 127  // (two tables of 12-byte entries in the kernel arguments: < 4 KB; N = 16384 = 128 panels)
#define SF_DF_FRONT_MAX 6    // slabs k+1 .. k+front of panel k are front slabs (the tables hold fronts up to 6 wide)
#define SF_DF_FRONT_WIDEST 3 // ... and the widest front chosen (by batch size and panel): the stride of the front's partial sums and counters
#define SF_DF_QTILES (2 * SF_CHIP_WGS / SF_DF_QUEUES)  // partial-sum tiles per queue and stage parity
struct sf_df_args {
    sf_panel_args p;  // matrix, right-hand side, generator, frame: the per-task fields are filled in by the kernel
    int nt, batch, front;  // front: the LARGEST front width (the width of panel k is st[.][k].fw & 255: it grows towards the end)
    int fstart[SF_DF_FRONT_MAX];        // first panel whose front is d slabs wide (index d - 1): chain_next[.][d - 1] counts from there
    int thr_base[2][2][SF_DF_FRONT_MAX];  // [table][panel parity][d - 1]: partial-sum arrivals of that parity before distance d existed
    int fp_pos;       // position of the front partial sums inside a stage's segment, in 1/256 of its rest tasks
    int bq[2], ntasks[2];  // table v serves the queues with bq[v] matrices
    int pt_cap;       // largest split of the front partial sums: a (matrix, front slab) owns pt_cap tiles per panel parity in region 2
    int *head, *abort_flag, *done_top, *done_D, *done_row, *row_L, *fp_cnt, *rp_cnt, *stage_done;
    int* chain_next;  // [batch][3]: the next chain task (d = 1) / front task (d = 2, 3) of every matrix (claimed by compare-and-swap once ready)
    double* T;        // per matrix: parked diagonal tile [GT x SF_LDT], then W_k for every panel
    int64_t sT;
    double* part;     // three regions of sf_split_region_tiles() tiles: rest partial sums by stage parity, front partial sums
    int* info;
    int qbal;         // 1: with fewer matrices than queues the XCDs are dealt to the non-empty queues round-robin
    long long* diag;  // the process's abort record in host memory (sf_df_diag), or NULL
    long long* dbg;   // tuning builds: per workgroup {ticks waiting, ticks in task bodies, tasks, ticks by type} (100 MHz)
    int miss_claims;  // tuning builds (SF_DF_MISS_CLAIMS): 1 = the dispenser leaves chain / front tasks to the waits' rescue while its queues hold tasks; 2 = a claimed chain task is never run (forces the stall bound)
    long long* trace; // tuning builds (SF_DF_TRACE_FILE): [0] = records written, then {type | k << 8 | i << 16 | b << 24 | workgroup << 40, claimed, body start, end}
    long long trace_cap;
    sf_df_stage_packed st[2][SF_DF_MAX_STAGES];
};
static_assert(sizeof(sf_df_args) <= 4096, "kernel arguments of k_potrf_dataflow");
#define SF_DF_LDS_DOUBLES ((37 * DBS + 128) > (4 * GT * GLD + 2 * GT) ? (37 * DBS + 128) : (4 * GT * GLD + 2 * GT))
#define SF_DF_LDS_BYTES ((SF_DF_LDS_DOUBLES + 4) * sizeof(double))

typedef const __attribute__((address_space(4))) sf_df_args sf_df_kargs;
// The dispenser's scans are real function calls (one lane, once per task): inlined at their three sites they pushed the
// register allocation of the whole task loop over the edge (a spill reload inside a K loop, tools/check_isa.py).
#define SF_DF_HELPER __attribute__((noinline))
#define SF_DF_PROGRESS() sf_df_add(a.abort_flag + 5, 1)
#ifdef SF_TUNING
#define SF_DF_MISS_CLAIMS(x) ((a.miss_claims & 1) && (x))
#else
#define SF_DF_MISS_CLAIMS(x) (false)
#endif
// A ready chain (d = 1) / front (d >= 2) task among the matrices of queue qx that nobody has claimed?  Claims it by
// compare-and-swap on the matrix's counter: cb = matrix, ck = chain task index (d = 1) or panel (d >= 2), cd = d.  One lane.
__device__ SF_DF_HELPER bool sf_df_try_chain(sf_df_kargs& a, const int qx, int& cb, int& ck, int& cd) {
    const int nt = a.nt, F = a.front;
    const int Bq = (a.batch - qx + SF_DF_QUEUES - 1) / SF_DF_QUEUES;
    const int vq = Bq == a.bq[0] ? 0 : 1;
    for (int dd = 1; dd <= F; ++dd) {  // (the chain itself first)
        for (int j = 0; j < Bq; ++j) {
            const int b1 = qx + SF_DF_QUEUES * j;
            int* ctr = a.chain_next + SF_DF_FRONT_MAX * b1 + dd - 1;
            const int k1 = sf_df_load(ctr);  // d = 1: chain task index (panel k1 - 1); d >= 2: panel - fstart
            const int kp = dd == 1 ? k1 - 1 : k1 + a.fstart[dd - 1];
            if (dd == 1 ? k1 >= nt : kp + dd > nt - 1) continue;
            bool ready = true;
            if (kp >= 0) {
                ready = sf_df_load(a.done_top + b1) >= kp;
                if (ready && kp >= 1) {
                    ready = sf_df_load(a.row_L + (size_t)b1 * nt + kp + dd) >= kp;
                    const int St = a.st[vq][kp - 1].split & 15;
                    if (ready && St > 0)
                        ready = sf_df_load(a.fp_cnt + 2 * SF_DF_FRONT_MAX * b1 + SF_DF_FRONT_MAX * (kp & 1) + dd - 1) >=
                                a.st[vq][kp - 1].thr_pt - a.thr_base[vq][kp & 1][dd - 1];
                }
            }
            if (!ready) continue;
            int expect = k1;
            if (__hip_atomic_compare_exchange_strong(ctr, &expect, k1 + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                cb = b1;
                ck = dd == 1 ? k1 : kp;
                cd = dd;
                return true;
            }
        }
    }
    return false;
}

template <bool RHS>
__global__ __launch_bounds__(512, 4) void k_potrf_dataflow(const sf_df_args a_in) {
    extern __shared__ __attribute__((aligned(16))) double dsm[];
    double* sm = dsm;
    double(*red)[GT] = (double(*)[GT])(dsm + 4 * GT * GLD);
    int* s_ints = (int*)(dsm + SF_DF_LDS_DOUBLES);  // [0] task id, [1] wait result, [2] [3] chain task: behind the kernels' LDS image, which starts at 0
    const size_t region = sf_split_region_tiles_dev() * (size_t)(GT * GT);
    // The arguments are read through the kernel-argument segment pointer inside the task loop, and everything derived from
    // the thread index is recomputed per task (the index is laundered through an empty asm): otherwise hipcc hoists the
    // lane-dependent invariants of all the inlined task bodies out of the loop and spills them (600 bytes of scratch per
    // lane, scratch loads inside the MFMA loops).
    sf_df_kargs* ap = (sf_df_kargs*)__builtin_amdgcn_kernarg_segment_ptr();
    (void)a_in;
    // (workgroup b of a launch runs on XCD b % 8 -- observed, not promised; placement is a speed matter only here: any
    // workgroup may serve any queue)
    // Workgroups are dealt to the queues in proportion to the MATRICES a queue holds (round 6): every matrix gets 512 / batch
    // workgroup slots.  A batch that is not a multiple of 8 leaves the first batch % 8 queues one matrix more than the others
    // (with fewer than 8 matrices: the others empty): the XCDs of the smaller queues keep round(matrices x 512 / batch) of
    // their 64 workgroups and send the rest to the larger queues, round-robin.  Before, such workgroups only moved on when
    // their own queue was exhausted -- with an empty own queue all of them to queue 0, whose one matrix then had five XCDs
    // (limited by its chain) while the others had one each (limited by throughput): N = 16384, 4 matrices 180 ms against 109
    // for the launch sequence; 12 matrices cost what 16 cost.  (8 % batch == 0: whole XCDs, the matrix's operands stay in
    // one L2.)
    int qcur = (int)(blockIdx.x & (SF_DF_QUEUES - 1));
    {
        const int nb = ap->batch, big = nb % SF_DF_QUEUES;  // queues 0 .. big - 1 hold one matrix more
        if (ap->qbal && big != 0) {
            if (nb < SF_DF_QUEUES && SF_DF_QUEUES % nb == 0) {
                qcur = qcur % nb;
            } else {
                const int mine = (nb - qcur + SF_DF_QUEUES - 1) / SF_DF_QUEUES;  // matrices of this XCD's own queue
                const int slot = (int)(blockIdx.x >> 3);
                const int keep = (int)(((long long)mine * gridDim.x + nb / 2) / nb);  // its share of the grid's workgroups
                if (qcur >= big && slot >= keep) qcur = (slot - keep + qcur) % big;
            }
        }
    }
    int visited = 0;
    int kst = 0;  // stage hint: a workgroup draws the tasks of a queue in increasing order
    if (threadIdx.x == 0) {
        s_ints[5] = 0;  // (idle spell of the end-of-launch phase, see the dispenser)
        s_ints[6] = 0;
        sf_df_add(ap->abort_flag + 6, 1);  // workgroups of the launch that have started (diagnostic of an aborted launch)
        if (blockIdx.x == 0)  // (where sf_df_report finds the abort record: the waits only carry the abort flag's address)
            __hip_atomic_store((long long*)(ap->abort_flag + 8), (long long)ap->diag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // A queued task whose wait was interrupted to run a chain / front task nobody had claimed (sf_df_wait_r): resume = 1 the
    // claimed chain task is in s_ints[0..4] already; pend_t >= 0: that queued task is taken up again instead of a new one.
    int pend_t = -1, resume = 0;
    for (;;) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        sf_df_kargs& a = *ap;
        const int nt = a.nt, F = a.front;
        const int n = a.p.n, fp = a.p.fp;
        const int B = (a.batch - qcur + SF_DF_QUEUES - 1) / SF_DF_QUEUES;  // matrices of this queue: qcur, qcur + 8, ...
        const int v = B == a.bq[0] ? 0 : 1;
        const int ntasks = B > 0 ? a.ntasks[v] : 0;
        // ---- dispenser.  Chain tasks first, then the queue of this workgroup's XCD, then the other queues.
        // (A claim can be missed: two workgroups that complete the last two dependencies of a chain task within a store's flight
        // time of each other may both read the other's counter too early and both find the task not ready.  The next
        // workgroup of the queue that passes here claims it, a few us later; if every workgroup of the queue sits in a wait
        // by then, the workgroups of the other queues do at the end of the launch, when each looks at every chain.  Measured
        // and not taken: waiting for this workgroup's counter stores to be acknowledged before the scan (2 % of a launch),
        // one lane per candidate instead of one lane walking the matrices (claims cost 20 instead of 28 us, launches of 8-32
        // matrices ran 2-5 % slower), waits that give up after 20 us to serve the chains and come back (3-14 % slower).
        // Since round 5 the window is closed where it matters: a queued task's wait that has lasted 500 us looks at the chains
        // itself, sf_df_wait_r.)
        if (resume) {  // s_ints[0..4] = the chain task claimed inside the interrupted wait
            resume = 0;
        } else if (pend_t >= 0) {  // back to the task that was set aside
            if (tid == 0) s_ints[0] = pend_t;
            pend_t = -1;
        } else if (tid == 0) {
            int t = -1, cb = 0, ck = 0, cd = 1;
            if (sf_df_load(a.abort_flag) == 0) {
                t = -2;
                auto try_chain = [&](int qx) { return SF_DF_MISS_CLAIMS(visited < SF_DF_QUEUES) ? false : sf_df_try_chain(a, qx, cb, ck, cd); };
                if (try_chain(qcur)) {
                    t = -3;
                } else if (visited < SF_DF_QUEUES) {
                    t = ntasks > 0 ? __hip_atomic_fetch_add(a.head + qcur, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ntasks;
                    if (t >= ntasks) t = -4;  // this queue is exhausted
                } else {
                    // every queue is exhausted: help the chains that are still running, leave when none is
                    bool live = false;
                    for (int qx = 0; qx < SF_DF_QUEUES && t == -2; ++qx)
                        if (try_chain(qx)) {
                            t = -3;
                            s_ints[5] = 0;
                        }
                    if (t == -2) {
                        for (int b1 = 0; b1 < a.batch; ++b1) {
                            live = live || sf_df_load(a.chain_next + SF_DF_FRONT_MAX * b1) < nt;
                            for (int dd = 2; dd <= F; ++dd)
                                live = live || sf_df_load(a.chain_next + SF_DF_FRONT_MAX * b1 + dd - 1) + a.fstart[dd - 1] + dd <= nt - 1;
                        }
                        if (!live) {
                            t = -5;
                        } else {
                            // (bounded like every wait: chains that stay open with nothing left to run them would spin here for ever)
                            // (s_ints[5]: the 10.5 ms unit of the wall clock at which this idle spell began -- or the launch's
                            // progress counter, s_ints[6], last moved --, + 1; 0 = none.  No task completed for three units, 21-31
                            // ms: SF_DF_STALL_TICKS)
                            const int now = (int)((wall_clock64() >> 20) & 0x3fffffff) + 1;
                            const int pg = sf_df_load(a.abort_flag + 5);
                            if (s_ints[5] == 0 || pg != s_ints[6]) {
                                s_ints[5] = now;
                                s_ints[6] = pg;
                            }
                            const int idle = (now - s_ints[5]) & 0x3fffffff;
                            const int stall = (int)(sf_df_stall_ticks(a.abort_flag) >> 20);
                            if (idle > stall) {
                                sf_df_report(a.abort_flag, a.chain_next, nt, SF_DF_ABORT_STALL, (long long)idle << 20);
                                t = -1;
                            }
                            __builtin_amdgcn_s_sleep(64);
                        }
                    }
                }
            }
            s_ints[0] = t;
            s_ints[2] = cb;
            s_ints[3] = ck;
            s_ints[4] = cd;
        }
        __syncthreads();
        const int t = __builtin_amdgcn_readfirstlane(s_ints[0]);  // (wave-uniform: everything decoded from it lives in SGPRs)
        const int chain_b = __builtin_amdgcn_readfirstlane(s_ints[2]), chain_k = __builtin_amdgcn_readfirstlane(s_ints[3]);
        const int chain_d = __builtin_amdgcn_readfirstlane(s_ints[4]);
        __syncthreads();
        if (t == -1) {  // a wait timed out somewhere: nothing of this launch can be trusted
            if (a.info)
                for (int bb = tid; bb < a.batch; bb += 512) a.info[bb] = SF_INFO_INTERNAL;
            return;
        }
        if (t == -5) return;
        if (t == -2) continue;
        if (t == -4) {  // this queue is exhausted: the next one
            ++visited;
            qcur = (qcur + 1) & (SF_DF_QUEUES - 1);
            kst = 0;
            continue;
        }

        // ---- decode: k = panel, i = slab, d = i - k for front tasks
        enum { T_C, T_FP, T_FR, T_R, T_RP, T_RR };
        int type, bl = 0, k, i = 0, sp = 0, S = 1, d = 0;
        int bchain = -1;
        if (t == -3) {
            type = chain_d == 1 ? T_C : T_FR;
            bchain = chain_b;
            k = chain_k;
            d = chain_d;
            i = k + d;
        } else {
            while (kst + 1 < nt - 1 && t >= a.st[v][kst + 1].off) ++kst;
            const sf_df_stage st = sf_df_stage_of(a.st[v][kst]);
            // front slabs of panel kst + 1 that exist, front slabs d >= 2 of this panel, ordinary slabs of this panel
            const int Fk = st.fw & 255, nF = st.fw >> 8;
            const int nord = max(0, nt - kst - 1 - Fk);
            const int n_fp = B * nF * st.St;
            const int n_r1 = B * nord * (st.Sr > 1 ? st.Sr : 1);
            // segment: fp_pos/256 of the rest tasks, the front partial sums of the NEXT panel, the other rest tasks, the reduces.
            // (FP tasks at the very front of the segment are claimed while the two rows they read are still being finished by
            // tasks of the previous stage: with many matrices per queue -- the chain is not what the rest waits for -- they
            // come later: 1.1 of 1.95 ms of waiting per workgroup at 32 matrices was theirs)
            const int n_r0 = (int)(((long long)n_r1 * a.fp_pos) >> 8);
            int u = t - st.off;
            if (u >= n_r0 && u < n_r0 + n_fp) {
                u -= n_r0;
                type = T_FP;
                k = kst + 1;
                S = st.St;
                d = 1 + u / (B * S);  // (d = 1 first: the chain's own partial sums)
                u -= (d - 1) * B * S;
                bl = u / S;
                sp = u - bl * S;
                i = k + d;
            } else if (u < n_r1 + n_fp) {
                if (u >= n_r0) u -= n_fp;
                k = kst;
                S = st.Sr;
                type = S > 1 ? T_RP : T_R;
                const int tile = u / S;  // ordinary slabs matrix by matrix: tasks side by side on an XCD stream the same B operand
                sp = u - tile * S;
                bl = tile / nord;
                i = k + 1 + Fk + (tile - bl * nord);
            } else {
                u -= n_r1 + n_fp;
                k = kst;
                S = st.Sr;
                type = T_RR;
                bl = u / nord;
                i = k + 1 + Fk + (u - bl * nord);
            }
        }
        bl = __builtin_amdgcn_readfirstlane(bl);  // (the divisions above ran on the VALU)
        i = __builtin_amdgcn_readfirstlane(i);
        sp = __builtin_amdgcn_readfirstlane(sp);
        k = __builtin_amdgcn_readfirstlane(k);
        S = __builtin_amdgcn_readfirstlane(S);
        d = __builtin_amdgcn_readfirstlane(d);
        type = __builtin_amdgcn_readfirstlane(type);
        const int b = bchain >= 0 ? bchain : qcur + SF_DF_QUEUES * bl;  // the matrix
#ifdef SF_TUNING
        // test aid (SF_DF_MISS_CLAIMS=2): the workgroup that claimed the chain task of panel 2 of matrix 0 never runs it --
        // what a workgroup that is kept from running looks like to the others: everything downstream waits, no task
        // completes any more, the stall bound gives the launch up (tests/test_gpu_recovery.py)
        if ((a.miss_claims & 2) && type == T_C && b == 0 && k == 2) {
            if (tid == 0)
                while (sf_df_load(a.abort_flag) == 0) __builtin_amdgcn_s_sleep(64);
            __syncthreads();
            continue;
        }
#endif
        const int vb = bchain >= 0 ? (((a.batch - (b & (SF_DF_QUEUES - 1)) + SF_DF_QUEUES - 1) / SF_DF_QUEUES) == a.bq[0] ? 0 : 1) : v;  // its queue's table
#ifdef SF_TUNING
        const long long dbg_t0 = wall_clock64();
        long long dbg_t1 = dbg_t0, dbg_top = 0;
#define SF_DF_MARK() dbg_t1 = wall_clock64()
#else
#define SF_DF_MARK()
#endif

        // ---- the per-task fields of the panel step (a.p holds what is constant over the factorisation)
        const auto& g = a.p;
        sf_panel_task q = {};
        q.nslab = 1;
        q.slab_step = 1;
        q.abort_flag = a.abort_flag;
        q.lds_int = s_ints + 1;
        q.sW = a.sT;
        auto Wof = [&](int kk) { return a.T + (size_t)(1 + kk) * GT * SF_LDT; };
        // front partial sums of (panel parity, front slab d, matrix): pt_cap tiles each in region 2; the body indexes them with
        // the matrix number b and the split S of the panel: base = slot of (parity, d, b) minus b S
        auto fpart = [&](int kk, int dd, int SS) {
            return a.part + 2 * region + (((int64_t)((kk & 1) * F + dd - 1) * a.batch + b) * a.pt_cap - (int64_t)b * SS) * (GT * GT);
        };
        int* fcnt = a.fp_cnt + 2 * SF_DF_FRONT_MAX * b;
        bool ok = true;
        int mode = 3, bid = b;  // which body runs: 1 = partial sums (bid = b S + split), 3 = everything else
        if (type == T_C || type == T_FR) {
            // the step of the front slab k+d (chain: of slab k for panel kp = k - 1) for panel kp: partial sums, K tail, epilogue
            const int kp = type == T_C ? k - 1 : k;
            const int slab = kp + d;
            if (type == T_C) {
                __builtin_amdgcn_s_setprio(2);  // the chain's waves share their SIMDs with rest tasks issuing MFMAs back to back
                q.Sout = a.T;                   // (g.sS = a.sT, g.ldS = SF_LDT)
            }
            if (kp < 0) {
                // start of the factorisation: diagonal tile 0 goes to the scratch unchanged (pw = 0, mode 0)
                if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                __syncthreads();
            } else {
                const sf_df_stage stp = sf_df_stage_of(a.st[vb][kp > 0 ? kp - 1 : 0]);  // (FP(., kp, ., .) belongs to stage kp - 1)
                const int St = kp >= 1 ? stp.St : 0;
                q.k0 = kp * GT;
                q.pw = min(GT, n - q.k0);
                q.row0 = slab * GT;
                q.Wt = Wof(kp);
                q.ksplit = St;
                q.ktail = St > 0 ? (kp - 1) * (GT / GK) : 0;
                q.part = fpart(kp, d, St);
                // the slab's own row left of the tail; row kp final = the FIRST half of the chain task C(b,kp) (only the solve
                // needs its second half, the diagonal tile: this task's K work runs beside it); the partial sums
                bool dready = false;
                // (own row: its L blocks left of the tail -- row_L; the slab's diagonal tile, updated by the previous panel's step
                // for this slab, is waited for inside the body, right before step 4)
                ok = sf_df_wait(kp >= 1 ? a.row_L + (size_t)b * nt + slab : nullptr, kp, a.done_top + b, kp,
                                St > 0 ? fcnt + SF_DF_FRONT_MAX * (kp & 1) + d - 1 : nullptr, stp.thr_pt - a.thr_base[vb][kp & 1][d - 1], a.done_D + b, kp + 1, &dready, a.abort_flag,
                                tid, s_ints + 1);
                if (!dready) {
                    q.wflag = a.done_D + b;
                    q.wval = kp + 1;
                }
                if (kp >= 1) {
                    q.sflag = a.done_row + (size_t)b * nt + slab;
                    q.sval = kp;
                }
                // (the row is published from inside the body, as soon as L is stored: the chain's row counter / the slab's row_L)
                q.top_flag = type == T_C ? a.done_top + b : a.row_L + (size_t)b * nt + slab;
                q.top_val = type == T_C ? k : kp + 1;
#ifdef SF_TUNING
                if (a.dbg && b == 0 && type == T_C && k < 64) q.stamps = a.dbg + 16 * SF_CHIP_WGS + 16 * 64 + 8 * k;
#endif
            }
        } else {
            // ---- queued tasks: ONE wait site for the four types (it carries the chain rescue, see sf_df_wait_r)
            const int k0 = k * GT;
            const int nk = (k0 > fp ? k0 - fp : 0) / GK;
            q.k0 = k0;
            q.pw = min(GT, n - k0);
            q.Wt = Wof(k);
            q.row0 = i * GT;
            const sf_df_stage st = sf_df_stage_of(a.st[vb][k]);
            const int Fk = st.fw & 255;
            const int nord = nt - k - 1 - Fk;
            int* rowflag = a.done_row + (size_t)b * nt + i;
            int* sdone = a.stage_done + (size_t)qcur * nt;
            const int *f1, *f2, *f3 = nullptr, *probe = nullptr;
            int t1, t2, t3 = 0;
            q.ksplit = S;
            if (type == T_FP) {
                // slab k+d, panel k, K slabs [fp / GK, (k - 1) 8): rows k and k+d through panel k-2; the slots' previous user (the
                // front task of (b, k-2, d)) must have read them: the chain's second half for d = 1, the row counter otherwise
                const int cnt = (k - 1) * (GT / GK) - fp / GK;
                q.kchunk = (cnt + S - 1) / S;
                q.kstop = (k - 1) * (GT / GK);
                q.part = fpart(k, d, S);
                f1 = a.done_row + (size_t)b * nt + k;
                t1 = k - 1;
                f2 = rowflag;
                t2 = k - 1;
                f3 = d == 1 ? a.done_D + b : a.done_row + (size_t)b * nt + i - 2;
                t3 = d == 1 ? k : k - 1;
            } else {
                q.kchunk = (nk + S - 1) / S;
                // (the body indexes the partial sums with the matrix number b: slot of (local matrix, slab) minus b S)
                q.part = a.part + (size_t)(k & 1) * region +
                         ((int64_t)qcur * SF_DF_QTILES + ((int64_t)bl * nord + (i - k - 1 - Fk) - b) * S) * (GT * GT);
                if (type == T_RR) {
                    f1 = a.rp_cnt + (size_t)b * nt + i;
                    t1 = st.thr_rp;
                    f2 = a.done_D + b;
                    t2 = k + 1;
                } else {
                    // K loop: row k through panel k-1 (the chain task's first half), the slab's own row through panel k-1; only
                    // the solve needs the diagonal tile -- if that is there already, this acquire covers it (T_R: probe)
                    f1 = k >= 1 ? a.done_top + b : nullptr;
                    t1 = k;
                    f2 = rowflag;
                    t2 = k;
                    if (type == T_R) {
                        probe = a.done_D + b;
                    } else if (st.dep >= 0) {  // T_RP re-uses the partial-sum slots of stage dep: its reduces must have read them
                        f3 = sdone + st.dep;
                        t3 = B * (nt - st.dep - 1 - (a.st[v][st.dep].fw & 255));
                    }
                }
            }
            bool dready = false;
            const int wr = sf_df_wait_r(f1, t1, f2, t2, f3, t3, probe, k + 1, &dready, a.abort_flag, tid, s_ints + 1,
                                        [&]() {  // (one lane) a ready chain / front task that nobody has claimed, on any queue
                                            int cb = 0, ck = 0, cd = 1;
                                            for (int x = 0; x < SF_DF_QUEUES; ++x) {
                                                const int qx = (qcur + x) & (SF_DF_QUEUES - 1);
                                                if (sf_df_try_chain(a, qx, cb, ck, cd)) {
                                                    s_ints[0] = -3;
                                                    s_ints[2] = cb;
                                                    s_ints[3] = ck;
                                                    s_ints[4] = cd;
                                                    return true;
                                                }
                                            }
                                            return false;
                                        },
                                        true);
            if (wr == SF_DF_DEFERRED) {  // a chain task first (claimed in the wait), then this task again
                pend_t = t;
                resume = 1;
                continue;
            }
            ok = wr == 1;
            if (type == T_FP || type == T_RP) {
                mode = 1;
                bid = b * S + sp;
            } else if (type == T_R) {  // the whole step: mode 3 without partial sums, K loop from the start
                q.ksplit = 0;
                q.ktail = 0;
                if (!dready) {
                    q.wflag = a.done_D + b;
                    q.wval = k + 1;
                }
            } else {  // T_RR: mode 3 with an empty K loop (the partial sums cover all of it)
                q.ktail = k0 / GK;
            }
        }
        // ---- the bodies: TWO inlined copies for the six task types -- the partial sums (FP, RP), and <3> for everything else: the
        // chain / front step as it is, the whole step (R) as <3> without partial sums, the reduce (RR) as <3> with an empty K
        // loop, the copy of diagonal tile 0 as <3> with pw = 0.  With one copy per type the kernel was 113 KB of code; the
        // instruction cache is 64 KB and shared by two CUs whose four workgroups run different task types (now: ~60 KB).
        SF_DF_MARK();
        if (ok) {
            if (mode == 1)
                sf_panel_body<RHS, 1>(g, q, bid, sm, red, tid);
            else
                sf_panel_body<RHS, 3>(g, q, bid, sm, red, tid);
        }
        if (type == T_C || type == T_FR) {
            const int kp = type == T_C ? k - 1 : k;
            const int slab = kp + d;
            if (ok && type == T_FR) {
                __syncthreads();
                if (tid == 0) {
                    sf_df_release();
                    sf_df_set(a.done_row + (size_t)b * nt + slab, kp + 1);
                    SF_DF_PROGRESS();  // (progress of the launch: see SF_DF_STALL_TICKS)
                }
            }
            if (ok && type == T_C) {
                __syncthreads();
#ifdef SF_TUNING
                dbg_top = wall_clock64();
#endif
                if (tid == 0) {  // the parked tile must be re-read through the L2 (k = 0: nothing was published from the body)
                    if (k == 0) {
                        sf_df_release();
                        sf_df_set(a.done_top + b, k);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                }
                __syncthreads();
                const int k0 = k * GT;
                const int pw = min(GT, n - k0);
                sf_diag_lds_body(a.T, a.sT, pw, a.info, k0 - fp, g.rhs ? g.rhs + k0 : nullptr, g.ldr,
                                 g.C + (int64_t)k0 * g.lda + k0, g.lda, g.sC, Wof(k), a.sT, k == 0 ? fp : 0, b, dsm, tid);
                __syncthreads();
                if (tid == 0) {
                    sf_df_release();
                    sf_df_set(a.done_D + b, k + 1);
                    SF_DF_PROGRESS();
                }
            }
            if (type == T_C) __builtin_amdgcn_s_setprio(0);
        } else {
            int* rowflag = a.done_row + (size_t)b * nt + i;
            int* sdone = a.stage_done + (size_t)qcur * nt;
            // (a workgroup that left the body on a timed-out wait finds the abort flag at the dispenser)
            __syncthreads();
            if (ok && tid == 0) {
                sf_df_release();
                if (type == T_FP) {
                    sf_df_add(fcnt + SF_DF_FRONT_MAX * (k & 1) + d - 1, 1);
                } else if (type == T_RP) {
                    sf_df_add(a.rp_cnt + (size_t)b * nt + i, 1);
                } else {
                    sf_df_set(a.row_L + (size_t)b * nt + i, k + 1);
                    sf_df_set(rowflag, k + 1);
                    if (type == T_RR) sf_df_add(sdone + k, 1);
                }
                SF_DF_PROGRESS();
            }
        }
        if (!ok) continue;  // (timed out: the dispenser sees the abort flag and flags every matrix)
        __syncthreads();  // the next task re-uses the LDS
#ifdef SF_TUNING
        if (a.dbg && tid == 0) {
            const long long t2 = wall_clock64();
            long long* dd = a.dbg + 16 * (size_t)blockIdx.x;
            dd[0] += dbg_t1 - dbg_t0;
            dd[1] += t2 - dbg_t1;
            dd[2] += 1;
            dd[3 + type] += t2 - dbg_t0;
            dd[9 + type] += dbg_t1 - dbg_t0;
            if (a.trace) {
                const long long slot = (long long)atomicAdd((unsigned long long*)a.trace, 1ull);
                if (slot < a.trace_cap) {
                    long long* r = a.trace + 4 + 4 * slot;
                    r[0] = (long long)type | ((long long)k << 8) | ((long long)i << 16) | ((long long)b << 24) | ((long long)blockIdx.x << 40);
                    r[1] = dbg_t0;
                    r[2] = dbg_t1;
                    r[3] = t2;
                }
            }
            if (b == 0 && k < 64) {  // timeline of matrix 0: chain task, its partial sums, the front slab d = 2
                long long* tr = a.dbg + 16 * SF_CHIP_WGS + 16 * k;
                const int slot = type == T_C ? 0 : (type == T_FP && d == 1 && sp == 0) ? 3 : (type == T_FP && d == 2 && sp == 0) ? 6 : (type == T_FR && d == 2) ? 9 : -1;
                if (slot >= 0) {
                    tr[slot] = dbg_t0;
                    tr[slot + 1] = dbg_t1;
                    tr[slot + 2] = t2;
                    if (type == T_C) tr[12] = dbg_top;
                }
            }
        }
#endif
    }
}
#undef SF_DF_MARK
#undef SF_DF_MISS_CLAIMS
#undef SF_DF_PROGRESS
#undef SF_DF_HELPER

// split factor of a stage's tasks: the largest power of two that keeps the stage within the workgroup slots of its queue's
// XCD and every K chunk at 8 slabs or more
static int sf_df_split(long long tasks, int nk, int smax, int cap) {
    int S = 1;
    while (2 * S <= smax && tasks * 2 * S <= cap && nk / (2 * S) >= 8) S *= 2;
    return S;
}

// sf_persistent_potrf(0): the callers' recovery after a launch that came back SF_INFO_INTERNAL -- from then on every
// factorisation of the process takes a launch sequence (no waits inside kernels), forced sequence 4 included.
static std::atomic<int> g_df_enabled{1};
int sf_set_persistent_potrf(int enable) {
    return enable < 0 ? g_df_enabled.load() : g_df_enabled.exchange(enable ? 1 : 0);
}
// What the stage tables and the front's partial-sum region hold.  Panels: n is a multiple of 64; an order of 64 mod 128 rows
// has (n + 64) / 128 of them in either frame (shifted by 64 virtual rows, sf_potrf_front_pad, or not) -- N = 16384 is 128
// panels = 127 stages, the tables' limit (the round-5 check added the 64 rows unconditionally: 129 panels, so N = 16384 never
// took the persistent kernel, forced or not).  Region 2 of `part` holds 2 x front x batch x pt_cap tiles with pt_cap >= 1.
static bool sf_df_fits(int n, int batch) {
    return (n + GT - 1) / GT - 1 <= SF_DF_MAX_STAGES && 2 * (size_t)SF_DF_FRONT_WIDEST * batch <= sf_split_region_tiles();
}
// ... and the persistent kernel is switched on: what sf_potrf_pick asks
static bool sf_potrf_dataflow_fits(int n, int batch) { return g_df_enabled.load() && sf_df_fits(n, batch); }

// The abort record of the process: six long longs of pinned host memory that the workgroup which aborts a persistent launch
// fills in (sf_df_report) and sf_persistent_potrf_status() hands to the caller's warning -- the status itself travels in
// d_info like every other (SF_INFO_INTERNAL).  Allocated on the first persistent launch; visible to every device.
static long long* g_df_diag = nullptr;
static std::atomic<long long> g_df_launches{0};
static long long* sf_df_diag(void) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (!g_df_diag) {
        void* p = nullptr;
        if (hipHostMalloc(&p, 8 * sizeof(long long), hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;  // (no record then: the launch itself does not depend on it)
        }
        for (int i = 0; i < 8; ++i) ((volatile long long*)p)[i] = 0;
        g_df_diag = (long long*)p;
    }
    return g_df_diag;
}
int sf_persistent_potrf_read_status(long long* out8) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    const volatile long long* d = g_df_diag;
    for (int i = 0; i < 6; ++i) out8[i] = d ? d[i] : 0;
    out8[6] = g_df_launches.load();
    out8[7] = g_df_enabled.load();
    return SF_OK;
}

// The counters of one persistent launch, as offsets in ints from `flags`: they live in the two inverse-tile buffers of the
// launch sequences (2 x batch x sW doubles), which this sequence does not use.  The last ndbg ints: the tuning builds' records.
struct sf_df_counters {
    int* flags;
    size_t head, abort_flag, done_top, done_D, chain_next, fp_cnt, done_row, row_L, rp_cnt, stage_done, ndbg, nflags;
    int* at(size_t off) const { return flags + off; }
};
static sf_df_counters sf_df_counters_of(int* flags, int batch, int nt) {
    const size_t b = (size_t)batch, fm = SF_DF_FRONT_MAX;
    sf_df_counters c = {flags, 0, 32};   // the queue heads [SF_DF_QUEUES]; the abort flag and its companions
    c.done_top = 64;                     // [batch], and so is done_D
    c.done_D = c.done_top + b;
    c.chain_next = c.done_D + b;         // [batch][SF_DF_FRONT_MAX]
    c.fp_cnt = c.chain_next + fm * b;    // [batch][2][SF_DF_FRONT_MAX]
    c.done_row = c.fp_cnt + 2 * fm * b;  // [batch][nt], and so are row_L and rp_cnt
    c.row_L = c.done_row + b * nt;
    c.rp_cnt = c.row_L + b * nt;
    c.stage_done = c.rp_cnt + b * nt;    // [SF_DF_QUEUES][nt]
    c.ndbg = 2 * (16 * SF_CHIP_WGS + 16 * 64 + 8 * 64);
    c.nflags = c.stage_done + (size_t)SF_DF_QUEUES * nt + 8 + c.ndbg;
    return c;
}

#ifdef SF_TUNING
// Tuning builds' reports of a persistent launch (stderr).  SF_DF_VERBOSE, ahead of the launch: the task tables ...
static void sf_df_tuning_tables(const sf_df_args& a, int n, long long total, int grid, const sf_df_stage* tab, int k_wide) {
    if (!SF_TUNE_FLAG("SF_DF_VERBOSE")) return;
    fprintf(stderr, "dataflow: n=%d nt=%d batch=%d tasks=%lld grid=%d lds=%zu bq=%d/%d St/Sr:", n, a.nt, a.batch, total, grid,
            (size_t)SF_DF_LDS_BYTES, a.bq[0], a.bq[1]);
    for (int k = 0; k + 1 < a.nt; ++k) fprintf(stderr, " %d/%d%s", tab[k].St, tab[k].Sr, k == k_wide ? "|" : "");
    fprintf(stderr, "\n");
}
// ... and behind it (these synchronise): SF_DF_CHECK names the wait that timed out and dumps the counters, SF_DF_VERBOSE sums
// the workgroups' records, SF_DF_TRACE prints matrix 0's chain, SF_DF_TRACE_FILE writes every task.  Frees a.trace.
static void sf_df_tuning_report(const sf_df_args& a, const sf_df_counters& cn, int n, int grid, const char* trace_file, hipStream_t s) {
    const int batch = a.batch, nt = a.nt, F = a.front;
    if (SF_TUNE_FLAG("SF_DF_CHECK")) {  // which wait timed out?
        int ab[4];
        (void)hipStreamSynchronize(s);
        (void)hipMemcpy(ab, a.abort_flag, sizeof(ab), hipMemcpyDeviceToHost);
        if (ab[0]) {
            const long off = ab[1] + (long)cn.abort_flag;  // offset from `flags`
            const struct {
                const char* what;
                size_t base;
                long per;
            } arrays[] = {{"stage_done[q][k]", cn.stage_done, nt}, {"rp_cnt[b][i]", cn.rp_cnt, nt}, {"row_L[b][i]", cn.row_L, nt},
                          {"done_row[b][i]", cn.done_row, nt}, {"fp_cnt[b][parity][d]", cn.fp_cnt, 2 * SF_DF_FRONT_MAX},
                          {"chain_next", cn.chain_next, 1}, {"done_D[b]", cn.done_D, 1}, {"done_top[b]", cn.done_top, 1}};
            int w = 0;
            while (w < 7 && off < (long)arrays[w].base) ++w;
            const long rel = off - (long)arrays[w].base, per = arrays[w].per;
            fprintf(stderr, "dataflow ABORTED (n=%d batch=%d front=%d): a wait for %s index %ld / %ld (target %d, value %d) timed out\n", n, batch, F,
                    arrays[w].what, rel / per, rel % per, ab[2], ab[3]);
            std::vector<int> fl(cn.nflags - cn.ndbg);
            (void)hipMemcpy(fl.data(), cn.flags, sizeof(int) * fl.size(), hipMemcpyDeviceToHost);
            for (int bb = 0; bb < batch; ++bb) {
                fprintf(stderr, "  b=%d: done_top %d done_D %d chain_next", bb, fl[cn.done_top + bb], fl[cn.done_D + bb]);
                for (int d = 0; d < F; ++d) fprintf(stderr, " %d", fl[cn.chain_next + SF_DF_FRONT_MAX * bb + d]);
                fprintf(stderr, " | row_L:");
                for (int i = 0; i < nt; ++i) fprintf(stderr, " %d", fl[cn.row_L + (size_t)bb * nt + i]);
                fprintf(stderr, " | done_row:");
                for (int i = 0; i < nt; ++i) fprintf(stderr, " %d", fl[cn.done_row + (size_t)bb * nt + i]);
                fprintf(stderr, "\n");
            }
            fprintf(stderr, "  queue heads:");
            for (int qx = 0; qx < SF_DF_QUEUES; ++qx) fprintf(stderr, " %d", fl[cn.head + qx]);
            fprintf(stderr, " of %d / %d tasks\n", a.ntasks[0], a.ntasks[1]);
        }
    }
    if (!a.dbg) return;
    static long long host[16 * SF_CHIP_WGS + 16 * 64 + 8 * 64];
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(host, a.dbg, sizeof(host), hipMemcpyDeviceToHost);
    double w = 0, bd = 0, nn = 0, ty[6] = {0, 0, 0, 0, 0, 0}, tw[6] = {0, 0, 0, 0, 0, 0};
    long long wmax = 0, bmax = 0;
    for (int i = 0; i < grid; ++i) {
        w += host[16 * i];
        bd += host[16 * i + 1];
        nn += host[16 * i + 2];
        for (int j = 0; j < 6; ++j) ty[j] += host[16 * i + 3 + j];
        for (int j = 0; j < 6; ++j) tw[j] += host[16 * i + 9 + j];
        wmax = std::max(wmax, host[16 * i]);
        bmax = std::max(bmax, host[16 * i] + host[16 * i + 1]);
    }
    if (SF_TUNE_FLAG("SF_DF_TRACE")) {
        const long long* tr = host + 16 * SF_CHIP_WGS;
        long long t0 = tr[0];
        fprintf(stderr, "matrix 0, us since its first task: k | C claim start end | FP(k,1) claim start end | FP(k,2) claim start end | FR(k,2) claim start end\n");
        for (int k = 1; k < nt && k < 64; ++k) {  // (k = 0 has no panel part)
            fprintf(stderr, "%2d |", k);
            for (int j = 0; j < 12; ++j) fprintf(stderr, "%s%8.1f", j % 3 == 0 && j ? " |" : "", tr[16 * k + j] ? (tr[16 * k + j] - t0) / 100.0 : 0.0);
            const long long* st4 = host + 16 * SF_CHIP_WGS + 16 * 64 + 8 * k;
            fprintf(stderr, " | C: reduce %6.1f + tail %6.1f", (st4[5] - tr[16 * k + 1]) / 100.0, (st4[0] - st4[5]) / 100.0);
            fprintf(stderr, " | C: K work %6.1f, wait D %6.1f, solve+store %6.1f, wait S %6.1f, step 4 %6.1f, D %6.1f\n",
                    (st4[0] - tr[16 * k + 1]) / 100.0, (st4[1] - st4[0]) / 100.0, (st4[2] - st4[1]) / 100.0, (st4[3] - st4[2]) / 100.0,
                    (tr[16 * k + 12] - st4[3]) / 100.0, (tr[16 * k + 2] - tr[16 * k + 12]) / 100.0);
        }
    }
    fprintf(stderr, "dataflow per workgroup: waiting %.2f ms (max %.2f), bodies %.2f ms, busy max %.2f ms, %.0f tasks; by type C %.2f FP %.2f FR %.2f R %.2f RP %.2f RR %.2f ms\n",
            w / grid / 1e5, wmax / 1e5, bd / grid / 1e5, bmax / 1e5, nn / grid, ty[0] / grid / 1e5, ty[1] / grid / 1e5, ty[2] / grid / 1e5,
            ty[3] / grid / 1e5, ty[4] / grid / 1e5, ty[5] / grid / 1e5);
    if (a.trace) {
        std::vector<long long> tr(4 + 4 * (size_t)a.trace_cap);
        (void)hipMemcpy(tr.data(), a.trace, sizeof(long long) * tr.size(), hipMemcpyDeviceToHost);
        (void)hipFree(a.trace);
        if (FILE* f = fopen(trace_file, "w")) {
            const long long nrec = std::min<long long>(tr[0], a.trace_cap);
            fprintf(f, "# n=%d batch=%d nt=%d front=%d grid=%d: type(C FP FR R RP RR) k i b workgroup claimed start end (10 ns ticks)\n", n, batch, nt, F, grid);
            for (long long r = 0; r < nrec; ++r) {
                const long long* e = &tr[4 + 4 * r];
                fprintf(f, "%lld %lld %lld %lld %lld %lld %lld %lld\n", e[0] & 255, (e[0] >> 8) & 255, (e[0] >> 16) & 255, (e[0] >> 24) & 65535, e[0] >> 40, e[1], e[2], e[3]);
            }
            fclose(f);
        }
    }
    fprintf(stderr, "dataflow waiting by type: C %.2f FP %.2f FR %.2f R %.2f RP %.2f RR %.2f ms\n", tw[0] / grid / 1e5, tw[1] / grid / 1e5,
            tw[2] / grid / 1e5, tw[3] / grid / 1e5, tw[4] / grid / 1e5, tw[5] / grid / 1e5);
}
#endif

static int sf_launch_potrf_v4(double* A, int n, int lda, int64_t stride, int* info, const sf_potrf_scratch& ws, double* rhs,
                              int ldr, hipStream_t s, const sf_gen_args* gen, int fp) {
    const int batch = ws.batch;
    static sf_dev_once attr_once;
    SF_CHECK(sf_lds_limit_once(&attr_once, (int)SF_DF_LDS_BYTES, {(const void*)k_potrf_dataflow<true>, (const void*)k_potrf_dataflow<false>}));
    const int nt = (n + GT - 1) / GT;
    const sf_df_counters cn = sf_df_counters_of((int*)ws.W, batch, nt);
    // (what sf_potrf_pick asked, and the counters must fit their buffers: a forced sequence 4 falls back in sf_potrf_pick)
    if (!sf_df_fits(n, batch) || cn.nflags * sizeof(int) > ws.Wdoubles() * sizeof(double)) {
        sf_set_error("potrf: dataflow sequence: %d panels / %d matrices do not fit its tables", nt, batch);
        return SF_EINVAL;
    }
    sf_df_args a = {};
    a.head = cn.at(cn.head), a.abort_flag = cn.at(cn.abort_flag);
    a.done_top = cn.at(cn.done_top), a.done_D = cn.at(cn.done_D), a.chain_next = cn.at(cn.chain_next), a.fp_cnt = cn.at(cn.fp_cnt);
    a.done_row = cn.at(cn.done_row), a.row_L = cn.at(cn.row_L), a.rp_cnt = cn.at(cn.rp_cnt), a.stage_done = cn.at(cn.stage_done);
    SF_HIP(hipMemsetAsync(cn.flags, 0, cn.nflags * sizeof(int), s));
    SF_HIP(hipMemsetAsync(info, 0, sizeof(int) * (size_t)batch, s));
#ifdef SF_TUNING
    // test aids: a launch that finds its abort flag raised (every matrix comes back SF_INFO_INTERNAL: the callers' recovery
    // path); a dispenser that leaves every chain / front task to the rescue of the waits (sf_df_wait_r)
    if (SF_TUNE_FLAG("SF_DF_FORCE_ABORT")) SF_HIP(hipMemsetAsync(a.abort_flag, 1, 1, s));
    static const int timeout_s = SF_TUNE_INT("SF_DF_TIMEOUT_S", 0);  // (bound of the waits in seconds instead of 4)
    if (timeout_s > 0) SF_HIP(hipMemsetD32Async((hipDeviceptr_t)(a.abort_flag + 4), timeout_s * 95, 1, s));
    // (no-progress bound in ms instead of 25; with SF_DF_TIMEOUT_S alone the stall bound follows it: the experiment that showed
    // the shared-device deadlock to be one -- a launch still stuck after 60 s -- stays reproducible)
    static const int stall_ms = SF_TUNE_INT("SF_DF_STALL_MS", 0);
    const long long stall_units = stall_ms > 0 ? ((long long)stall_ms * 100000) >> 16 : (timeout_s > 0 ? ((long long)timeout_s * 100000000) >> 16 : 0);
    if (stall_units > 0) SF_HIP(hipMemsetD32Async((hipDeviceptr_t)(a.abort_flag + 7), (int)std::min<long long>(stall_units, 0x7fffffff), 1, s));
    a.miss_claims = SF_TUNE_INT("SF_DF_MISS_CLAIMS", 0);
#endif

    a.p = sf_panel_frame<sf_panel_args>(A, n, lda, stride, rhs, ldr, gen, fp);
    a.p.sS = ws.sT;  // (the parked diagonal tile of matrix b: T + b sT, row stride SF_LDT)
    a.p.ldS = SF_LDT;
    // front width: the rows the chain needs next must be a reduce-and-epilogue behind it, and the first ORDINARY slab of a
    // stage (a long-K task, or partial sums + reduce) gets `front` chain periods before the front needs its row.  Front tasks
    // cost more than ordinary ones (partial sums written and read back).  N = 4096, front 1 / 2 / 3 / 4 / 6: B = 16 8.1 / 8.0 /
    // 7.87 / 7.84 / 7.85 ms, B = 32 13.7 / 13.8 / 13.7 / 13.9 / 14.6, B = 64 25.45 / 25.7 / 26.3 / 26.85 / 28.0
    const int F0 = batch <= 20 ? 3 : 1;
    // ... and for 21-48 matrices the front widens to three slabs for the last panels: where a stage has fewer tasks than the
    // chip has workgroup slots (batch x slabs left <= 400) AND its K loops are long (2048 columns or more: the front keeps
    // long-K tasks out of the chain's way, its partial sums cost a round trip through memory).  Same-box, wide front from
    // that panel on / never: N = 4096: B = 24 10.55 / 11.2 ms, 32: 13.42 / 13.65, 40: 16.7 / 16.93, 48: 19.75 / 19.8,
    // 64: 25.7 / 25.5 (not taken from 49 matrices on); N = 3008, B = 32: 6.2 / 6.25; a wide front over the short K loops
    // of N = 2048 loses 3-5 %.
    const int Ftail = SF_DF_FRONT_WIDEST;
    const int kT = batch > 20 && batch <= 48 ? std::max(2048 / GT, nt - 400 / batch) : nt;  // first panel of the wide front
    auto Fof = [&](int k) { return k >= kT ? Ftail : F0; };
    const int F = Ftail;  // (the largest width: strides of the front's partial sums and counters; sf_df_fits counted with it)
    a.front = F;
    for (int d = 1; d <= SF_DF_FRONT_MAX; ++d) a.fstart[d - 1] = d <= F0 ? 0 : kT;
    a.fp_pos = 256;  // (0 / 64 / 128 / 192 / 256: B = 16 7.75 / 7.7 / 7.6 / 7.7 / 7.55 ms, B = 32 13.8 / 13.9 / 13.75 / 13.7 / 13.65)
    a.nt = nt;
    a.batch = batch;
    a.T = ws.T;
    a.sT = ws.sT;
    a.part = ws.part;
    a.info = info;
    a.diag = sf_df_diag();
    a.qbal = 1;
#ifdef SF_TUNING
    if (SF_TUNE_FLAG("SF_DF_VERBOSE")) a.dbg = (long long*)cn.at((cn.nflags - cn.ndbg + 1) & ~(size_t)1);
    static const char* trace_file = SF_TUNE_STR("SF_DF_TRACE_FILE");  // every task's {what, claimed, body start, end} as text
    if (trace_file && a.dbg) {
        a.trace_cap = 1 << 18;
        SF_HIP(hipMalloc((void**)&a.trace, sizeof(long long) * (4 + 4 * (size_t)a.trace_cap)));
        SF_HIP(hipMemsetAsync(a.trace, 0, sizeof(long long) * 4, s));
    }
#endif

    // ---- the task tables: one per queue size (ceil and floor of batch / 8)
    // workgroup slots a queue can count on: those of one XCD -- of 8 / batch XCDs when there are fewer matrices than queues
    // (bounded by the partial-sum tiles a queue owns)
    auto cap_of = [&](int Bq) {
        if (batch % SF_DF_QUEUES == 0) return SF_CHIP_WGS / SF_DF_QUEUES;
        return std::max(16, std::min<int>(SF_DF_QTILES, (int)((long long)Bq * SF_CHIP_WGS / batch)));
    };
    // front partial-sum tasks per queue, panel and front slab (64 / 32 / 16 / 8 with a one-slab front: B = 32 14.9 / 14.8 / 14.55 /
    // 14.45 ms, B = 48 20.8 / 20.2 / 20.2 / 20.6)
    const int pt_tasks = 16;
    const int kpb = GT / GK;
    const int st_cap = (int)std::min<size_t>(SF_SPLIT_MAX, std::max<size_t>(1, sf_split_region_tiles() / (2 * (size_t)F * (size_t)batch)));
    a.pt_cap = st_cap;
    a.bq[0] = (batch + SF_DF_QUEUES - 1) / SF_DF_QUEUES;
    a.bq[1] = batch / SF_DF_QUEUES;
    static thread_local sf_df_stage tab[2][SF_DF_MAX_STAGES];
    for (int v = 0; v < 2; ++v) {
        const int B = a.bq[v];
        if (B <= 0 || (v == 1 && a.bq[1] == a.bq[0])) {
            a.ntasks[v] = v == 1 ? a.ntasks[0] : 0;
            continue;
        }
        const int cap = cap_of(B);
        int off = 0, thr_pt[2] = {0, 0}, thr_rp = 0, last_split[2] = {-1, -1};
        bool seen[2][SF_DF_FRONT_MAX] = {};
        for (int k = 0; k + 1 < nt; ++k) {
            sf_df_stage& st = tab[v][k];
            st.off = off;
            // FP(., k+1, ., .): K slabs [fp / GK, k 8) of panel k+1 (everything left of panel k)
            const int nF = std::max(0, std::min(Fof(k + 1), nt - 1 - (k + 1)));
            const int nord = std::max(0, nt - k - 1 - Fof(k));
            st.fw = Fof(k) | (nF << 8);
            const int cnt_pt = nF > 0 ? k * kpb - fp / GK : 0;
            st.St = cnt_pt >= 8 ? sf_df_split(B, cnt_pt, st_cap, pt_tasks) : 0;
            for (int d = 1; d <= nF; ++d)  // (a distance that appears with the wide front has missed the arrivals counted so far)
                if (!seen[(k + 1) & 1][d - 1]) {
                    seen[(k + 1) & 1][d - 1] = true;
                    a.thr_base[v][(k + 1) & 1][d - 1] = thr_pt[(k + 1) & 1];
                }
            thr_pt[(k + 1) & 1] += st.St;
            st.thr_pt = thr_pt[(k + 1) & 1];
            const int nk = (k * GT > fp ? k * GT - fp : 0) / GK;
            st.Sr = nord > 0 ? sf_df_split((long long)B * nord, nk, SF_SPLIT_MAX, cap) : 1;
            while (st.Sr > 1 && (size_t)B * nord * st.Sr > SF_DF_QTILES) st.Sr /= 2;
            st.dep = -1;
            if (st.Sr > 1) {
                thr_rp += st.Sr;
                st.dep = last_split[k & 1];
                last_split[k & 1] = k;
            }
            st.thr_rp = thr_rp;
            off += B * nF * st.St + B * nord * (st.Sr > 1 ? st.Sr + 1 : 1);
        }
        a.ntasks[v] = off;
    }
    if (a.bq[1] == a.bq[0]) {
        for (int k = 0; k + 1 < nt; ++k) tab[1][k] = tab[0][k];
        for (int par = 0; par < 2; ++par)
            for (int d = 0; d < SF_DF_FRONT_MAX; ++d) a.thr_base[1][par][d] = a.thr_base[0][par][d];
    }
    for (int v = 0; v < 2; ++v)
        for (int k = 0; k + 1 < nt; ++k) a.st[v][k] = sf_df_pack(tab[v][k]);
    // algorithmic flops (as the launch sequences count them): update, solve, diagonal-tile update of every panel
    double flops = 0.0;
    for (int k = 0; k + 1 < nt; ++k) {
        const int k0 = k * GT, pw = std::min(GT, n - k0);
        const double rows = (double)(n - (k + 1) * GT);
        flops += (2.0 * (k0 > fp ? k0 - fp : 0) * rows * pw + rows * pw * (double)pw + (double)GT * rows * pw) * batch;
    }
    long long total = (long long)batch * nt * F;  // the chain and front tasks
    for (int qx = 0; qx < SF_DF_QUEUES; ++qx) {
        const int B = (batch - qx + SF_DF_QUEUES - 1) / SF_DF_QUEUES;
        if (B > 0) total += a.ntasks[B == a.bq[0] ? 0 : 1];
    }
    const int grid = (int)std::min<long long>(total, SF_CHIP_WGS);
#ifdef SF_TUNING
    sf_df_tuning_tables(a, n, total, grid, tab[0], Ftail > F0 ? kT : -1);
#endif
    void* tok;
    sf_prof_gemm_begin(s, flops, &tok);
    if (rhs)
        hipLaunchKernelGGL(k_potrf_dataflow<true>, dim3(grid), dim3(512), SF_DF_LDS_BYTES, s, a);
    else
        hipLaunchKernelGGL(k_potrf_dataflow<false>, dim3(grid), dim3(512), SF_DF_LDS_BYTES, s, a);
    g_df_launches.fetch_add(1);
    sf_prof_gemm_end(tok);
    SF_LAUNCH_CHECK();
#ifdef SF_TUNING
    sf_df_tuning_report(a, cn, n, grid, trace_file, s);
#endif
    return SF_OK;
}
