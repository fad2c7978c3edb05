// What the multi-order calls share (internal; sf_multi.cpp: the dense calls, sf_multi_banded.cpp: the band solver's): the
// frame of a segment list, the checks of the gradient requests and the lane / chunk pipeline of their launch sequences.
#pragma once
#include <algorithm>
#include <vector>

#include "sf_stages.h"

#pragma GCC visibility push(hidden)
// models[i] describes the rows of segment i; *uni receives what the shared buffers are sized for (segment 0's
// descriptor with has_vsini set if ANY segment broadens: the transient buffers of the transform chains are shared)
int multi_layout(const sf_segment* segs, int nseg, const sf_model_desc* const* models, Layout* L, int* units, int* bmax,
                 sf_model_desc* uni);
// every per-segment requirement of the two single-order gradient calls, for the segment that requests the part (behind
// multi_layout: contexts and models are good)
// call: the entry point the messages name
int multi_grad_requests_ok(const sf_segment* segs, int nseg, const sf_model_desc* const* models, const sf_grad_request* reqs,
                           int grad_stride, const char* call);
#pragma GCC visibility pop

// Chunks of a multi-order call (whole segments): a SMALL first chunk (at least 256 units: enough matrices to keep a
// factorisation's launches full) and the rest as the second -- only the first chunk's fills are exposed, the others
// run behind the first factorisation.  (Equal chunks: 1, 2, 3, 4 of them gave 283.1, 282.1, 282.7, 283.9 ms at cfg 3.)
// (the band solver's gradient with a chunk every 256 units instead: 51.7 against 51.2 ms of device time at 25 x 3000 x 64)
// Orders whose transform chains + fills run side by side (own stream and own set of transient buffers each): a chain is
// ~14 small dependent launches, latency-bound -- alone it takes ~1 ms per order with the chip idle around it.
#define SF_MULTI_LANES 3  // (4, 6 and 8 lanes measured: no further gain)
static int multi_first_units(int U) { return std::min(U, 256); }

struct MultiChunk {
    int u0, units;
    hipEvent_t filled[SF_MULTI_LANES];  // per lane that has a segment of the chunk: everything of them is enqueued
    int s0, s1;                         // its segments [s0, s1)
};
struct MultiSegment {
    int lane;
    hipStream_t stream;
    int u0;  // the segment's first unit
};
// The pipeline of a call's launch sequence: the per-segment work (many small launches) runs on the lanes -- streams of the
// context's executor -- one chunk of segments ahead of the per-chunk work on the caller's stream, so all but the first chunk's
// is hidden behind the previous chunk's.  Bookkeeping only: the caller enqueues between start() and done(), and behind join().
// (no stream is created for the lanes: every additional ACTIVE stream costs dispatch latency on all of them --
// one more for the wide sequence's A launches made a cfg-2 step 3 % slower)
struct MultiPipeline {
    sf_exec* ex;
    hipStream_t s, lane_stream[SF_MULTI_LANES];
    int nseg, first_units;
    std::vector<MultiChunk> chunks;
    std::vector<int> seg_u0;
    bool lane_used[SF_MULTI_LANES] = {};
    int u0 = 0, cu0 = 0, cs0 = 0;

    // the lanes wait for what the caller's stream s holds; U: the units of the call
    int begin(sf_exec* exec, hipStream_t stream, int nsegments, int U) {
        ex = exec, s = stream, nseg = nsegments, first_units = multi_first_units(U);
        SF_CHECK(sf_exec_prepare(ex));
        lane_stream[0] = ex->aux, lane_stream[1] = ex->side, lane_stream[2] = ex->grp[0];
        seg_u0.assign(nseg, 0);
        SF_HIP(hipEventRecord(ex->fork, s));
        for (int l = 0; l < SF_MULTI_LANES; ++l) SF_HIP(hipStreamWaitEvent(lane_stream[l], ex->fork, 0));
        return SF_OK;
    }
    MultiSegment start(int i) {
        const int lane = i % SF_MULTI_LANES;
        lane_used[lane] = true;
        seg_u0[i] = u0;
        return MultiSegment{lane, lane_stream[lane], u0};
    }
    // segment i of B units is enqueued: closes a chunk when the rule above says so (its events in lane order)
    int done(int i, int B) {
        u0 += B;
        if (!((chunks.empty() && u0 - cu0 >= first_units) || i == nseg - 1)) return SF_OK;
        MultiChunk ch{cu0, u0 - cu0, {}, cs0, i + 1};
        for (int l = 0; l < SF_MULTI_LANES; ++l) {
            if (!lane_used[l]) continue;
            SF_CHECK(sf_exec_event(ex, &ch.filled[l]));
            SF_HIP(hipEventRecord(ch.filled[l], lane_stream[l]));
            lane_used[l] = false;
        }
        chunks.push_back(ch);
        cu0 = u0, cs0 = i + 1;
        return SF_OK;
    }
    // the caller's stream waits for the chunk's segments
    int join(const MultiChunk& ch) const {
        for (int l = 0; l < SF_MULTI_LANES; ++l)
            if (ch.filled[l]) SF_HIP(hipStreamWaitEvent(s, ch.filled[l], 0));
        return SF_OK;
    }
};
