// replay.h — one replay of a captured HIP graph from ONE host call, the body of dlrm_graph_replay (loss_opt.hip: a training step) and
// dlrm_forward_replay (stage.hip: a forward).  The order is the protocol of dlrm_amd/graph_core.py and the same for both:
//   1. every segment is checked before anything touches the device;
//   2. sync_first: wait for everything enqueued on the stream — the previous replay, which shares every buffer with this one.  Polled, not
//      slept on (dlrm_stream_wait_polling, common.h);
//   3. the inputs go into the static buffers: at most memcpy_max_segs segments with one hipMemcpyAsync each, more with dlrm_stage_inputs
//      (one launch per 64 copying segments).  A segment that is empty or already in place (dst == src) copies nothing;
//   4. n_scalars > 0: device floats written in front of the launch (dlrm_set_f32: the learning rates the captured update kernels read);
//   5. hipGraphLaunch.
// At Criteo-Kaggle shapes the GPU finishes a replay in ~0.3 ms and then waits for the host; the same sequence issued from Python
// (stream.synchronize(), one copy_ per input, CUDAGraph.replay()) was ~60 us of that wait.
#pragma once
#include <limits.h>
#include "common.h"

static inline int dlrm_replay(int n_seg, void* const* dst_host, const void* const* src_host, const int64_t* bytes_host, int memcpy_max_segs,
                              int n_scalars, float* const* scalar_dst_host, const float* scalar_values_host, void* graph_exec,
                              int sync_first, void* stream) {
    if (n_seg < 0 || !graph_exec || (n_seg > 0 && (!dst_host || !src_host || !bytes_host))) return DLRM_E_ARG;
    for (int i = 0; i < n_seg; ++i)
        if (!dst_host[i] || !src_host[i] || bytes_host[i] < 0) return DLRM_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (sync_first) {
        const hipError_t e = dlrm_stream_wait_polling(st);
        if (e != hipSuccess) return (int)e;
    }
    if (n_seg <= memcpy_max_segs) {
        for (int i = 0; i < n_seg; ++i) {
            if (dst_host[i] == src_host[i] || bytes_host[i] == 0) continue;
            const hipError_t e = hipMemcpyAsync(dst_host[i], src_host[i], (size_t)bytes_host[i], hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return (int)e;
        }
    } else {
        const int rc = dlrm_stage_inputs(n_seg, dst_host, src_host, bytes_host, stream);
        if (rc) return rc;
    }
    if (n_scalars > 0) {          // (a schedule changed the step sizes: written behind the previous replay, in front of this one)
        const int rc = dlrm_set_f32(n_scalars, scalar_dst_host, scalar_values_host, stream);
        if (rc) return rc;
    }
    const hipError_t e = hipGraphLaunch((hipGraphExec_t)graph_exec, st);
    return e == hipSuccess ? 0 : (int)e;
}
