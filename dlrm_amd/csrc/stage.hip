// stage.hip — the inputs of one inference request into a captured forward's static buffers in ONE launch, and the forward's replay call
// (dlrm_amd.graph.GraphedForward).  A request is X plus T index tensors plus T offset tensors, usually Python lists: 53 tensors at
// Criteo-Kaggle's 26 tables, each a few hundred bytes to a few KiB.  One hipMemcpyAsync per tensor is 53 runtime calls in front of a
// graph whose whole replay is a few hundred microseconds; here the (destination, source, length) triples travel BY VALUE in the kernarg,
// like every other multi-table launch of this library, and one grid copies them all.
#include "common.h"
#include "replay.h"

namespace {

#define DLRM_MAX_STAGE_SEGS 64
struct StageArgs {                      // 64 x 24 B = 1.5 KiB of kernarg
    char*       dst[DLRM_MAX_STAGE_SEGS];
    const char* src[DLRM_MAX_STAGE_SEGS];
    long long   bytes[DLRM_MAX_STAGE_SEGS];
};

constexpr int kStageBlock = 256;
constexpr int kStageMaxBlocksX = 256;

template <typename V>
__device__ __forceinline__ void stage_body(char* __restrict__ d, const char* __restrict__ s, long long count, long long tid, long long stride) {
    V* __restrict__ dv = reinterpret_cast<V*>(d);
    const V* __restrict__ sv = reinterpret_cast<const V*>(s);
    for (long long e = tid; e < count; e += stride) dv[e] = sv[e];
}

// blockIdx.y = segment, blockIdx.x strides its bytes.  Every pointer and length is a multiple of 4 (checked on the host).  The widest element
// both pointers admit TOGETHER is the body's: 16 bytes when destination and source are congruent modulo 16, 8 when modulo 8, else 4; up to
// three 4-byte words in front bring the destination (and with it the source) to that boundary, up to three behind finish the segment.
// Segments are tiny (n * 8 bytes for an id row at n = 1 is ONE word): nothing here assumes a full block of work, a thread with nothing to do
// falls through.  No LDS, no atomics; plain vector loads and stores.
__global__ __launch_bounds__(kStageBlock) void stage_inputs_kernel(StageArgs a) {
    const int seg = blockIdx.y;
    char* __restrict__ d = a.dst[seg];
    const char* __restrict__ s = a.src[seg];
    const long long n = a.bytes[seg];
    if (n <= 0) return;
    const unsigned rel = (unsigned)(((uintptr_t)d ^ (uintptr_t)s) & 15u);
    const int unit = rel == 0u ? 16 : ((rel & 7u) == 0u ? 8 : 4);
    long long head = (long long)((unit - (int)((uintptr_t)d & (uintptr_t)(unit - 1))) & (unit - 1));
    if (head > n) head = n;
    const long long body = (n - head) / unit;                 // elements of `unit` bytes
    const long long tail0 = head + body * unit;               // first byte behind the body
    const long long tid = (long long)blockIdx.x * kStageBlock + threadIdx.x;
    const long long stride = (long long)gridDim.x * kStageBlock;
    if (unit == 16) stage_body<uint4>(d + head, s + head, body, tid, stride);
    else if (unit == 8) stage_body<uint2>(d + head, s + head, body, tid, stride);
    else stage_body<unsigned>(d + head, s + head, body, tid, stride);
    const long long hw = head >> 2, tw = (n - tail0) >> 2;    // 4-byte words in front of and behind the body: at most 3 each
    for (long long w = tid; w < hw + tw; w += stride) {
        const long long off = w < hw ? (w << 2) : tail0 + ((w - hw) << 2);
        *reinterpret_cast<unsigned*>(d + off) = *reinterpret_cast<const unsigned*>(s + off);
    }
}

}  // namespace

extern "C" int dlrm_stage_inputs(int n_seg, void* const* dst_host, const void* const* src_host, const int64_t* bytes_host, void* stream) {
    if (n_seg < 0 || (n_seg > 0 && (!dst_host || !src_host || !bytes_host))) return DLRM_E_ARG;
    for (int i = 0; i < n_seg; ++i) {
        if (!dst_host[i] || !src_host[i] || bytes_host[i] < 0) return DLRM_E_ARG;
        if ((((uintptr_t)dst_host[i]) | ((uintptr_t)src_host[i]) | (uintptr_t)bytes_host[i]) & 3u) return DLRM_E_ALIGN;
    }
    int i = 0;
    while (i < n_seg) {
        StageArgs a = {};
        int m = 0;
        long long widest = 0;
        // (segments that copy nothing — empty, or already in place — take no block)
        for (; i < n_seg && m < DLRM_MAX_STAGE_SEGS; ++i) {
            if (bytes_host[i] == 0 || dst_host[i] == src_host[i]) continue;
            a.dst[m] = (char*)dst_host[i]; a.src[m] = (const char*)src_host[i]; a.bytes[m] = bytes_host[i];
            if (bytes_host[i] > widest) widest = bytes_host[i];
            ++m;
        }
        if (m == 0) break;
        long long nbx = (widest / 16 + kStageBlock - 1) / kStageBlock;
        if (nbx < 1) nbx = 1;
        if (nbx > kStageMaxBlocksX) nbx = kStageMaxBlocksX;
        hipLaunchKernelGGL(stage_inputs_kernel, dim3((unsigned)nbx, (unsigned)m), dim3(kStageBlock), 0, (hipStream_t)stream, a);
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int dlrm_forward_replay(int n_seg, void* const* dst_host, const void* const* src_host, const int64_t* bytes_host,
                                   int memcpy_max_segs, void* graph_exec, int sync_first, void* stream) {
    return dlrm_replay(n_seg, dst_host, src_host, bytes_host, memcpy_max_segs, 0, nullptr, nullptr, graph_exec, sync_first, stream);
}
