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

// One segment's copy, by every thread of the blocks that stride it (tid of stride).  Every pointer and length is a multiple of 4 (checked on
// the host).  The widest element both pointers admit TOGETHER is the body's: 16 bytes when destination and source are congruent modulo 16, 8
// when modulo 8, else 4; up to three 4-byte words in front bring the destination (and with it the source) to that boundary, up to three behind
// finish the segment.  Segments are tiny (n * 8 bytes for an id row at n = 1 is ONE word): nothing here assumes a full block of work, a thread
// with nothing to do falls through.  No LDS, no atomics; plain vector loads and stores.
__device__ __forceinline__ void stage_copy(char* __restrict__ d, const char* __restrict__ s, long long n, long long tid, long long stride) {
    if (n <= 0) return;
    const unsigned rel = (unsigned)(((uintptr_t)d ^ (uintptr_t)s) & 15u);
    const int unit = rel == 0u ? 16 : ((rel & 7u) == 0u ? 8 : 4);
    long long head = (long long)((unit - (int)((uintptr_t)d & (uintptr_t)(unit - 1))) & (unit - 1));
    if (head > n) head = n;
    const long long body = (n - head) / unit;                 // elements of `unit` bytes
    const long long tail0 = head + body * unit;               // first byte behind the body
    if (unit == 16) stage_body<uint4>(d + head, s + head, body, tid, stride);
    else if (unit == 8) stage_body<uint2>(d + head, s + head, body, tid, stride);
    else stage_body<unsigned>(d + head, s + head, body, tid, stride);
    const long long hw = head >> 2, tw = (n - tail0) >> 2;    // 4-byte words in front of and behind the body: at most 3 each
    for (long long w = tid; w < hw + tw; w += stride) {
        const long long off = w < hw ? (w << 2) : tail0 + ((w - hw) << 2);
        *reinterpret_cast<unsigned*>(d + off) = *reinterpret_cast<const unsigned*>(s + off);
    }
}

// blockIdx.y = segment, blockIdx.x strides its bytes.
__global__ __launch_bounds__(kStageBlock) void stage_inputs_kernel(StageArgs a) {
    const int seg = blockIdx.y;
    stage_copy(a.dst[seg], a.src[seg], a.bytes[seg], (long long)blockIdx.x * kStageBlock + threadIdx.x, (long long)gridDim.x * kStageBlock);
}

// ---- a ragged multi-hot request into a ragged bucket (graph_forward.py: "Ragged buckets") --------------------------------------------------
// The bucket's lookups were captured with nnz = cap baked into their kernargs, so a request of nnz <= cap ids sits at the END of the static
// ids buffer: shift = cap - nnz, ids_static[shift .. cap) = the request's ids (a copy segment whose destination is base + shift * elem: any
// relative alignment modulo 16, which stage_copy's unit selection covers), and the static offsets become
//     off_static[b] = b < n ? shift + min(max(off_req[b], 0), nnz) : cap          for ALL b < bucket, on every request.
// Real bags keep their ids in order, the last real bag ends at off_static[n] = cap (or at the baked nnz = cap when n == bucket), tail bags
// are empty; what lies in front of off_static[0] is never pooled.  The clamp changes nothing for well-formed offsets and keeps the captured
// lookups inside [shift, cap) for any others.
#define DLRM_MAX_RAGGED_SEGS 64
struct RaggedArgs {                     // 64 x 32 B + 24 B = 2072 B; .kernarg_segment_size 2328 with the hidden arguments (a launch takes 4 KiB)
    char*       dst[DLRM_MAX_RAGGED_SEGS];
    const char* src[DLRM_MAX_RAGGED_SEGS];
    long long   len[DLRM_MAX_RAGGED_SEGS];      // copy: bytes.  offsets: nnz
    long long   cap[DLRM_MAX_RAGGED_SEGS];      // copy: -1.     offsets: cap (>= 0)
    long long   n, bucket;                      // bags of the request, bags of the bucket: the same for every offsets segment
    int         elem;                           // bytes of an offset: 4 or 8
};

// the 4-byte word w of the static offsets: element w (int32) or half w & 1 of element w >> 1 (int64, little endian).  Sources are read as
// 4-byte words too, so an int64 offsets tensor needs no more than the 4-byte alignment the host checks.
template <int ELEM>
__device__ __forceinline__ unsigned ragged_offset_word(const unsigned* __restrict__ s, long long w, long long n, long long shift, long long nnz,
                                                       long long cap) {
    const long long b = ELEM == 8 ? (w >> 1) : w;
    long long v = cap;
    if (b < n) {
        long long o;
        if (ELEM == 8) o = (long long)(((unsigned long long)s[2 * b + 1] << 32) | (unsigned long long)s[2 * b]);
        else o = (long long)(int)s[b];
        o = o < 0 ? 0 : (o > nnz ? nnz : o);
        v = shift + o;
    }
    return (ELEM == 8 && (w & 1)) ? (unsigned)((unsigned long long)v >> 32) : (unsigned)v;
}

// all `bucket` offsets of one static tensor: 16-byte stores from the destination's first 16-byte boundary on, single words in front and behind
template <int ELEM>
__device__ __forceinline__ void ragged_offsets(char* __restrict__ d, const char* __restrict__ s, long long n, long long bucket, long long nnz,
                                               long long cap, long long tid, long long stride) {
    const unsigned* __restrict__ sw = reinterpret_cast<const unsigned*>(s);
    unsigned* __restrict__ dw = reinterpret_cast<unsigned*>(d);
    const long long shift = cap - nnz;
    const long long words = bucket * (ELEM / 4);
    long long head = (long long)(((16u - (unsigned)((uintptr_t)d & 15u)) & 15u) >> 2);
    if (head > words) head = words;
    const long long quads = (words - head) >> 2;
    const long long tail0 = head + (quads << 2);
    for (long long q = tid; q < quads; q += stride) {
        const long long w = head + (q << 2);
        uint4 v;
        v.x = ragged_offset_word<ELEM>(sw, w, n, shift, nnz, cap);
        v.y = ragged_offset_word<ELEM>(sw, w + 1, n, shift, nnz, cap);
        v.z = ragged_offset_word<ELEM>(sw, w + 2, n, shift, nnz, cap);
        v.w = ragged_offset_word<ELEM>(sw, w + 3, n, shift, nnz, cap);
        *reinterpret_cast<uint4*>(dw + w) = v;
    }
    const long long tw = words - tail0;
    for (long long k = tid; k < head + tw; k += stride) {
        const long long w = k < head ? k : tail0 + (k - head);
        dw[w] = ragged_offset_word<ELEM>(sw, w, n, shift, nnz, cap);
    }
}

// blockIdx.y = segment (a block-uniform index into the kernarg's tables: scalar loads, no scratch), blockIdx.x strides it
__global__ __launch_bounds__(kStageBlock) void stage_ragged_kernel(RaggedArgs a) {
    const int seg = blockIdx.y;
    char* __restrict__ d = a.dst[seg];
    const char* __restrict__ s = a.src[seg];
    const long long len = a.len[seg], cap = a.cap[seg];
    const long long tid = (long long)blockIdx.x * kStageBlock + threadIdx.x;
    const long long stride = (long long)gridDim.x * kStageBlock;
    if (cap < 0) stage_copy(d, s, len, tid, stride);
    else if (a.elem == 8) ragged_offsets<8>(d, s, a.n, a.bucket, len, cap, tid, stride);
    else ragged_offsets<4>(d, s, a.n, a.bucket, len, cap, tid, stride);
}

// every check of a ragged request, before anything touches the device
int ragged_check(void* x_dst, const void* x_src, int64_t x_bytes, int n_ids, void* const* ids_dst_host, const void* const* ids_src_host,
                 const int64_t* ids_nnz_host, const int64_t* ids_cap_host, int n_off, void* const* off_dst_host,
                 const void* const* off_src_host, const int64_t* off_nnz_host, const int64_t* off_cap_host, int64_t n, int64_t bucket,
                 int idx_bytes) {
    if (idx_bytes != 4 && idx_bytes != 8) return DLRM_E_ARG;
    if (n < 0 || bucket < 1 || n > bucket || x_bytes < 0 || n_ids < 0 || n_off < 0) return DLRM_E_ARG;
    if (x_bytes > 0 && (!x_dst || !x_src)) return DLRM_E_ARG;
    if (n_ids > 0 && (!ids_dst_host || !ids_src_host || !ids_nnz_host || !ids_cap_host)) return DLRM_E_ARG;
    if (n_off > 0 && (!off_dst_host || !off_src_host || !off_nnz_host || !off_cap_host)) return DLRM_E_ARG;
    const int64_t cap_max = idx_bytes == 4 ? (int64_t)INT_MAX : (int64_t)1 << 48;      // (a static offset holds cap itself)
    for (int i = 0; i < n_ids; ++i) {
        if (ids_nnz_host[i] < 0 || ids_nnz_host[i] > ids_cap_host[i] || ids_cap_host[i] > cap_max || !ids_dst_host[i]) return DLRM_E_ARG;
        if (ids_nnz_host[i] > 0 && !ids_src_host[i]) return DLRM_E_ARG;      // (nothing to copy: the source may be null)
    }
    for (int i = 0; i < n_off; ++i) {
        if (off_nnz_host[i] < 0 || off_nnz_host[i] > off_cap_host[i] || off_cap_host[i] > cap_max || !off_dst_host[i]) return DLRM_E_ARG;
        if (n > 0 && !off_src_host[i]) return DLRM_E_ARG;
    }
    if ((((uintptr_t)x_dst) | ((uintptr_t)x_src) | (uintptr_t)x_bytes) & 3u) return DLRM_E_ALIGN;
    for (int i = 0; i < n_ids; ++i)
        if ((((uintptr_t)ids_dst_host[i]) | ((uintptr_t)ids_src_host[i])) & 3u) return DLRM_E_ALIGN;
    for (int i = 0; i < n_off; ++i)
        if ((((uintptr_t)off_dst_host[i]) | ((uintptr_t)off_src_host[i])) & 3u) return DLRM_E_ALIGN;
    return 0;
}

struct RaggedBatch {                    // the segments of one launch, collected on the host
    RaggedArgs a;
    int m;
    long long widest;                   // bytes of the longest segment
};

int ragged_flush(RaggedBatch& r, hipStream_t st) {
    if (r.m == 0) return 0;
    long long nbx = (r.widest / 16 + kStageBlock - 1) / kStageBlock;
    if (nbx < 1) nbx = 1;
    if (nbx > kStageMaxBlocksX) nbx = kStageMaxBlocksX;
    hipLaunchKernelGGL(stage_ragged_kernel, dim3((unsigned)nbx, (unsigned)r.m), dim3(kStageBlock), 0, st, r.a);
    DLRM_LAUNCH_CHECK();
    r.m = 0;
    r.widest = 0;
    return 0;
}

int ragged_push(RaggedBatch& r, hipStream_t st, void* dst, const void* src, long long len, long long cap, long long bytes) {
    if (r.m == DLRM_MAX_RAGGED_SEGS) {
        const int rc = ragged_flush(r, st);
        if (rc) return rc;
    }
    r.a.dst[r.m] = (char*)dst; r.a.src[r.m] = (const char*)src; r.a.len[r.m] = len; r.a.cap[r.m] = cap;
    if (bytes > r.widest) r.widest = bytes;
    ++r.m;
    return 0;
}

// the launches of a checked request: X, then the ids at the END of their buffers, then every offsets tensor in full
int ragged_launch(void* x_dst, const void* x_src, int64_t x_bytes, int n_ids, void* const* ids_dst_host, const void* const* ids_src_host,
                  const int64_t* ids_nnz_host, const int64_t* ids_cap_host, int n_off, void* const* off_dst_host,
                  const void* const* off_src_host, const int64_t* off_nnz_host, const int64_t* off_cap_host, int64_t n, int64_t bucket,
                  int idx_bytes, hipStream_t st) {
    RaggedBatch r = {};
    r.a.n = n; r.a.bucket = bucket; r.a.elem = idx_bytes;
    int rc = 0;
    // (segments that copy nothing — empty, or already in place — take no block)
    if (x_bytes > 0 && x_dst != x_src) rc = ragged_push(r, st, x_dst, x_src, x_bytes, -1, x_bytes);
    for (int i = 0; i < n_ids && !rc; ++i) {
        const long long bytes = ids_nnz_host[i] * idx_bytes;
        char* d = (char*)ids_dst_host[i] + (ids_cap_host[i] - ids_nnz_host[i]) * idx_bytes;
        if (bytes > 0 && (const void*)d != ids_src_host[i]) rc = ragged_push(r, st, d, ids_src_host[i], bytes, -1, bytes);
    }
    for (int i = 0; i < n_off && !rc; ++i)
        rc = ragged_push(r, st, off_dst_host[i], off_src_host[i], off_nnz_host[i], off_cap_host[i], bucket * idx_bytes);
    return rc ? rc : ragged_flush(r, st);
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

extern "C" int dlrm_stage_ragged(void* x_dst, const void* x_src, int64_t x_bytes, int n_ids, void* const* ids_dst_host,
                                 const void* const* ids_src_host, const int64_t* ids_nnz_host, const int64_t* ids_cap_host, int n_off,
                                 void* const* off_dst_host, const void* const* off_src_host, const int64_t* off_nnz_host,
                                 const int64_t* off_cap_host, int64_t n, int64_t bucket, int idx_bytes, void* stream) {
    const int rc = ragged_check(x_dst, x_src, x_bytes, n_ids, ids_dst_host, ids_src_host, ids_nnz_host, ids_cap_host, n_off, off_dst_host,
                                off_src_host, off_nnz_host, off_cap_host, n, bucket, idx_bytes);
    if (rc) return rc;
    return ragged_launch(x_dst, x_src, x_bytes, n_ids, ids_dst_host, ids_src_host, ids_nnz_host, ids_cap_host, n_off, off_dst_host,
                         off_src_host, off_nnz_host, off_cap_host, n, bucket, idx_bytes, (hipStream_t)stream);
}

// the protocol of replay.h with the ragged staging as its step 3: check, wait, stage, launch — one host call per request
extern "C" int dlrm_forward_replay_ragged(void* x_dst, const void* x_src, int64_t x_bytes, int n_ids, void* const* ids_dst_host,
                                          const void* const* ids_src_host, const int64_t* ids_nnz_host, const int64_t* ids_cap_host,
                                          int n_off, void* const* off_dst_host, const void* const* off_src_host,
                                          const int64_t* off_nnz_host, const int64_t* off_cap_host, int64_t n, int64_t bucket,
                                          int idx_bytes, void* graph_exec, int sync_first, void* stream) {
    if (!graph_exec) return DLRM_E_ARG;
    int rc = ragged_check(x_dst, x_src, x_bytes, n_ids, ids_dst_host, ids_src_host, ids_nnz_host, ids_cap_host, n_off, off_dst_host,
                          off_src_host, off_nnz_host, off_cap_host, n, bucket, idx_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (sync_first) {
        const hipError_t e = dlrm_stream_wait_polling(st);
        if (e != hipSuccess) return (int)e;
    }
    rc = ragged_launch(x_dst, x_src, x_bytes, n_ids, ids_dst_host, ids_src_host, ids_nnz_host, ids_cap_host, n_off, off_dst_host,
                       off_src_host, off_nnz_host, off_cap_host, n, bucket, idx_bytes, st);
    if (rc) return rc;
    const hipError_t e = hipGraphLaunch((hipGraphExec_t)graph_exec, st);
    return e == hipSuccess ? 0 : (int)e;
}
