// emb_bf16.hip — embedding tables whose rows are stored in bfloat16: EmbeddingBag(sum) forward, and the fused backward + SGD /
// row-wise Adagrad update with ONE rounding per touched row per step (nearest-even or stochastic).
//
// Contracts (include/dlrm_hip.h):
//   forward : bit-identical to dlrm_emb_fwd on the same tables upcast to fp32 — a row element is widened by a 16-bit shift and accumulated
//             in index order per column, acc = fmaf(psw, v, acc) from +0.0.  The body of emb_lookup.h: a lane owns 16 bytes of a row (here 8
//             columns), D / 8 lanes own a bag (a wave reads 4 rows of D = 128 per load instruction), the first-row loads of U bags go back
//             to back, longer bags continue with a 4-deep load pipeline.  No LDS staging, no cross-lane reduction over rows.
//   update  : the walk of sorted_walk.h over bf16 rows — lookups sorted by (table, row) with the library's sorter, a lane group owns 64
//             consecutive sorted entries and sums each run of equal keys in input order IN FP32, runs that cross a group boundary go
//             through the edge buffers and the second pass; no atomics on the table.  The lane geometry is the fp32 kernel's (a lane owns
//             4 columns: 16 bytes of the fp32 gradient row, 8 bytes of the bf16 table row), so that g_r and the Adagrad accumulator have the
//             bits of dlrm_emb_bwd_rowwise_adagrad.  Each touched row is read once, stepped in fp32, rounded once and written once.
//   rounding: nearest = the compiler's fp32 -> bf16 conversion (IEEE round-to-nearest-even); stochastic = (bits(v) + u) >> 16 with u 16 bits
//             of Philox4x32-10 keyed by the call's seed, counter (row lo, row hi, column / 8, 0xB0000000 | table): a pure function of
//             (seed, table, row, column), hence independent of the launch shape and restatable on the host.
#include <stdlib.h>
#include "sorted_walk.h"

namespace {

typedef unsigned short bf16_bits;
typedef unsigned int bf_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) bf_u32x2 bf_gu32x2;
typedef __attribute__((address_space(1))) unsigned short bf_gu16;

// bf16 -> fp32 is exact: the 16 bits are the high half of the fp32 pattern
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }

__device__ __forceinline__ void fma8(float (&acc)[8], float w, const uint4& q) {
    acc[0] = __builtin_fmaf(w, bf_lo(q.x), acc[0]); acc[1] = __builtin_fmaf(w, bf_hi(q.x), acc[1]);
    acc[2] = __builtin_fmaf(w, bf_lo(q.y), acc[2]); acc[3] = __builtin_fmaf(w, bf_hi(q.y), acc[3]);
    acc[4] = __builtin_fmaf(w, bf_lo(q.z), acc[4]); acc[5] = __builtin_fmaf(w, bf_hi(q.z), acc[5]);
    acc[6] = __builtin_fmaf(w, bf_lo(q.w), acc[6]); acc[7] = __builtin_fmaf(w, bf_hi(q.w), acc[7]);
}

// -------------------------------------------------------------------------------------------
// forward, 16 bytes (8 columns) per lane: D % 8 == 0, D <= 512, 16-byte aligned tables and out
// -------------------------------------------------------------------------------------------
// emb_lookup.h's row source: 8 bf16 columns per 16-byte load
struct Bf16Rows {
    using Elem = bf16_bits;
    using Staged = uint4;
    using Acc = float[8];
    static constexpr int COLS = 8;
    static __device__ __forceinline__ long long pitch(int D) { return D; }
    static __device__ __forceinline__ void zero(Staged& v) { v = make_uint4(0u, 0u, 0u, 0u); }
    static __device__ __forceinline__ void clear(Acc& a) {
#pragma unroll
        for (int c = 0; c < 8; ++c) a[c] = 0.f;
    }
    static __device__ __forceinline__ void load(Staged& v, const bf16_bits* __restrict__ row, int, int col) { v = *(const uint4*)(row + col); }
    static __device__ __forceinline__ void accum(Acc& a, float w, const Staged& v) { fma8(a, w, v); }
    static __device__ __forceinline__ void store(float* o, const Acc& a) { store8(o, a); }
};

template <int LPB, typename IT, int U>
__global__ __launch_bounds__(256) void emb_fwd_bf16_kernel(EmbArgs a, long long B, int D, float* __restrict__ out, long long out_ld) {
    emb_lookup_body<Bf16Rows, LPB, 1, IT, U, false>(a, B, D, out, out_ld);
}

// forward, 2 bytes per lane: any D, any alignment.  One wavefront per bag, a lane walks its columns; correct, not fast.
template <typename IT>
__global__ __launch_bounds__(256) void emb_fwd_bf16_scalar_kernel(EmbArgs a, long long B, int D, float* __restrict__ out, long long out_ld) {
    if (a.pred.skip()) return;
    const int t = blockIdx.y;
    const bf16_bits* __restrict__ W = (const bf16_bits*)a.w[t];
    const IT* __restrict__ idx = (const IT*)a.idx[t];
    const IT* __restrict__ off = (const IT*)a.off[t];
    const float* __restrict__ psw = a.psw[t];
    const long long nnz = a.nnz[t], rows = a.rows[t];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + wave;
    if (b >= B) return;
    const long long s = (long long)off[b];
    const long long e = (b + 1 < B) ? (long long)off[b + 1] : nnz;
    float* o = out + b * out_ld + (long long)a.slot[t] * D;
    for (int d = lane; d < D; d += 64) {
        float acc = 0.f;
        for (long long i = s; i < e; ++i) {
            const long long r = (long long)idx[i];
            if (!dlrm_index_ok(r, rows)) { dlrm_report_bad_index(a.err, a.slot[t], r, rows); continue; }
            const float w = psw ? psw[i] : 1.f;
            acc = __builtin_fmaf(w, bf_lo((unsigned)W[r * D + d]), acc);
        }
        o[d] = acc;
    }
}

// -------------------------------------------------------------------------------------------
// rounding
// -------------------------------------------------------------------------------------------
// tbase: index of the launch group's first table in the caller's list.  key_dev != nullptr: the Philox key is READ FROM DEVICE MEMORY when the
// kernel runs (the *_devkey calls: what a captured HIP graph needs, as DlrmStep's `dev` is for the step size), else it is (k0, k1) by value.
struct RoundArgs { int stochastic; unsigned k0, k1; unsigned tbase; const unsigned long long* key_dev; };

// the call's rounding arguments with the key in registers: one uniform 8-byte load per workgroup when the key lives on the device
__device__ __forceinline__ RoundArgs round_args_now(RoundArgs ra) {
    if (ra.key_dev) {
        const unsigned long long k = *ra.key_dev;
        ra.k0 = (unsigned)(k & 0xFFFFFFFFull); ra.k1 = (unsigned)(k >> 32);
    }
    return ra;
}

__device__ __forceinline__ void philox4x32_10(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned (&out)[4]) {
    unsigned c[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}

__device__ __forceinline__ unsigned round_nearest(float v) {
    const __bf16 h = (__bf16)v;                      // the compiler's conversion: round-to-nearest-even
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}
// finite v: (bits + u) >> 16, a carry into the exponent gives the correct next value; Inf / NaN: truncated, a NaN stays a NaN
__device__ __forceinline__ unsigned round_stochastic(float v, unsigned u16) {
    const unsigned b = __float_as_uint(v);
    if ((b & 0x7F800000u) == 0x7F800000u) {
        unsigned h = b >> 16;
        if ((b & 0x007FFFFFu) != 0u && (h & 0x7Fu) == 0u) h |= 0x40u;
        return h;
    }
    return (b + u16) >> 16;
}

// One row's step + rounding + store.  Called by all LPB lanes of a lane group together (same control flow); `acc` = the lane's columns of
// the row's coalesced gradient.  ADA: the arithmetic of adagrad.hip's adagrad_apply with the row widened on load; the sum of squares is that kernel's (sorted_walk.h).
template <int VEC, int LPB, int NCH, bool ADA>
__device__ __forceinline__ void bf16_apply(bf16_bits* __restrict__ wrow, float* __restrict__ mom_r, int D, int lig,
                                           const typename Vec<VEC>::T (&acc)[NCH], float step, float eps, const RoundArgs& ra, unsigned table,
                                           long long row) {
    float denom = 1.f, m = 0.f;
    if constexpr (ADA) {
        const float sq = group_sum_sq<VEC, LPB, NCH>(acc, D, lig);
        m = *(const sc_gfloat*)mom_r + sq / (float)D;              // every lane reads the old value before lane 0 stores the new one
        denom = sqrtf(m) + eps;
    }
    const float f = ADA ? -step : step;                             // (SGD: the caller passes -lr)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int col = (c * LPB + lig) * VEC;
        if (col < D) {
            if constexpr (VEC == 4) {
                const bf_u32x2 raw = *(const bf_gu32x2*)(wrow + col);
                float w[4] = {bf_lo(raw.x), bf_hi(raw.x), bf_lo(raw.y), bf_hi(raw.y)};
                float g[4] = {acc[c].x, acc[c].y, acc[c].z, acc[c].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if constexpr (ADA) g[k] = g[k] / denom;
                    w[k] = __builtin_fmaf(f, g[k], w[k]);
                }
                unsigned h[4];
                if (ra.stochastic) {
                    unsigned r4[4];
                    philox4x32_10(ra.k0, ra.k1, (unsigned)row, (unsigned)((unsigned long long)row >> 32), (unsigned)col >> 3, 0xB0000000u | table, r4);
                    const unsigned ua = (col & 4) ? r4[2] : r4[0], ub = (col & 4) ? r4[3] : r4[1];
                    h[0] = round_stochastic(w[0], ua & 0xFFFFu); h[1] = round_stochastic(w[1], ua >> 16);
                    h[2] = round_stochastic(w[2], ub & 0xFFFFu); h[3] = round_stochastic(w[3], ub >> 16);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) h[k] = round_nearest(w[k]);
                }
                bf_u32x2 o;
                o.x = (h[0] & 0xFFFFu) | (h[1] << 16);
                o.y = (h[2] & 0xFFFFu) | (h[3] << 16);
                *(bf_gu32x2*)(wrow + col) = o;
            } else {
                float w = bf_lo((unsigned)*(const bf_gu16*)(wrow + col));
                float g = acc[c];
                if constexpr (ADA) g = g / denom;
                w = __builtin_fmaf(f, g, w);
                unsigned h;
                if (ra.stochastic) {
                    unsigned r4[4];
                    philox4x32_10(ra.k0, ra.k1, (unsigned)row, (unsigned)((unsigned long long)row >> 32), (unsigned)col >> 3, 0xB0000000u | table, r4);
                    const int wi = (col & 7) >> 1;
                    const unsigned word = wi == 0 ? r4[0] : wi == 1 ? r4[1] : wi == 2 ? r4[2] : r4[3];
                    h = round_stochastic(w, (col & 1) ? (word >> 16) : (word & 0xFFFFu));
                } else {
                    h = round_nearest(w);
                }
                *(bf_gu16*)(wrow + col) = (unsigned short)h;
            }
        }
    }
    if constexpr (ADA) { if (lig == 0) *(sc_gfloat*)mom_r = m; }
}

// -------------------------------------------------------------------------------------------
// the sorted walk (sorted_walk.h, pass 1 and pass 2) over bf16 rows
// -------------------------------------------------------------------------------------------
constexpr int kC = 2;           // gradient rows in flight per lane group (the fp32 walk's default)

struct StateArgs { float* state[DLRM_MAX_TABLES_PER_LAUNCH]; };

// the walk's row-update policy: SGD (ADA = false; step = -lr, no state) or row-wise Adagrad on the bf16 row `row` of table t
template <bool ADA>
struct Bf16Update {
    float step, eps;
    RoundArgs ra;
    template <int VEC, int LPB, int NCH>
    __device__ __forceinline__ void apply(float* w, float* state, int t, long long row, int D, int lig, const typename Vec<VEC>::T (&acc)[NCH]) const {
        bf16_apply<VEC, LPB, NCH, ADA>((bf16_bits*)w + row * D, ADA ? state + row : nullptr, D, lig, acc, step, eps, ra, ra.tbase + (unsigned)t, row);
    }
};

// Waves per SIMD the register allocator is held to (1: no request).  Over the shared body the D = 256 row-wise kernel with 64-bit sort keys
// came out at 81 VGPRs, one above the 80 of six waves per SIMD that it had as a separate kernel, and measured 4 % slower (1.04 -> 1.09 ms,
// profiles/emb_refactor/ab.md); held to six waves it takes 73, no scratch.  No other instantiation changes with the request.
template <int VEC, int LPB, int NCH, typename KT, bool ADA>
constexpr int kBf16GroupsMinWaves = (VEC == 4 && LPB == 64 && NCH == 1 && sizeof(KT) == 8 && ADA) ? 6 : 1;

template <int VEC, int LPB, int NCH, typename KT, bool ADA>
__global__ __launch_bounds__(256, (kBf16GroupsMinWaves<VEC, LPB, NCH, KT, ADA>)) void bf16_groups_kernel(SortedArgs sa, StateArgs aa, long long L, int D, int row_bits,
                                                          const KT* __restrict__ keys, const unsigned* __restrict__ vals,
                                                          const unsigned* __restrict__ bag_of,
                                                          const float* __restrict__ dout, long long dout_ld,
                                                          DlrmStep step_, float eps, RoundArgs ra_, float* __restrict__ edge_first,
                                                          float* __restrict__ edge_last) {
    const float step = step_;            // (by value, or read from the device scalar: common.h DlrmStep)
    const RoundArgs ra = round_args_now(ra_);
    WALK_STAGE_TABLES(sa, aa);
    walk_groups<VEC, LPB, NCH, KT, kC>(wt, L, D, row_bits, keys, vals, bag_of, dout, dout_ld, Bf16Update<ADA>{step, eps, ra}, edge_first,
                                       edge_last);
}

template <int VEC, int LPB, int NCH, typename KT, bool ADA>
__global__ __launch_bounds__(256) void bf16_fixup_kernel(SortedArgs sa, StateArgs aa, long long L, int D, int row_bits,
                                                         const KT* __restrict__ keys, DlrmStep step_, float eps, RoundArgs ra_,
                                                         const float* __restrict__ edge_first, const float* __restrict__ edge_last) {
    const float step = step_;
    const RoundArgs ra = round_args_now(ra_);
    walk_fixup<VEC, LPB, NCH, KT>(sa, aa.state, L, D, row_bits, keys, Bf16Update<ADA>{step, eps, ra}, edge_first, edge_last);
}

template <bool ADA>
static int bwd_bf16_impl(const char* what, int T, int64_t B, int D, void* const* weight_host, void* const* state_host,
                         const int64_t* rows_host, const void* const* indices_host, const void* const* offsets_host,
                         const int64_t* nnz_host, const void* const* psw_host, int idx_bits, const float* dout, int64_t dout_ld,
                         DlrmStep step, float eps, int rounding, uint64_t seed, const uint64_t* seed_dev, int table0, void* workspace,
                         int64_t workspace_bytes, int64_t* err, void* stream) {
    if (T <= 0 || B <= 0 || D <= 0 || !weight_host || (ADA && !state_host) || !rows_host || !indices_host || !offsets_host || !nnz_host ||
        !dout || dout_ld < (int64_t)T * D)
        return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    if (rounding != 0 && rounding != 1) return DLRM_E_MODE;
    if (table0 < 0 || (int64_t)table0 + T > 0x0FFFFFFF) return DLRM_E_RANGE;      // (the table id shares a counter word with the 0xB tag)
    hipStream_t st = (hipStream_t)stream;
    bool vec_ok = dlrm_aligned16(dout) && (dout_ld % 4 == 0);
    for (int t = 0; t < T; ++t) {
        if (!weight_host[t] || (ADA && !state_host[t]) || !offsets_host[t]) return DLRM_E_ARG;
        if (nnz_host[t] < 0 || rows_host[t] <= 0 || (nnz_host[t] > 0 && !indices_host[t])) return DLRM_E_ARG;
        if (((uintptr_t)weight_host[t]) & 1u) return DLRM_E_ALIGN;
        vec_ok = vec_ok && ((((uintptr_t)weight_host[t]) & 7u) == 0);
    }
    const WalkCall c{T, B, D, weight_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, idx_bits, dout, dout_ld,
                     workspace, workspace_bytes, err, st};
    return walk_update(what, c, vec_ok, [&](const auto& w, auto vec, auto lpb, auto nch) {
        using KT = typename std::decay_t<decltype(w)>::Key;
        constexpr int V = decltype(vec)::value, LP = decltype(lpb)::value, NC = decltype(nch)::value;
        StateArgs aa;
        for (int k = 0; k < DLRM_MAX_TABLES_PER_LAUNCH; ++k) aa.state[k] = ADA ? (float*)state_host[w.g->t0 + (k < w.g->n ? k : 0)] : nullptr;
        RoundArgs ra;
        ra.stochastic = rounding; ra.k0 = (unsigned)(seed & 0xFFFFFFFFull); ra.k1 = (unsigned)(seed >> 32); ra.tbase = (unsigned)(table0 + w.g->t0);
        ra.key_dev = (const unsigned long long*)seed_dev;
        hipLaunchKernelGGL((bf16_groups_kernel<V, LP, NC, KT, ADA>), w.grid, w.block, 0, st, w.sa, aa, (long long)w.g->L, D, w.g->row_bits, w.keys, w.vals,
                           w.bag_of, dout, (long long)dout_ld, step, eps, ra, w.edge_first, w.edge_last);
        DLRM_LAUNCH_CHECK();
        hipLaunchKernelGGL((bf16_fixup_kernel<V, LP, NC, KT, ADA>), w.grid, w.block, 0, st, w.sa, aa, (long long)w.g->L, D, w.g->row_bits, w.keys,
                           step, eps, ra, (const float*)w.edge_first, (const float*)w.edge_last);
        DLRM_LAUNCH_CHECK();
        return 0;
    });
}

}  // namespace

static int emb_fwd_bf16_impl(int T, int64_t B, int D, const void* const* weight_host, const int64_t* rows_host,
                            const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                            const void* const* psw_host, int idx_bits, float* out, int64_t out_ld, int64_t* err, DlrmPred pred, void* stream) {
    const int rc = emb_check_lists(T, B, D, weight_host, rows_host, indices_host, offsets_host, nnz_host, idx_bits);
    if (rc) return rc;
    if (!out || out_ld < (int64_t)T * D) return DLRM_E_ARG;
    bool fast = D % 8 == 0 && D <= 512 && dlrm_aligned16(out) && (out_ld % 4 == 0);
    for (int t = 0; t < T; ++t) {
        if (emb_check_table(t, weight_host, rows_host, indices_host, offsets_host, nnz_host)) return DLRM_E_ARG;
        if (((uintptr_t)weight_host[t]) & 1u) return DLRM_E_ALIGN;
        fast = fast && dlrm_aligned16(weight_host[t]);
    }
    hipStream_t st = (hipStream_t)stream;
    int lpb = 4;
    if (fast) lpb = lanes_per_bag(D / 8);
    constexpr int U = 2;             // bags per lane group (emb.hip's measured choice for the 4-rows-per-wave shape: the U = 2 figures there)
    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
        EmbArgs a;
        emb_fill_args(a, t0, n, weight_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, err, pred);
        dim3 block(256, 1, 1);
        if (!fast) {
            dim3 grid((unsigned)((B + 3) / 4), (unsigned)n, 1);
            if (idx_bits == 64) hipLaunchKernelGGL(emb_fwd_bf16_scalar_kernel<long long>, grid, block, 0, st, a, (long long)B, D, out, (long long)out_ld);
            else                hipLaunchKernelGGL(emb_fwd_bf16_scalar_kernel<int>, grid, block, 0, st, a, (long long)B, D, out, (long long)out_ld);
            DLRM_LAUNCH_CHECK();
            continue;
        }
        const int bpb = (256 / lpb) * U;
        dim3 grid((unsigned)((B + bpb - 1) / bpb), (unsigned)n, 1);
#define BF16_FWD(LP)                                                                                                                          \
    do {                                                                                                                                      \
        if (idx_bits == 64) hipLaunchKernelGGL((emb_fwd_bf16_kernel<LP, long long, U>), grid, block, 0, st, a, (long long)B, D, out, (long long)out_ld); \
        else                hipLaunchKernelGGL((emb_fwd_bf16_kernel<LP, int, U>), grid, block, 0, st, a, (long long)B, D, out, (long long)out_ld);       \
    } while (0)
        switch (lpb) {
            case 4: BF16_FWD(4); break;   case 8: BF16_FWD(8); break;   case 16: BF16_FWD(16); break;
            case 32: BF16_FWD(32); break; case 64: BF16_FWD(64); break;
            default: return DLRM_E_RANGE;
        }
#undef BF16_FWD
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int dlrm_emb_fwd_bf16(int T, int64_t B, int D, const void* const* weight_host, const int64_t* rows_host,
                                 const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                                 const void* const* psw_host, int idx_bits, float* out, int64_t out_ld, int64_t* err, void* stream) {
    return emb_fwd_bf16_impl(T, B, D, weight_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, idx_bits, out, out_ld, err,
                             DlrmPred{nullptr, 0}, stream);
}

// dlrm_emb_fwd_bf16 behind a launch predicate (common.h DlrmPred): the same kernels, whose workgroups return at once unless
// (*pred_flag != 0) == (pred_nonzero != 0)
extern "C" int dlrm_emb_fwd_bf16_pred(int T, int64_t B, int D, const void* const* weight_host, const int64_t* rows_host,
                                      const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                                      const void* const* psw_host, int idx_bits, float* out, int64_t out_ld, int64_t* err,
                                      const int32_t* pred_flag, int pred_nonzero, void* stream) {
    return emb_fwd_bf16_impl(T, B, D, weight_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, idx_bits, out, out_ld, err,
                             DlrmPred{(const int*)pred_flag, pred_nonzero}, stream);
}

extern "C" int64_t dlrm_emb_bwd_bf16_workspace_bytes(int T, int D, const int64_t* nnz_host, const int64_t* rows_host) {
    return walk_workspace_bytes(T, D, nnz_host, rows_host);
}

extern "C" int dlrm_emb_bwd_sgd_bf16(int T, int64_t B, int D, void* const* weight_host, const int64_t* rows_host,
                                     const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                                     const void* const* psw_host, int idx_bits, const float* dout, int64_t dout_ld, float lr,
                                     const float* lr_dev, int rounding, uint64_t seed, int table0, void* workspace, int64_t workspace_bytes,
                                     int64_t* err, void* stream) {
    return bwd_bf16_impl<false>("dlrm_emb_bwd_sgd_bf16", T, B, D, weight_host, nullptr, rows_host, indices_host, offsets_host, nnz_host, psw_host,
                                idx_bits, dout, dout_ld, dlrm_step_neg(lr, lr_dev), 0.f, rounding, seed, nullptr, table0, workspace, workspace_bytes,
                                err, stream);
}

extern "C" int dlrm_emb_bwd_rowwise_adagrad_bf16(int T, int64_t B, int D, void* const* weight_host, void* const* state_host,
                                                 const int64_t* rows_host, const void* const* indices_host,
                                                 const void* const* offsets_host, const int64_t* nnz_host, const void* const* psw_host,
                                                 int idx_bits, const float* dout, int64_t dout_ld, float lr, const float* lr_dev, float eps,
                                                 int rounding, uint64_t seed, int table0, void* workspace, int64_t workspace_bytes,
                                                 int64_t* err, void* stream) {
    return bwd_bf16_impl<true>("dlrm_emb_bwd_rowwise_adagrad_bf16", T, B, D, weight_host, state_host, rows_host, indices_host, offsets_host,
                               nnz_host, psw_host, idx_bits, dout, dout_ld, dlrm_step_pos(lr, lr_dev), eps, rounding, seed, nullptr, table0,
                               workspace, workspace_bytes, err, stream);
}

// The two update calls with the Philox key READ FROM DEVICE MEMORY when the kernels run (seed_dev: 8-byte aligned device uint64): the same
// kernels, the same bits as the by-value calls given the same key.  What a captured whole-step graph takes: dlrm_philox_key_next writes a
// fresh key in front of every replayed update.
extern "C" int dlrm_emb_bwd_sgd_bf16_devkey(int T, int64_t B, int D, void* const* weight_host, const int64_t* rows_host,
                                            const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                                            const void* const* psw_host, int idx_bits, const float* dout, int64_t dout_ld, float lr,
                                            const float* lr_dev, int rounding, const uint64_t* seed_dev, int table0, void* workspace,
                                            int64_t workspace_bytes, int64_t* err, void* stream) {
    if (!seed_dev) return DLRM_E_ARG;
    if (((uintptr_t)seed_dev) & 7u) return DLRM_E_ALIGN;
    return bwd_bf16_impl<false>("dlrm_emb_bwd_sgd_bf16_devkey", T, B, D, weight_host, nullptr, rows_host, indices_host, offsets_host, nnz_host,
                                psw_host, idx_bits, dout, dout_ld, dlrm_step_neg(lr, lr_dev), 0.f, rounding, 0, seed_dev, table0, workspace,
                                workspace_bytes, err, stream);
}

extern "C" int dlrm_emb_bwd_rowwise_adagrad_bf16_devkey(int T, int64_t B, int D, void* const* weight_host, void* const* state_host,
                                                        const int64_t* rows_host, const void* const* indices_host,
                                                        const void* const* offsets_host, const int64_t* nnz_host,
                                                        const void* const* psw_host, int idx_bits, const float* dout, int64_t dout_ld,
                                                        float lr, const float* lr_dev, float eps, int rounding, const uint64_t* seed_dev,
                                                        int table0, void* workspace, int64_t workspace_bytes, int64_t* err, void* stream) {
    if (!seed_dev) return DLRM_E_ARG;
    if (((uintptr_t)seed_dev) & 7u) return DLRM_E_ALIGN;
    return bwd_bf16_impl<true>("dlrm_emb_bwd_rowwise_adagrad_bf16_devkey", T, B, D, weight_host, state_host, rows_host, indices_host,
                               offsets_host, nnz_host, psw_host, idx_bits, dout, dout_ld, dlrm_step_pos(lr, lr_dev), eps, rounding, 0, seed_dev,
                               table0, workspace, workspace_bytes, err, stream);
}

namespace {
// one lane: key = mix(seed0, calls), calls += 1 (the mix of dlrm_net._mix_seed(seed0, call_no, 0): wrap-around 64-bit arithmetic)
__global__ __launch_bounds__(64) void philox_key_next_kernel(unsigned long long seed0, unsigned long long* __restrict__ calls,
                                                             unsigned long long* __restrict__ key) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long n = *calls;
    unsigned long long z = seed0 * 0x9E3779B97F4A7C15ull + n * 0xBF58476D1CE4E5B9ull;
    z ^= z >> 31;
    *key = z;
    *calls = n + 1ull;
}
}  // namespace

// The per-update Philox key of a model, advanced ON THE DEVICE: *key_dev = mix(seed0, *calls_dev), then *calls_dev += 1.  One launch of one
// workgroup; allocates nothing and synchronises nothing (capturable).  calls_dev, key_dev: distinct 8-byte aligned device uint64.
extern "C" int dlrm_philox_key_next(uint64_t seed0, uint64_t* calls_dev, uint64_t* key_dev, void* stream) {
    if (!calls_dev || !key_dev || calls_dev == key_dev) return DLRM_E_ARG;
    if ((((uintptr_t)calls_dev) | ((uintptr_t)key_dev)) & 7u) return DLRM_E_ALIGN;
    hipLaunchKernelGGL(philox_key_next_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long)seed0,
                       (unsigned long long*)calls_dev, (unsigned long long*)key_dev);
    DLRM_LAUNCH_CHECK();
    return 0;
}
