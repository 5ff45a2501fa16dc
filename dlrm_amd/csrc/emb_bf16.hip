// emb_bf16.hip — embedding tables whose rows are stored in bfloat16: EmbeddingBag(sum) forward, and the fused backward + SGD /
// row-wise Adagrad update with ONE rounding per touched row per step (nearest-even or stochastic).
//
// Contracts (include/dlrm_hip.h):
//   forward : bit-identical to dlrm_emb_fwd on the same tables upcast to fp32 — a row element is widened by a 16-bit shift and accumulated
//             in index order per column, acc = fmaf(psw, v, acc) from +0.0.  Structure of emb.hip: a lane owns 16 bytes of a row (here 8
//             columns), D / 8 lanes own a bag (a wave reads 4 rows of D = 128 per load instruction), the first-row loads of U bags go back
//             to back, longer bags continue with a 4-deep load pipeline.  No LDS staging, no cross-lane reduction over rows.
//   update  : the walk of adagrad.hip over bf16 rows — lookups sorted by (table, row) with the library's sorter, a lane group owns 64
//             consecutive sorted entries and sums each run of equal keys in input order IN FP32, runs that cross a group boundary go
//             through the edge buffers and the second pass; no atomics on the table.  The lane geometry is the fp32 kernel's (a lane owns
//             4 columns: 16 bytes of the fp32 gradient row, 8 bytes of the bf16 table row), so that g_r and the Adagrad accumulator have the
//             bits of dlrm_emb_bwd_rowwise_adagrad.  Each touched row is read once, stepped in fp32, rounded once and written once.
//   rounding: nearest = the compiler's fp32 -> bf16 conversion (IEEE round-to-nearest-even); stochastic = (bits(v) + u) >> 16 with u 16 bits
//             of Philox4x32-10 keyed by the call's seed, counter (row lo, row hi, column / 8, 0xB0000000 | table): a pure function of
//             (seed, table, row, column), hence independent of the launch shape and restatable on the host.
#include <stdlib.h>
#include "sorted_common.h"

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
template <int LPB, typename IT, int U>
__global__ __launch_bounds__(256) void emb_fwd_bf16_kernel(EmbArgs a, long long B, int D, float* __restrict__ out, long long out_ld) {
    if (a.pred.skip()) return;          // dlrm_emb_fwd_bf16_pred (flag == nullptr: always run)
    const int t = blockIdx.y;
    const bf16_bits* __restrict__ W = (const bf16_bits*)a.w[t];
    const IT* __restrict__ idx = (const IT*)a.idx[t];
    const IT* __restrict__ off = (const IT*)a.off[t];
    const float* __restrict__ psw = a.psw[t];
    const long long nnz = a.nnz[t];
    const long long rows = a.rows[t];

    constexpr int GPB = 256 / LPB;  // groups (bags in flight) per workgroup
    const int g = threadIdx.x / LPB;
    const int lig = threadIdx.x % LPB;
    const int col = lig * 8;
    const bool live = col < D;
    const long long b0 = ((long long)blockIdx.x * GPB + g) * U;
    if (b0 >= B) return;

    long long s[U], e[U];
    {
        long long o[U + 1];
#pragma unroll
        for (int u = 0; u <= U; ++u) {
            const long long b = b0 + u;
            o[u] = (b < B) ? (long long)off[b] : nnz;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { s[u] = o[u]; e[u] = (b0 + u < B) ? o[u + 1] : o[u]; }
    }

    float acc[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[u][c] = 0.f;

    // ---- phase 1: first row of every bag, all loads in flight together
    long long r0[U];
    float w0[U];
    bool ok0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        r0[u] = 0; w0[u] = 1.f; ok0[u] = false;
        if (s[u] < e[u]) {
            r0[u] = (long long)idx[s[u]];
            if (psw) w0[u] = psw[s[u]];
            ok0[u] = dlrm_index_ok(r0[u], rows);
            if (!ok0[u]) dlrm_report_bad_index(a.err, a.slot[t], r0[u], rows);
        }
    }
    uint4 v0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        v0[u] = make_uint4(0u, 0u, 0u, 0u);
        if (ok0[u] && live) v0[u] = *(const uint4*)(W + r0[u] * D + col);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (ok0[u]) fma8(acc[u], w0[u], v0[u]);

    // ---- phase 2: remaining rows of multi-hot bags, 4 row loads in flight per bag
#pragma unroll
    for (int u = 0; u < U; ++u) {
        long long i = s[u] + 1;
        const long long end = e[u];
        for (; i + 4 <= end; i += 4) {
            long long r[4]; float w[4]; uint4 v[4];
            bool ok[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r[k] = (long long)idx[i + k]; w[k] = psw ? psw[i + k] : 1.f;
                ok[k] = dlrm_index_ok(r[k], rows);
                if (!ok[k]) dlrm_report_bad_index(a.err, a.slot[t], r[k], rows);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = make_uint4(0u, 0u, 0u, 0u);
                if (ok[k] && live) v[k] = *(const uint4*)(W + r[k] * D + col);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) fma8(acc[u], w[k], v[k]);
        }
        for (; i < end; ++i) {
            const long long r = (long long)idx[i];
            const float w = psw ? psw[i] : 1.f;
            if (!dlrm_index_ok(r, rows)) { dlrm_report_bad_index(a.err, a.slot[t], r, rows); continue; }
            if (live) { const uint4 v = *(const uint4*)(W + r * D + col); fma8(acc[u], w, v); }
        }
    }

    // ---- store: bag b of table t goes to out[b, slot*D : +D]
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const long long b = b0 + u;
        if (b < B && live) {
            float* o = out + b * out_ld + (long long)a.slot[t] * D + col;
            *(float4*)(o) = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
            *(float4*)(o + 4) = make_float4(acc[u][4], acc[u][5], acc[u][6], acc[u][7]);
        }
    }
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
struct RoundArgs { int stochastic; unsigned k0, k1; unsigned tbase; };   // tbase: index of the launch group's first table in the caller's list

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
// the row's coalesced gradient.  ADA: the arithmetic of adagrad.hip's adagrad_apply, statement for statement, with the row widened on load.
template <int VEC, int LPB, int NCH, bool ADA>
__device__ __forceinline__ void bf16_apply(bf16_bits* __restrict__ wrow, float* __restrict__ mom_r, int D, int lig,
                                           const typename Vec<VEC>::T (&acc)[NCH], float step, float eps, const RoundArgs& ra, unsigned table,
                                           long long row) {
    float denom = 1.f, m = 0.f;
    if constexpr (ADA) {
        float sq = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int col = (c * LPB + lig) * VEC;
            // The products and sums of adagrad.hip's v_sq, with the roundings SPELLED OUT.  That file leaves fusing a multiply into the next
            // add to the compiler, which decides per inlined copy; its compiled vector kernels (D % 4 == 0) round every square and every
            // sum separately and its one-column kernels chain fmaf(v, v, sq) — restated here with intrinsics the compiler may not re-associate
            // or contract, so that the accumulator has that library's bits whatever the surrounding code looks like.
            if constexpr (VEC == 4) {
                if (col < D)
                    sq = __fadd_rn(sq, __fadd_rn(__fadd_rn(__fmul_rn(acc[c].x, acc[c].x), __fmul_rn(acc[c].y, acc[c].y)),
                                                 __fadd_rn(__fmul_rn(acc[c].z, acc[c].z), __fmul_rn(acc[c].w, acc[c].w))));
            } else {
                if (col < D) sq = __builtin_fmaf(acc[c], acc[c], sq);
            }
        }
#pragma unroll
        for (int o = LPB >> 1; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
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
// the sorted walk (adagrad.hip, pass 1 and pass 2) over bf16 rows
// -------------------------------------------------------------------------------------------
constexpr int kG = 64;          // sorted entries per lane group
constexpr int kC = 2;           // gradient rows in flight per lane group (adagrad.hip's default)

struct StateArgs { float* state[DLRM_MAX_TABLES_PER_LAUNCH]; };

__device__ __forceinline__ float4 v_add(const float4& a, const float4& b) {
    return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float v_add(const float& a, const float& b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float4 v_scale(float s, const float4& v) {
    return make_float4(__fmul_rn(s, v.x), __fmul_rn(s, v.y), __fmul_rn(s, v.z), __fmul_rn(s, v.w));
}
__device__ __forceinline__ float v_scale(float s, const float& v) { return __fmul_rn(s, v); }

template <typename T> __device__ __forceinline__ T group_bcast(T v, int src_lane);
template <> __device__ __forceinline__ unsigned group_bcast<unsigned>(unsigned v, int src_lane) { return (unsigned)__shfl((int)v, src_lane, 64); }
template <> __device__ __forceinline__ unsigned long long group_bcast<unsigned long long>(unsigned long long v, int src_lane) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src_lane, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src_lane, 64);
    return ((unsigned long long)hi << 32) | lo;
}
template <> __device__ __forceinline__ float group_bcast<float>(float v, int src_lane) { return __shfl(v, src_lane, 64); }

template <int VEC, int LPB, int NCH, typename KT, bool ADA>
__global__ __launch_bounds__(256) void bf16_groups_kernel(SortedArgs sa, StateArgs aa, long long L, int D, int row_bits,
                                                          const KT* __restrict__ keys, const unsigned* __restrict__ vals,
                                                          const unsigned* __restrict__ bag_of,
                                                          const float* __restrict__ dout, long long dout_ld,
                                                          DlrmStep step_, float eps, RoundArgs ra, float* __restrict__ edge_first,
                                                          float* __restrict__ edge_last) {
    const float step = step_;            // (by value, or read from the device scalar: common.h DlrmStep)
    using VT = typename Vec<VEC>::T;
    constexpr int DP = NCH * LPB * VEC;                  // padded row length of the edge buffers
    constexpr int GPB = 256 / LPB;
    constexpr int NS = kG / LPB;                         // entries a lane resolves for its group (LPB is a power of two <= 64)
    static_assert(kG % LPB == 0 && LPB % kC == 0, "group geometry");
    // per-table arguments are indexed by a lane-dependent table id: staged in LDS (adagrad.hip)
    __shared__ long long s_w[DLRM_MAX_TABLES_PER_LAUNCH], s_state[DLRM_MAX_TABLES_PER_LAUNCH], s_psw[DLRM_MAX_TABLES_PER_LAUNCH],
        s_base[DLRM_MAX_TABLES_PER_LAUNCH];
    __shared__ int s_slot[DLRM_MAX_TABLES_PER_LAUNCH];
#pragma unroll
    for (int k = 0; k < DLRM_MAX_TABLES_PER_LAUNCH; ++k)
        if (threadIdx.x == k) {
            s_w[k] = (long long)sa.w[k]; s_state[k] = (long long)aa.state[k]; s_psw[k] = (long long)sa.psw[k]; s_base[k] = sa.base[k];
            s_slot[k] = sa.slot[k];
        }
    __syncthreads();
    const int g = threadIdx.x / LPB, lig = threadIdx.x % LPB;
    const int lane0 = (threadIdx.x & 63) & ~(LPB - 1);   // first lane of this group inside its wave
    const long long grp = (long long)blockIdx.x * GPB + g;
    const long long g0 = grp * kG;
    if (g0 >= L) return;
    const long long g_end = (g0 + kG < L) ? g0 + kG : L;
    const KT row_mask = (((KT)1) << row_bits) - 1;
    const bool cont_in = g0 > 0 && keys[g0 - 1] == keys[g0];
    const bool tail_cont = g0 + kG < L && keys[g0 + kG - 1] == keys[g0 + kG];

    // ---- resolve: entry g0 + s * LPB + lig for s = 0 .. NS-1
    KT e_key[NS];
    unsigned e_bag[NS];
    float e_sc[NS];
    bool e_w[NS];
    {
        unsigned pos[NS];
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) {
            const long long e = g0 + s_ * LPB + lig;
            const bool live = e < g_end;
            e_key[s_] = live ? keys[e] : (KT)0;
            pos[s_] = live ? vals[e] : 0u;
        }
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) {
            const bool live = g0 + s_ * LPB + lig < g_end;
            const int t = (int)(e_key[s_] >> row_bits);
            e_bag[s_] = live ? bag_of[pos[s_]] : DLRM_DEAD_BAG;
            const float* psw = (const float*)s_psw[t];
            e_w[s_] = live && psw != nullptr;
            e_sc[s_] = e_w[s_] ? psw[(long long)pos[s_] - s_base[t]] : 1.f;
        }
    }

    VT acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) v_zero(acc[c]);
    KT run_key = group_bcast<KT>(e_key[0], lane0);       // key of entry g0
    bool run_first = true, run_empty = true;

    auto finish = [&](bool is_last) {
        if (run_first && cont_in) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) *(VT*)(edge_first + grp * DP + (c * LPB + lig) * VEC) = acc[c];
        } else if (is_last && tail_cont) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) *(VT*)(edge_last + grp * DP + (c * LPB + lig) * VEC) = acc[c];
        } else {
            const int t = (int)(run_key >> row_bits);
            const long long row = (long long)(run_key & row_mask);
            bf16_apply<VEC, LPB, NCH, ADA>((bf16_bits*)s_w[t] + row * D, ADA ? (float*)s_state[t] + row : nullptr, D, lig, acc, step, eps, ra,
                                           ra.tbase + (unsigned)t, row);
        }
    };

#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) {
        const long long s0 = g0 + s_ * LPB;
        if (s0 >= g_end) break;
        for (int j0 = 0; j0 < LPB; j0 += kC) {
            if (s0 + j0 >= g_end) break;
            KT k[kC];
            VT gr[kC][NCH];
            float sc[kC];
            bool live[kC], weighted[kC];
#pragma unroll
            for (int j = 0; j < kC; ++j) {
                const int src = lane0 + j0 + j;
                live[j] = s0 + j0 + j < g_end;
                k[j] = group_bcast<KT>(e_key[s_], src);
                unsigned bag = group_bcast<unsigned>(e_bag[s_], src);
                sc[j] = group_bcast<float>(e_sc[s_], src);
                const bool w_ = __shfl((int)e_w[s_], src, 64) != 0;
                const int t = (int)(k[j] >> row_bits);
                const bool dead = bag == DLRM_DEAD_BAG;            // out-of-range lookup (expand_kernel): zero gradient
                if (dead) bag = 0u;
                weighted[j] = live[j] && w_ && !dead;
                const float* grow = dout + (long long)bag * dout_ld + (long long)s_slot[t] * D;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int col = (c * LPB + lig) * VEC;
                    v_zero(gr[j][c]);
                    if (live[j] && !dead && col < D) gr[j][c] = *(const VT*)(grow + col);
                }
            }
#pragma unroll
            for (int j = 0; j < kC; ++j) {
                if (!live[j]) break;
                if (k[j] != run_key) {
                    finish(false);
                    run_key = k[j]; run_first = false; run_empty = true;
                }
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const VT v = weighted[j] ? v_scale(sc[j], gr[j][c]) : gr[j][c];
                    acc[c] = run_empty ? v : v_add(acc[c], v);
                }
                run_empty = false;
            }
        }
    }
    finish(true);
}

// one lane group per group index: acts only where a run starts in this group and continues into the next one
template <int VEC, int LPB, int NCH, typename KT, bool ADA>
__global__ __launch_bounds__(256) void bf16_fixup_kernel(SortedArgs sa, StateArgs aa, long long L, int D, int row_bits,
                                                         const KT* __restrict__ keys, DlrmStep step_, float eps, RoundArgs ra,
                                                         const float* __restrict__ edge_first, const float* __restrict__ edge_last) {
    const float step = step_;
    using VT = typename Vec<VEC>::T;
    constexpr int DP = NCH * LPB * VEC;
    constexpr int GPB = 256 / LPB;
    const int g = threadIdx.x / LPB, lig = threadIdx.x % LPB;
    const long long grp = (long long)blockIdx.x * GPB + g;
    const long long g0 = grp * kG;
    if (g0 + kG >= L) return;                                   // no next group: nothing continues
    const KT key = keys[g0 + kG - 1];
    if (key != keys[g0 + kG]) return;                           // last run ends inside this group
    if (g0 > 0 && keys[g0 - 1] == key) return;                  // the run began before this group: not the owner
    long long lo = g0 + kG + 1, hi = L;                         // keys[lo - 1] == key; run end = first position with another key
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] == key) lo = mid + 1; else hi = mid;
    }
    const long long last_grp = (lo - 1) / kG;                   // group holding the run's last entry (> grp)
    VT acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] = *(const VT*)(edge_last + grp * DP + (c * LPB + lig) * VEC);
    long long j = grp + 1;
    for (; j + 7 <= last_grp; j += 8) {                         // 8 independent partial rows in flight
        VT p[8][NCH];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int c = 0; c < NCH; ++c) p[u][c] = *(const VT*)(edge_first + (j + u) * DP + (c * LPB + lig) * VEC);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int c = 0; c < NCH; ++c) acc[c] = v_add(acc[c], p[u][c]);
    }
    for (; j <= last_grp; ++j)
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = v_add(acc[c], *(const VT*)(edge_first + j * DP + (c * LPB + lig) * VEC));
    const KT row_mask = (((KT)1) << row_bits) - 1;
    const int t = (int)(key >> row_bits);
    const long long row = (long long)(key & row_mask);
    bf16_apply<VEC, LPB, NCH, ADA>((bf16_bits*)sa.w[t] + row * D, ADA ? aa.state[t] + row : nullptr, D, lig, acc, step, eps, ra,
                                   ra.tbase + (unsigned)t, row);
}

// ---- host side ---------------------------------------------------------------------------------
struct Shape { int vec, lpb, nch, dp; };

// the lane geometry of adagrad.hip's pick(): 4 gradient columns per lane when D % 4 == 0 and everything is aligned, else 1
static int pick(int D, bool vec_ok, Shape* s) {
    s->vec = (vec_ok && D % 4 == 0) ? 4 : 1;
    const int units = s->vec == 4 ? D / 4 : D;
    s->lpb = pow2ceil(units); if (s->lpb < 4) s->lpb = 4; if (s->lpb > 64) s->lpb = 64;
    s->nch = (units + s->lpb - 1) / s->lpb; if (s->nch == 3) s->nch = 4;
    if (s->nch > 4) return DLRM_E_RANGE;
    s->dp = s->nch * s->lpb * s->vec;
    return 0;
}

static size_t edge_row_floats(int D) {
    Shape a, b;
    size_t m = 0;
    if (pick(D, true, &a) == 0) m = (size_t)a.dp;
    if (pick(D, false, &b) == 0 && (size_t)b.dp > m) m = (size_t)b.dp;
    return m;
}

struct Bf16Layout { Layout sort; size_t edge_first, edge_last, total; };

static int bf16_layout(size_t L, bool wide, int key_bits, int D, Bf16Layout* lo, int n, const int64_t* nnz, const int64_t* rows) {
    int rc = make_layout(L, wide, key_bits, &lo->sort, n, nnz, rows);
    if (rc) return rc;
    const size_t groups = (L + kG - 1) / kG;
    const size_t row = edge_row_floats(D);
    if (row == 0) return DLRM_E_RANGE;
    size_t o = lo->sort.total;
    lo->edge_first = o; o += align256(groups * row * sizeof(float));
    lo->edge_last = o;  o += align256(groups * row * sizeof(float));
    lo->total = o;
    return 0;
}

template <typename KT, bool ADA>
static int run_update(int n, const int* ids, int64_t B, int D, void* const* weight_host, void* const* state_host,
                      const int64_t* rows_host, const void* const* indices_host, const void* const* offsets_host,
                      const int64_t* nnz_host, const void* const* psw_host, int idx_bits, const float* dout, int64_t dout_ld,
                      DlrmStep step, float eps, RoundArgs ra, char* ws, const Bf16Layout& lo, size_t L, int row_bits, int key_bits, bool vec_ok,
                      hipStream_t st, int64_t* err) {
    SortedArgs sa;
    int rc = expand_and_sort<KT>(n, ids, B, weight_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, idx_bits, ws,
                                 lo.sort, L, row_bits, key_bits, st, &sa, err);
    if (rc) return rc;
    StateArgs aa;
    for (int k = 0; k < DLRM_MAX_TABLES_PER_LAUNCH; ++k) aa.state[k] = ADA ? (float*)state_host[ids[k < n ? k : 0]] : nullptr;
    const KT* keys = (const KT*)(ws + lo.sort.keys_out);
    const unsigned* vals = (const unsigned*)(ws + lo.sort.vals_out);
    const unsigned* bag_of = (const unsigned*)(ws + lo.sort.bag_of);
    float* ef = (float*)(ws + lo.edge_first);
    float* el = (float*)(ws + lo.edge_last);
    Shape s;
    rc = pick(D, vec_ok, &s);
    if (rc) return rc;
    const size_t groups = (L + kG - 1) / kG;
    const int gpb = 256 / s.lpb;
    dim3 grid((unsigned)((groups + gpb - 1) / gpb), 1, 1), block(256);
#define BF16_UPD(V, LP, NC)                                                                                                     \
    do {                                                                                                                        \
        hipLaunchKernelGGL((bf16_groups_kernel<V, LP, NC, KT, ADA>), grid, block, 0, st, sa, aa, (long long)L, D, row_bits, keys, vals, \
                           bag_of, dout, (long long)dout_ld, step, eps, ra, ef, el);                                            \
        DLRM_LAUNCH_CHECK();                                                                                                    \
        hipLaunchKernelGGL((bf16_fixup_kernel<V, LP, NC, KT, ADA>), grid, block, 0, st, sa, aa, (long long)L, D, row_bits, keys, \
                           step, eps, ra, (const float*)ef, (const float*)el);                                                  \
        DLRM_LAUNCH_CHECK();                                                                                                    \
    } while (0)
    const int key = s.vec * 10000 + s.lpb * 10 + s.nch;
    switch (key) {
        case 40041: BF16_UPD(4, 4, 1); break;   case 40081: BF16_UPD(4, 8, 1); break;   case 40161: BF16_UPD(4, 16, 1); break;
        case 40321: BF16_UPD(4, 32, 1); break;  case 40641: BF16_UPD(4, 64, 1); break;  case 40642: BF16_UPD(4, 64, 2); break;
        case 40644: BF16_UPD(4, 64, 4); break;
        case 10041: BF16_UPD(1, 4, 1); break;   case 10081: BF16_UPD(1, 8, 1); break;   case 10161: BF16_UPD(1, 16, 1); break;
        case 10321: BF16_UPD(1, 32, 1); break;  case 10641: BF16_UPD(1, 64, 1); break;  case 10642: BF16_UPD(1, 64, 2); break;
        case 10644: BF16_UPD(1, 64, 4); break;
        default: return DLRM_E_RANGE;
    }
#undef BF16_UPD
    return 0;
}

template <bool ADA>
static int bwd_bf16_impl(const char* what, int T, int64_t B, int D, void* const* weight_host, void* const* state_host,
                         const int64_t* rows_host, const void* const* indices_host, const void* const* offsets_host,
                         const int64_t* nnz_host, const void* const* psw_host, int idx_bits, const float* dout, int64_t dout_ld,
                         DlrmStep step, float eps, int rounding, uint64_t seed, int table0, void* workspace, int64_t workspace_bytes,
                         int64_t* err, void* stream) {
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
    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
        int ids[DLRM_MAX_TABLES_PER_LAUNCH];
        size_t L = 0; long long max_rows = 1;
        for (int k = 0; k < n; ++k) {
            ids[k] = t0 + k; L += (size_t)nnz_host[t0 + k];
            if (rows_host[t0 + k] > max_rows) max_rows = rows_host[t0 + k];
        }
        if (L == 0) continue;
        if (L >= ((size_t)1 << 32)) return DLRM_E_RANGE;
        const int row_bits = bits_for(max_rows), key_bits = row_bits + bits_for(n);
        const bool wide = key_bits > 32;
        Bf16Layout lo;
        int rc = bf16_layout(L, wide, key_bits, D, &lo, n, nnz_host + t0, rows_host + t0);
        if (rc) return rc;
        if (!workspace || !dlrm_aligned16(workspace) || (size_t)workspace_bytes < lo.total) {
            fprintf(stderr, "libdlrm_hip: %s: workspace too small (%lld < %zu bytes)\n", what, (long long)workspace_bytes, lo.total);
            return DLRM_E_ARG;
        }
        RoundArgs ra;
        ra.stochastic = rounding; ra.k0 = (unsigned)(seed & 0xFFFFFFFFull); ra.k1 = (unsigned)(seed >> 32); ra.tbase = (unsigned)(table0 + t0);
        rc = wide ? run_update<unsigned long long, ADA>(n, ids, B, D, weight_host, state_host, rows_host, indices_host, offsets_host, nnz_host,
                                                        psw_host, idx_bits, dout, dout_ld, step, eps, ra, (char*)workspace, lo, L, row_bits,
                                                        key_bits, vec_ok, st, err)
                  : run_update<unsigned, ADA>(n, ids, B, D, weight_host, state_host, rows_host, indices_host, offsets_host, nnz_host, psw_host,
                                              idx_bits, dout, dout_ld, step, eps, ra, (char*)workspace, lo, L, row_bits, key_bits, vec_ok, st, err);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

static int emb_fwd_bf16_impl(int T, int64_t B, int D, const void* const* weight_host, const int64_t* rows_host,
                            const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                            const void* const* psw_host, int idx_bits, float* out, int64_t out_ld, int64_t* err, DlrmPred pred, void* stream) {
    if (T <= 0 || B <= 0 || D <= 0) return DLRM_E_ARG;
    if (!weight_host || !rows_host || !indices_host || !offsets_host || !nnz_host) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    if (!out || out_ld < (int64_t)T * D) return DLRM_E_ARG;
    bool fast = D % 8 == 0 && D <= 512 && dlrm_aligned16(out) && (out_ld % 4 == 0);
    for (int t = 0; t < T; ++t) {
        if (!weight_host[t] || !offsets_host[t]) return DLRM_E_ARG;
        if (nnz_host[t] < 0 || rows_host[t] <= 0) return DLRM_E_ARG;
        if (nnz_host[t] > 0 && !indices_host[t]) return DLRM_E_ARG;
        if (((uintptr_t)weight_host[t]) & 1u) return DLRM_E_ALIGN;
        fast = fast && dlrm_aligned16(weight_host[t]);
    }
    hipStream_t st = (hipStream_t)stream;
    int lpb = 4;
    if (fast) { lpb = pow2ceil(D / 8); if (lpb < 4) lpb = 4; }
    constexpr int U = 2;             // bags per lane group (emb.hip's measured choice for the 4-rows-per-wave shape)
    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
        EmbArgs a;
        a.err = (long long*)err; a.pred = pred;
        for (int k = 0; k < DLRM_MAX_TABLES_PER_LAUNCH; ++k) {
            const int t = t0 + (k < n ? k : 0);
            a.w[k] = (float*)weight_host[t]; a.idx[k] = indices_host[t]; a.off[k] = offsets_host[t];
            a.psw[k] = psw_host ? (const float*)psw_host[t] : nullptr;
            a.nnz[k] = nnz_host[t]; a.rows[k] = rows_host[t]; a.slot[k] = t;
        }
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
    if (T <= 0 || D <= 0 || !nnz_host || !rows_host) return 0;
    size_t worst = 0;
    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
        size_t L = 0; long long max_rows = 1;
        for (int k = 0; k < n; ++k) { L += (size_t)nnz_host[t0 + k]; if (rows_host[t0 + k] > max_rows) max_rows = rows_host[t0 + k]; }
        if (L == 0) continue;
        const int row_bits = bits_for(max_rows), key_bits = row_bits + bits_for(n);
        Bf16Layout lo;
        if (bf16_layout(L, key_bits > 32, key_bits, D, &lo, n, nnz_host + t0, rows_host + t0) != 0) return -1;
        if (lo.total > worst) worst = lo.total;
    }
    return (int64_t)worst;
}

extern "C" int dlrm_emb_bwd_sgd_bf16(int T, int64_t B, int D, void* const* weight_host, const int64_t* rows_host,
                                     const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                                     const void* const* psw_host, int idx_bits, const float* dout, int64_t dout_ld, float lr,
                                     const float* lr_dev, int rounding, uint64_t seed, int table0, void* workspace, int64_t workspace_bytes,
                                     int64_t* err, void* stream) {
    return bwd_bf16_impl<false>("dlrm_emb_bwd_sgd_bf16", T, B, D, weight_host, nullptr, rows_host, indices_host, offsets_host, nnz_host, psw_host,
                                idx_bits, dout, dout_ld, dlrm_step_neg(lr, lr_dev), 0.f, rounding, seed, table0, workspace, workspace_bytes, err,
                                stream);
}

extern "C" int dlrm_emb_bwd_rowwise_adagrad_bf16(int T, int64_t B, int D, void* const* weight_host, void* const* state_host,
                                                 const int64_t* rows_host, const void* const* indices_host,
                                                 const void* const* offsets_host, const int64_t* nnz_host, const void* const* psw_host,
                                                 int idx_bits, const float* dout, int64_t dout_ld, float lr, const float* lr_dev, float eps,
                                                 int rounding, uint64_t seed, int table0, void* workspace, int64_t workspace_bytes,
                                                 int64_t* err, void* stream) {
    return bwd_bf16_impl<true>("dlrm_emb_bwd_rowwise_adagrad_bf16", T, B, D, weight_host, state_host, rows_host, indices_host, offsets_host,
                               nnz_host, psw_host, idx_bits, dout, dout_ld, dlrm_step_pos(lr, lr_dev), eps, rounding, seed, table0, workspace,
                               workspace_bytes, err, stream);
}
