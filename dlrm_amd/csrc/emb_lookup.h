// emb_lookup.h — the pooled EmbeddingBag(sum) lookup, once, for every row format, and the host side the lookup entry points share.
//
// emb_lookup_body is the algorithm of emb.hip's header comment: a group of LPB lanes owns a bag, a lane owns its columns of the row and sums
// the rows itself in index order (no cross-lane reduction, so the bits do not depend on the launch shape); each group works on U bags at once,
// issues the U first-row loads back to back, and continues longer bags four rows at a time.  What differs between the formats is a ROW
// SOURCE, a type of static members only:
//   Elem                          the table's element type; a row starts at W + row * pitch(D)
//   COLS                          columns a lane owns per chunk; a lane's chunk c starts at column (c * LPB + lig) * COLS
//   Staged / Acc                  a loaded, not yet accumulated chunk of a row / the chunk's fp32 sums
//   zero(Staged&), clear(Acc&)
//   load(Staged&, row, D, col)    the lane's loads of one chunk (row = start of the row)
//   accum(Acc&, w, Staged)        acc = fmaf(w, value, acc) per column: ONE rounding per row and column on the widened / dequantised value
//   store(float*, Acc)            the chunk's sums to out
// The sources: Fp32Rows<VEC> here (VEC = 4 or 1 columns per lane, up to 4 chunks), Bf16Rows (emb_bf16.hip) and QuantRows<BITS>
// (emb_quant.hip), 8 columns per lane and one chunk.  A new row format supplies a source, a thin __global__ wrapper around the body and its
// launch plan; emb_fwd_qr_kernel (two sums per bag, no pooling weights) keeps its own body and takes the host helpers only.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

template <int VEC> struct Vec;
template <> struct Vec<4> { using T = float4; };
template <> struct Vec<1> { using T = float; };

__device__ __forceinline__ void v_zero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void v_zero(float& a) { a = 0.f; }
// acc = fma(w, v, acc) per component.  With w == 1.0f this is exactly acc + v (single rounding),
// so the unweighted path reproduces the reference's plain in-order sum bit for bit.
__device__ __forceinline__ void v_fma(float4& a, float w, const float4& v) {
    a.x = __builtin_fmaf(w, v.x, a.x); a.y = __builtin_fmaf(w, v.y, a.y);
    a.z = __builtin_fmaf(w, v.z, a.z); a.w = __builtin_fmaf(w, v.w, a.w);
}
__device__ __forceinline__ void v_fma(float& a, float w, const float& v) { a = __builtin_fmaf(w, v, a); }

template <int VEC>
struct Fp32Rows {
    using Elem = float;
    using Staged = typename Vec<VEC>::T;
    using Acc = Staged;
    static constexpr int COLS = VEC;
    static __device__ __forceinline__ long long pitch(int D) { return D; }
    static __device__ __forceinline__ void zero(Staged& v) { v_zero(v); }
    static __device__ __forceinline__ void clear(Acc& a) { v_zero(a); }
    static __device__ __forceinline__ void load(Staged& v, const float* __restrict__ row, int, int col) { v = *(const Staged*)(row + col); }
    static __device__ __forceinline__ void accum(Acc& a, float w, const Staged& v) { v_fma(a, w, v); }
    static __device__ __forceinline__ void store(float* o, const Acc& a) { *(Acc*)o = a; }
};

// the store of the sources with 8 columns per lane
__device__ __forceinline__ void store8(float* o, const float (&acc)[8]) {
    *(float4*)(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *(float4*)(o + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// LOOP (dlrm_emb_fwd_pred only): a capped grid walks the bags with a grid stride.  A predicated launch that does NOT run still has its
// workgroups dispatched, and the plain launch has one workgroup per 16 bags (106 k workgroups at Criteo-Terabyte shapes: ~20 us of dispatch
// for a launch that returns at once); LOOP = false is the straight-line kernel of every other call, unchanged.
template <typename Src, int LPB, int NCH, typename IT, int U, bool LOOP>
__device__ __forceinline__ void emb_lookup_body(const EmbArgs& a, long long B, int D, float* __restrict__ out, long long out_ld) {
    using Staged = typename Src::Staged;
    using Acc = typename Src::Acc;
    if (a.pred.skip()) return;      // (the *_pred entry points: the other implementation of this step runs instead)
    const int t = blockIdx.y;
    const typename Src::Elem* __restrict__ W = (const typename Src::Elem*)a.w[t];
    const IT* __restrict__ idx = (const IT*)a.idx[t];
    const IT* __restrict__ off = (const IT*)a.off[t];
    const float* __restrict__ psw = a.psw[t];
    const long long nnz = a.nnz[t];
    const long long rows = a.rows[t];
    const long long RP = Src::pitch(D);

    constexpr int GPB = 256 / LPB;  // groups (bags in flight) per workgroup
    const int g = threadIdx.x / LPB;
    const int lig = threadIdx.x % LPB;
    long long b0 = ((long long)blockIdx.x * GPB + g) * U;
    if (b0 >= B) return;
  for (;;) {
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

    Acc acc[U][NCH];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < NCH; ++c) Src::clear(acc[u][c]);

    // ---- phase 1: first row of every bag, all loads in flight together --------------------
    // an out-of-range index contributes nothing and is reported (the reference raises on it)
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
    Staged v0[U][NCH];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int col = (c * LPB + lig) * Src::COLS;
            Src::zero(v0[u][c]);
            if (ok0[u] && col < D) Src::load(v0[u][c], W + r0[u] * RP, D, col);
        }
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (ok0[u]) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) Src::accum(acc[u][c], w0[u], v0[u][c]);
        }

    // ---- phase 2: remaining rows of multi-hot bags, 4 row loads in flight per bag ----------
#pragma unroll
    for (int u = 0; u < U; ++u) {
        long long i = s[u] + 1;
        const long long end = e[u];
        for (; i + 4 <= end; i += 4) {
            long long r[4]; float w[4]; Staged v[4][NCH];
            bool ok[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r[k] = (long long)idx[i + k]; w[k] = psw ? psw[i + k] : 1.f;
                ok[k] = dlrm_index_ok(r[k], rows);
                if (!ok[k]) dlrm_report_bad_index(a.err, a.slot[t], r[k], rows);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int col = (c * LPB + lig) * Src::COLS;
                    Src::zero(v[k][c]);
                    if (ok[k] && col < D) Src::load(v[k][c], W + r[k] * RP, D, col);
                }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (ok[k]) {
#pragma unroll
                    for (int c = 0; c < NCH; ++c) Src::accum(acc[u][c], w[k], v[k][c]);
                }
            }
        }
        for (; i < end; ++i) {
            const long long r = (long long)idx[i];
            const float w = psw ? psw[i] : 1.f;
            if (!dlrm_index_ok(r, rows)) { dlrm_report_bad_index(a.err, a.slot[t], r, rows); continue; }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int col = (c * LPB + lig) * Src::COLS;
                if (col < D) { Staged v; Src::load(v, W + r * RP, D, col); Src::accum(acc[u][c], w, v); }
            }
        }
    }

    // ---- store: bag b of table t goes to out[b, slot*D : +D] ----------------------------------
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const long long b = b0 + u;
        if (b < B) {
            float* o = out + b * out_ld + (long long)a.slot[t] * D;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int col = (c * LPB + lig) * Src::COLS;
                if (col < D) Src::store(o + col, acc[u][c]);
            }
        }
    }
    if constexpr (!LOOP) break;
    b0 += (long long)gridDim.x * GPB * U;
    if (b0 >= B) break;
  }
}

// -------------------------------------------------------------------------------------------
// host side: the argument checks and the EmbArgs fill of every lookup entry point (and of emb.hip's backward kernels)
// -------------------------------------------------------------------------------------------
static int pow2ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// lanes per bag for `units` lane-sized pieces of a row: a power of two, 4 .. 64
static int lanes_per_bag(int units) { const int l = pow2ceil(units); return l < 4 ? 4 : l > 64 ? 64 : l; }

// The lane geometry of fp32 rows (the lookup, emb.hip's atomic backward, the gradient rows of sorted_walk.h): 4 columns per lane when
// D % 4 == 0 and everything is 16-byte aligned, else 1; 1, 2 or 4 chunks.  dp: the padded row length.
struct Shape { int vec, lpb, nch, dp; };

static int pick(int D, bool vec_ok, Shape* s) {
    s->vec = (vec_ok && D % 4 == 0) ? 4 : 1;
    const int units = s->vec == 4 ? D / 4 : D;
    s->lpb = lanes_per_bag(units);
    s->nch = (units + s->lpb - 1) / s->lpb; if (s->nch == 3) s->nch = 4;
    if (s->nch > 4) return DLRM_E_RANGE;
    s->dp = s->nch * s->lpb * s->vec;
    return 0;
}

// The shape dispatch, once: f(VEC, LPB, NCH) is called with the shape as integral_constants and its code returned; DLRM_E_RANGE: no
// kernel is built for the shape.
template <int V, int L, int N, typename F>
static bool shape_case(const Shape& s, F& f, int* rc) {
    if (s.vec != V || s.lpb != L || s.nch != N) return false;
    *rc = f(std::integral_constant<int, V>{}, std::integral_constant<int, L>{}, std::integral_constant<int, N>{});
    return true;
}
template <int V, typename F>
static bool shape_cases(const Shape& s, F& f, int* rc) {
    return shape_case<V, 4, 1>(s, f, rc) || shape_case<V, 8, 1>(s, f, rc) || shape_case<V, 16, 1>(s, f, rc) || shape_case<V, 32, 1>(s, f, rc) ||
           shape_case<V, 64, 1>(s, f, rc) || shape_case<V, 64, 2>(s, f, rc) || shape_case<V, 64, 4>(s, f, rc);
}
template <typename F>
static int dispatch_shape(const Shape& s, F f) {
    int rc = DLRM_E_RANGE;
    (void)(shape_cases<4>(s, f, &rc) || shape_cases<1>(s, f, &rc));
    return rc;
}

// the head of the checks; more_lists: the entry point's further host arrays are there too
static int emb_check_lists(int T, int64_t B, int D, const void* const* weight_host, const int64_t* rows_host, const void* const* indices_host,
                           const void* const* offsets_host, const int64_t* nnz_host, int idx_bits, bool more_lists = true) {
    if (T <= 0 || B <= 0 || D <= 0) return DLRM_E_ARG;
    if (!weight_host || !rows_host || !indices_host || !offsets_host || !nnz_host || !more_lists) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    return 0;
}
static int emb_check_table(int t, const void* const* weight_host, const int64_t* rows_host, const void* const* indices_host,
                           const void* const* offsets_host, const int64_t* nnz_host) {
    if (!weight_host[t] || !offsets_host[t]) return DLRM_E_ARG;
    if (nnz_host[t] < 0 || rows_host[t] <= 0) return DLRM_E_ARG;
    if (nnz_host[t] > 0 && !indices_host[t]) return DLRM_E_ARG;
    return 0;
}
static int emb_check_tables(int T, const void* const* weight_host, const int64_t* rows_host, const void* const* indices_host,
                            const void* const* offsets_host, const int64_t* nnz_host) {
    for (int t = 0; t < T; ++t)
        if (emb_check_table(t, weight_host, rows_host, indices_host, offsets_host, nnz_host)) return DLRM_E_ARG;
    return 0;
}
static int emb_check_common(int T, int64_t B, int D, const void* const* weight_host, const int64_t* rows_host, const void* const* indices_host,
                            const void* const* offsets_host, const int64_t* nnz_host, int idx_bits) {
    const int rc = emb_check_lists(T, B, D, weight_host, rows_host, indices_host, offsets_host, nnz_host, idx_bits);
    return rc ? rc : emb_check_tables(T, weight_host, rows_host, indices_host, offsets_host, nnz_host);
}

// tables ids[0 .. n) of the caller's list as one launch group; unused slots repeat the first one (never dereferenced)
static void emb_fill_args(EmbArgs& a, const int* ids, int n, const void* const* weight_host, const int64_t* rows_host,
                          const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                          const void* const* psw_host, int64_t* err, DlrmPred pred = DlrmPred{nullptr, 0}) {
    a.err = (long long*)err;
    a.pred = pred;
    for (int k = 0; k < DLRM_MAX_TABLES_PER_LAUNCH; ++k) {
        const int t = ids[k < n ? k : 0];
        a.w[k] = (float*)weight_host[t];            // (bf16 / packed rows too: the kernels read them as their source's Elem)
        a.idx[k] = indices_host[t];
        a.off[k] = offsets_host[t];
        a.psw[k] = psw_host ? (const float*)psw_host[t] : nullptr;
        a.nnz[k] = nnz_host[t];
        a.rows[k] = rows_host[t];
        a.slot[k] = t;
    }
}
// ... tables t0 .. t0 + n
static void emb_fill_args(EmbArgs& a, int t0, int n, const void* const* weight_host, const int64_t* rows_host,
                          const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                          const void* const* psw_host, int64_t* err, DlrmPred pred = DlrmPred{nullptr, 0}) {
    int ids[DLRM_MAX_TABLES_PER_LAUNCH];
    for (int k = 0; k < n; ++k) ids[k] = t0 + k;
    emb_fill_args(a, ids, n, weight_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, err, pred);
}

}  // namespace
