// emb_md.hip — mixed-dimension embedding tables for gfx950: pooled lookup fused with the projection to the common width, and its backward.
//
// Reference replaced: tricks/md_embedding_bag.py (PrEmbeddingBag.forward and its autograd), built by DLRM_Net.create_emb for every table with
// more than md_threshold rows under --md-flag (dlrm_s_pytorch.py:267-275).  Table t keeps W_t [rows_t, d_t] and, when d_t < D, a bias-free
// projection P_t [D, d_t] (nn.Linear(d_t, D).weight):  out_t[b] = (sum_{i in bag} W_t[idx_i]) . P_t^T.  P_t == NULL is nn.Identity (d_t == D).
//
// Arithmetic, independent of the launch shape, of B and of the path taken:
//   pooled_t[b, c] = in-order fp32 sum from +0.0 (the bits of dlrm_emb_fwd at D = d_t, of F.embedding_bag(mode="sum") on the CPU);
//   out[b, t*D + j] = fmaf chain over c = 0 .. d_t-1 from +0.0 of pooled[c] * P_t[j, c];
//   gout[b, col_t + c] = fmaf chain over j = 0 .. D-1 from +0.0 of dout[b, t*D + j] * P_t[j, c];
//   dproj_t[j, c] = sum, in slab order, of the slab partials; a partial is the fmaf chain over the MD_SLAB bags of the slab in bag order.
// No atomics anywhere: every result is bit-identical from run to run.
//
// Forward design (dlrm_emb_fwd's conventions: blockIdx.y = table, pointers by value in the kernarg).  A workgroup owns one table and a tile of
// MD_TB bags.  (1) P_t is staged once in LDS, transposed to [c][j] at pitch D + 4: a lane's four outputs j .. j+3 are one 16-byte LDS read and
// lanes along j read consecutive addresses.  (2) Pooling: a lane owns (bag, 4 columns) — or (bag, column) when d_t % 4 != 0 or an operand is
// unaligned —, two such elements per pass with the first row loads of both issued before the first add, further lookups two at a time.  The
// pooled tile goes to LDS (odd pitch: lanes of different bags hit different banks), and to `saved` for the backward pass.  (3) Projection on
// the VALU (at Criteo-Terabyte shapes ~14 GFLOP against an 872 MB store: no MFMA needed): a lane owns (bag, 4 outputs) and stores 16 bytes
// when D % 4 == 0 and out is aligned, else (bag, output) and 4 bytes.
// A table whose (D + 4) * d_t + MD_TB * (d_t | 1) floats exceed 64 KiB of LDS (D = 512 with d_t >= 32, ...) keeps P_t in global memory: same
// chain, correct, not fast.  Identity tables pool straight into out.
//
// Backward design.  dlrm_emb_md_bwd_gout_kernel: a workgroup owns (table, MD_TBA bags), stages the dout tile (pitch D + 1) and P_t (when
// D * d_t + MD_TBA * (D + 1) floats fit 64 KiB, else P_t is read from global memory) and a lane owns (bag, column c).  Identity: a copy.
// dproj: dlrm_emb_md_bwd_dproj_partial_kernel — grid (elements of P_t / 256, slabs, tables), a lane owns one (j, c) and walks the slab's bags
// in order, reading dout and saved through the vector L1 (a wave reads one broadcast value and one coalesced run per bag) — then
// dlrm_emb_md_bwd_dproj_reduce_kernel sums the slab partials in slab order and OVERWRITES dproj_t.  Every shape takes these kernels: nothing
// is routed through dlrm_linear_bwd_weight.
#include "common.h"

namespace {

constexpr int MD_TB = 32;            // bags per workgroup, forward
constexpr int MD_TBA = 16;           // bags per workgroup, backward gout
constexpr int MD_SLAB = 512;         // bags per dproj partial: a compile-time constant, so the summation tree depends on B only
constexpr int MD_LDS_FLOATS = 16384; // 64 KiB

struct MdArgs {
    const float* proj[DLRM_MAX_TABLES_PER_LAUNCH];   // P_t [D, d_t], nullptr: identity
    int          dim[DLRM_MAX_TABLES_PER_LAUNCH];    // d_t
    int          col[DLRM_MAX_TABLES_PER_LAUNCH];    // first column of the table in saved / gout
    int          flags[DLRM_MAX_TABLES_PER_LAUNCH];  // MD_F_*
};
constexpr int MD_F_STAGE = 1;        // P_t staged in LDS
constexpr int MD_F_PVEC = 2;         // pooling with 16-byte loads / stores

template <int V> struct MdVec { float v[V]; };
template <int V> __device__ __forceinline__ MdVec<V> md_zero() { MdVec<V> r; for (int k = 0; k < V; ++k) r.v[k] = 0.f; return r; }
template <int V> __device__ __forceinline__ MdVec<V> md_load(const float* p);
template <> __device__ __forceinline__ MdVec<4> md_load<4>(const float* p) { const float4 x = *(const float4*)p; MdVec<4> r; r.v[0] = x.x; r.v[1] = x.y; r.v[2] = x.z; r.v[3] = x.w; return r; }
template <> __device__ __forceinline__ MdVec<1> md_load<1>(const float* p) { MdVec<1> r; r.v[0] = *p; return r; }
__device__ __forceinline__ void md_store(float* p, const MdVec<4>& a) { *(float4*)p = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]); }
__device__ __forceinline__ void md_store(float* p, const MdVec<1>& a) { *p = a.v[0]; }
template <int V> __device__ __forceinline__ void md_add(MdVec<V>& a, const MdVec<V>& x) {
#pragma unroll
    for (int k = 0; k < V; ++k) a.v[k] += x.v[k];
}

// pooled sums of the tile's bags: to LDS (`pooled`, pitch ppitch; nullptr for an identity table), to out (identity table) and to saved
template <typename IT, int V>
__device__ __forceinline__ void md_pool_tile(const float* __restrict__ W, const IT* __restrict__ idx, const IT* __restrict__ off, long long nnz,
                                             long long n, int d, long long B, long long b0, int nb, long long* err, int slot,
                                             float* pooled, int ppitch, float* outp, long long out_ld, float* savedp, long long saved_ld) {
    const int dv = d / V;
    const int nel = nb * dv;
    for (int e0 = threadIdx.x; e0 < nel; e0 += 512) {
        int u[2], c[2];
        bool act[2], ok[2];
        long long s[2], en[2], id[2];
        MdVec<V> acc[2], x[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = e0 + k * 256;
            act[k] = e < nel;
            u[k] = act[k] ? e / dv : 0;
            c[k] = act[k] ? (e - u[k] * dv) * V : 0;
            const long long b = b0 + u[k];
            s[k] = 0; en[k] = 0;
            if (act[k]) { s[k] = (long long)off[b]; en[k] = (b + 1 < B) ? (long long)off[b + 1] : nnz; }
            acc[k] = md_zero<V>();
            ok[k] = false; id[k] = 0;
            if (s[k] < en[k]) {
                id[k] = (long long)idx[s[k]];
                ok[k] = dlrm_index_ok(id[k], n);
                if (!ok[k]) dlrm_report_bad_index(err, slot, id[k], n);
            }
        }
        // the first row of both elements in flight before the first add
#pragma unroll
        for (int k = 0; k < 2; ++k) { x[k] = md_zero<V>(); if (ok[k]) x[k] = md_load<V>(W + id[k] * d + c[k]); }
#pragma unroll
        for (int k = 0; k < 2; ++k) if (ok[k]) md_add<V>(acc[k], x[k]);
        // further lookups of a multi-hot bag, two rows in flight
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            for (long long i = s[k] + 1; i < en[k]; i += 2) {
                long long r[2];
                bool okr[2];
                MdVec<V> y[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    r[j] = 0; okr[j] = false;
                    if (i + j < en[k]) {
                        r[j] = (long long)idx[i + j];
                        okr[j] = dlrm_index_ok(r[j], n);
                        if (!okr[j]) dlrm_report_bad_index(err, slot, r[j], n);
                    }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) { y[j] = md_zero<V>(); if (okr[j]) y[j] = md_load<V>(W + r[j] * d + c[k]); }
#pragma unroll
                for (int j = 0; j < 2; ++j) if (okr[j]) md_add<V>(acc[k], y[j]);
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!act[k]) continue;
            const long long b = b0 + u[k];
            if (pooled) {
#pragma unroll
                for (int q = 0; q < V; ++q) pooled[u[k] * ppitch + c[k] + q] = acc[k].v[q];
            }
            if (outp) md_store(outp + b * out_ld + c[k], acc[k]);
            if (savedp) md_store(savedp + b * saved_ld + c[k], acc[k]);
        }
    }
}

// OV = 4: D % 4 == 0, out 16-byte aligned, out_ld % 4 == 0
template <typename IT, int OV>
__global__ __launch_bounds__(256) void emb_fwd_md_kernel(EmbArgs a, MdArgs ma, long long B, int D, float* __restrict__ out, long long out_ld,
                                                         float* __restrict__ saved, long long saved_ld) {
    extern __shared__ __align__(16) float md_lds[];
    const int t = blockIdx.y;
    const long long b0 = (long long)blockIdx.x * MD_TB;
    if (b0 >= B) return;
    const int nb = (B - b0 < MD_TB) ? (int)(B - b0) : MD_TB;
    const float* __restrict__ W = a.w[t];
    const float* __restrict__ P = ma.proj[t];
    const IT* __restrict__ idx = (const IT*)a.idx[t];
    const IT* __restrict__ off = (const IT*)a.off[t];
    const int d = ma.dim[t], slot = a.slot[t], flags = ma.flags[t];
    const bool stage = (flags & MD_F_STAGE) != 0;
    float* savedp = saved ? saved + ma.col[t] : nullptr;
    float* o = out + (long long)slot * D;

    if (!P) {                                        // identity (d == D): the pooled row is the output
        if (flags & MD_F_PVEC) md_pool_tile<IT, 4>(W, idx, off, a.nnz[t], a.rows[t], d, B, b0, nb, a.err, slot, nullptr, 0, o, out_ld, savedp, saved_ld);
        else                   md_pool_tile<IT, 1>(W, idx, off, a.nnz[t], a.rows[t], d, B, b0, nb, a.err, slot, nullptr, 0, o, out_ld, savedp, saved_ld);
        return;
    }
    const int tpitch = D + 4;                        // P_t transposed: Pt[c * tpitch + j]
    float* Pt = md_lds;
    float* pooled = stage ? md_lds + tpitch * d : md_lds;
    const int ppitch = d | 1;
    if (stage) {
        const int np = D * d;
        for (int e = threadIdx.x; e < np; e += 256) {
            const int j = e / d, c = e - j * d;
            Pt[c * tpitch + j] = P[e];
        }
    }
    if (flags & MD_F_PVEC) md_pool_tile<IT, 4>(W, idx, off, a.nnz[t], a.rows[t], d, B, b0, nb, a.err, slot, pooled, ppitch, nullptr, 0, savedp, saved_ld);
    else                   md_pool_tile<IT, 1>(W, idx, off, a.nnz[t], a.rows[t], d, B, b0, nb, a.err, slot, pooled, ppitch, nullptr, 0, savedp, saved_ld);
    __syncthreads();

    const int Dv = D / OV;
    const int nel = nb * Dv;
    for (int e = threadIdx.x; e < nel; e += 256) {
        const int u = e / Dv, j = (e - u * Dv) * OV;
        const float* pr = pooled + u * ppitch;
        float acc[OV];
#pragma unroll
        for (int q = 0; q < OV; ++q) acc[q] = 0.f;
        if (stage) {
            for (int c = 0; c < d; ++c) {
                const float p = pr[c];
                const MdVec<OV> w = md_load<OV>(Pt + c * tpitch + j);
#pragma unroll
                for (int q = 0; q < OV; ++q) acc[q] = fmaf(p, w.v[q], acc[q]);
            }
        } else {
            for (int c = 0; c < d; ++c) {
                const float p = pr[c];
#pragma unroll
                for (int q = 0; q < OV; ++q) acc[q] = fmaf(p, P[(long long)(j + q) * d + c], acc[q]);
            }
        }
        MdVec<OV> r;
#pragma unroll
        for (int q = 0; q < OV; ++q) r.v[q] = acc[q];
        md_store(o + (b0 + u) * out_ld + j, r);
    }
}

// -------------------------------------------------------------------------------------------
// backward (a): gout[b, col_t + c] = sum_j dout[b, t*D + j] * P_t[j, c]
// -------------------------------------------------------------------------------------------
struct MdBwdArgs {
    const float* proj[DLRM_MAX_TABLES_PER_LAUNCH];
    float*       dproj[DLRM_MAX_TABLES_PER_LAUNCH];
    long long    woff[DLRM_MAX_TABLES_PER_LAUNCH];   // first float of the table's slab partials in the workspace
    int          dim[DLRM_MAX_TABLES_PER_LAUNCH];
    int          col[DLRM_MAX_TABLES_PER_LAUNCH];
    int          slot[DLRM_MAX_TABLES_PER_LAUNCH];
    int          stage[DLRM_MAX_TABLES_PER_LAUNCH];
};

__global__ __launch_bounds__(256) void emb_md_bwd_gout_kernel(MdBwdArgs a, long long B, int D, const float* __restrict__ dout, long long dout_ld,
                                                              float* __restrict__ gout, long long gout_ld) {
    extern __shared__ __align__(16) float md_lds[];
    const int t = blockIdx.y;
    const long long b0 = (long long)blockIdx.x * MD_TBA;
    if (b0 >= B) return;
    const int nb = (B - b0 < MD_TBA) ? (int)(B - b0) : MD_TBA;
    const float* __restrict__ P = a.proj[t];
    const int d = a.dim[t];
    const float* g = dout + (long long)a.slot[t] * D;
    float* o = gout + a.col[t];
    if (!P) {
        for (int e = threadIdx.x; e < nb * D; e += 256) {
            const int u = e / D, j = e - u * D;
            o[(b0 + u) * gout_ld + j] = g[(b0 + u) * dout_ld + j];
        }
        return;
    }
    const int gp = D + 1;
    float* gt = md_lds;                              // dout tile [MD_TBA][D + 1]
    float* Ps = md_lds + MD_TBA * gp;                // P_t [D][d] as it is
    const bool stage = a.stage[t] != 0;
    for (int e = threadIdx.x; e < nb * D; e += 256) {
        const int u = e / D, j = e - u * D;
        gt[u * gp + j] = g[(b0 + u) * dout_ld + j];
    }
    if (stage) for (int e = threadIdx.x; e < D * d; e += 256) Ps[e] = P[e];
    __syncthreads();
    const float* Pr = stage ? Ps : P;
    for (int e = threadIdx.x; e < nb * d; e += 256) {
        const int u = e / d, c = e - u * d;
        const float* gr = gt + u * gp;
        float acc = 0.f;
        for (int j = 0; j < D; ++j) acc = fmaf(gr[j], Pr[j * d + c], acc);
        o[(b0 + u) * gout_ld + c] = acc;
    }
}

// backward (b), slab partials: ws[woff_t + s * D * d_t + (j * d_t + c)] = fmaf chain over the slab's bags of dout[b, t*D + j] * saved[b, col_t + c]
__global__ __launch_bounds__(256) void emb_md_bwd_dproj_partial_kernel(MdBwdArgs a, long long B, int D, const float* __restrict__ dout,
                                                                      long long dout_ld, const float* __restrict__ saved, long long saved_ld,
                                                                      float* __restrict__ ws) {
    const int t = blockIdx.z;
    if (!a.dproj[t]) return;
    const int d = a.dim[t];
    const int np = D * d;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= np) return;
    const long long s = blockIdx.y;
    const long long b0 = s * MD_SLAB;
    const long long b1 = (b0 + MD_SLAB < B) ? b0 + MD_SLAB : B;
    const int j = e / d, c = e - j * d;
    const float* g = dout + (long long)a.slot[t] * D + j;
    const float* sv = saved + a.col[t] + c;
    float acc = 0.f;
    for (long long b = b0; b < b1; ++b) acc = fmaf(g[b * dout_ld], sv[b * saved_ld], acc);
    ws[a.woff[t] + s * np + e] = acc;
}

__global__ __launch_bounds__(256) void emb_md_bwd_dproj_reduce_kernel(MdBwdArgs a, int nslab, int D, const float* __restrict__ ws) {
    const int t = blockIdx.y;
    float* dp = a.dproj[t];
    if (!dp) return;
    const int np = D * a.dim[t];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= np) return;
    const float* p = ws + a.woff[t] + e;
    float acc = p[0];
    for (int s = 1; s < nslab; ++s) acc += p[(long long)s * np];
    dp[e] = acc;
}

bool md_dims_ok(int T, int D, const int32_t* dims_host) {
    for (int t = 0; t < T; ++t) if (dims_host[t] <= 0 || dims_host[t] > D) return false;
    return true;
}

}  // namespace

extern "C" int dlrm_emb_fwd_md(int T, int64_t B, int D, const int32_t* dims_host, const void* const* weight_host, const void* const* proj_host,
                               const int64_t* rows_host, const void* const* indices_host, const void* const* offsets_host,
                               const int64_t* nnz_host, int idx_bits, float* out, int64_t out_ld, float* saved, int64_t saved_ld,
                               const int32_t* col_host, int64_t* err, void* stream) {
    if (T <= 0 || B <= 0 || D <= 0) return DLRM_E_ARG;
    if (!dims_host || !weight_host || !proj_host || !rows_host || !indices_host || !offsets_host || !nnz_host) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    if (!out || out_ld < (int64_t)T * D) return DLRM_E_ARG;
    if (saved && !col_host) return DLRM_E_ARG;
    DLRM_REQUIRE(D <= 512, DLRM_E_RANGE, "embedding dimension above 512");
    if (!md_dims_ok(T, D, dims_host)) return DLRM_E_ARG;
    const bool ovec = D % 4 == 0 && dlrm_aligned16(out) && out_ld % 4 == 0;
    const bool svec = !saved || (dlrm_aligned16(saved) && saved_ld % 4 == 0);
    for (int t = 0; t < T; ++t) {
        if (!weight_host[t] || !offsets_host[t] || nnz_host[t] < 0 || rows_host[t] <= 0) return DLRM_E_ARG;
        if (nnz_host[t] > 0 && !indices_host[t]) return DLRM_E_ARG;
        if (!proj_host[t] && dims_host[t] != D) return DLRM_E_ARG;
        if (saved && (col_host[t] < 0 || (int64_t)col_host[t] + dims_host[t] > saved_ld)) return DLRM_E_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
        EmbArgs a = {};
        MdArgs ma = {};
        a.err = (long long*)err;
        int lds_floats = 0;
        for (int k = 0; k < n; ++k) {
            const int t = t0 + k;
            const int d = dims_host[t];
            a.w[k] = (float*)weight_host[t]; a.idx[k] = indices_host[t]; a.off[k] = offsets_host[t];
            a.nnz[k] = nnz_host[t]; a.rows[k] = rows_host[t]; a.slot[k] = t;
            ma.proj[k] = (const float*)proj_host[t]; ma.dim[k] = d; ma.col[k] = saved ? col_host[t] : 0;
            bool pvec = d % 4 == 0 && dlrm_aligned16(weight_host[t]) && svec && (!saved || col_host[t] % 4 == 0);
            int need = 0;
            if (proj_host[t]) {
                const int tile = MD_TB * (d | 1);
                const int staged = (D + 4) * d + tile;
                if (ovec && staged <= MD_LDS_FLOATS) { ma.flags[k] |= MD_F_STAGE; need = staged; }
                else need = tile;                    // (d < D <= 512: at most 32 * 511 floats)
            } else {
                pvec = pvec && ovec;                 // the pooled row is stored to out
            }
            if (pvec) ma.flags[k] |= MD_F_PVEC;
            DLRM_REQUIRE(need <= MD_LDS_FLOATS, DLRM_E_RANGE, "a projection with d == D == 512 (use an identity table)");
            if (need > lds_floats) lds_floats = need;
        }
        dim3 grid((unsigned)((B + MD_TB - 1) / MD_TB), (unsigned)n, 1), block(256, 1, 1);
        const size_t lds = (size_t)lds_floats * sizeof(float);
        if (ovec) {
            if (idx_bits == 64) hipLaunchKernelGGL((emb_fwd_md_kernel<long long, 4>), grid, block, lds, st, a, ma, (long long)B, D, out, (long long)out_ld, saved, (long long)saved_ld);
            else                hipLaunchKernelGGL((emb_fwd_md_kernel<int, 4>), grid, block, lds, st, a, ma, (long long)B, D, out, (long long)out_ld, saved, (long long)saved_ld);
        } else {
            if (idx_bits == 64) hipLaunchKernelGGL((emb_fwd_md_kernel<long long, 1>), grid, block, lds, st, a, ma, (long long)B, D, out, (long long)out_ld, saved, (long long)saved_ld);
            else                hipLaunchKernelGGL((emb_fwd_md_kernel<int, 1>), grid, block, lds, st, a, ma, (long long)B, D, out, (long long)out_ld, saved, (long long)saved_ld);
        }
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int64_t dlrm_emb_md_bwd_workspace_bytes(int T, int64_t B, int D, const int32_t* dims_host) {
    if (T <= 0 || B <= 0 || D <= 0 || !dims_host) return -1;
    const int64_t nslab = (B + MD_SLAB - 1) / MD_SLAB;
    int64_t floats = 0;
    for (int t = 0; t < T; ++t) {
        if (dims_host[t] <= 0 || dims_host[t] > D) return -1;
        floats += nslab * (int64_t)D * dims_host[t];
    }
    return floats * (int64_t)sizeof(float);
}

extern "C" int dlrm_emb_md_bwd(int T, int64_t B, int D, const int32_t* dims_host, const void* const* proj_host, const float* dout, int64_t dout_ld,
                               const float* saved, int64_t saved_ld, const int32_t* col_host, float* gout, int64_t gout_ld,
                               void* const* dproj_host, void* workspace, int64_t workspace_bytes, void* stream) {
    if (T <= 0 || B <= 0 || D <= 0 || !dims_host || !proj_host || !dout || !col_host || !gout || !dproj_host) return DLRM_E_ARG;
    DLRM_REQUIRE(D <= 512, DLRM_E_RANGE, "embedding dimension above 512");
    if (!md_dims_ok(T, D, dims_host) || dout_ld < (int64_t)T * D) return DLRM_E_ARG;
    bool any_dproj = false;
    for (int t = 0; t < T; ++t) {
        if (!proj_host[t] && (dims_host[t] != D || dproj_host[t])) return DLRM_E_ARG;
        if (col_host[t] < 0 || (int64_t)col_host[t] + dims_host[t] > gout_ld) return DLRM_E_ARG;
        if (dproj_host[t]) {
            any_dproj = true;
            if (!saved || (int64_t)col_host[t] + dims_host[t] > saved_ld) return DLRM_E_ARG;
        }
    }
    const int64_t nslab = (B + MD_SLAB - 1) / MD_SLAB;
    if (any_dproj && (!workspace || workspace_bytes < dlrm_emb_md_bwd_workspace_bytes(T, B, D, dims_host))) return DLRM_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    long long woff = 0;
    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
        MdBwdArgs a = {};
        int lds_floats = 0, dmax = 0;
        bool dproj_here = false;
        for (int k = 0; k < n; ++k) {
            const int t = t0 + k;
            const int d = dims_host[t];
            a.proj[k] = (const float*)proj_host[t]; a.dproj[k] = (float*)dproj_host[t];
            a.dim[k] = d; a.col[k] = col_host[t]; a.slot[k] = t; a.woff[k] = woff;
            woff += (long long)nslab * D * d;
            if (proj_host[t]) {
                const int tile = MD_TBA * (D + 1);
                const int staged = tile + D * d;
                if (staged <= MD_LDS_FLOATS) { a.stage[k] = 1; if (staged > lds_floats) lds_floats = staged; }
                else if (tile > lds_floats) lds_floats = tile;
            }
            if (dproj_host[t]) { dproj_here = true; if (d > dmax) dmax = d; }
        }
        dim3 block(256, 1, 1);
        dim3 grid((unsigned)((B + MD_TBA - 1) / MD_TBA), (unsigned)n, 1);
        hipLaunchKernelGGL(emb_md_bwd_gout_kernel, grid, block, (size_t)lds_floats * sizeof(float), st, a, (long long)B, D, dout, (long long)dout_ld,
                           gout, (long long)gout_ld);
        DLRM_LAUNCH_CHECK();
        if (dproj_here) {
            const unsigned nbx = (unsigned)(((long long)D * dmax + 255) / 256);
            DLRM_REQUIRE(nslab <= 65535, DLRM_E_RANGE, "more than 65535 slabs of bags");
            hipLaunchKernelGGL(emb_md_bwd_dproj_partial_kernel, dim3(nbx, (unsigned)nslab, (unsigned)n), block, 0, st, a, (long long)B, D, dout,
                               (long long)dout_ld, saved, (long long)saved_ld, (float*)workspace);
            DLRM_LAUNCH_CHECK();
            hipLaunchKernelGGL(emb_md_bwd_dproj_reduce_kernel, dim3(nbx, (unsigned)n, 1), block, 0, st, a, (int)nslab, D, (const float*)workspace);
            DLRM_LAUNCH_CHECK();
        }
    }
    return 0;
}
