// emb_qr.hip — quotient-remainder (compositional) embedding tables for gfx950: pooled lookup, gradient split, index split.
//
// Reference replaced: tricks/qr_embedding_bag.py (QREmbeddingBag.forward), built by DLRM_Net.create_emb for every table with more than
// qr_threshold rows (dlrm_s_pytorch.py:258-266).  A QR table of n categories and c collisions keeps weight_q [ceil(n / c), D] and
// weight_r [c, D];  out[b] = (sum_i Wq[q_i]) o (sum_i Wr[r_i])  with o = * ("mult") or + ("add"): the composition is applied to the two
// POOLED sums (for multi-hot bags the product of sums, not the sum of products).
//
// THE QUOTIENT IS A FLOAT32 DIVISION.  The reference computes `(input / c).long()`: torch's true division of an int64 tensor by a Python
// int converts both to float32 (round to nearest), divides (IEEE) and truncates.  That equals id / c (integer) for every id < 2^24; above,
// float32 cannot hold the id and other rows are chosen (n = 39,884,406, c = 4: 1,125,000 of the top 3,000,000 ids), and an id close to
// n can even get the quotient ceil(n / c), which is no row (n = 40,000,000, c = 4: ids 39,999,998 and 39,999,999).  A checkpoint the
// reference trained is read correctly by this mapping only, so the kernels compute exactly that: (long long)__fdiv_rn((float)id, (float)c).
// r = id mod c is integer arithmetic in the reference too.  An id outside [0, n), or one whose quotient is >= ceil(n / c), is SKIPPED
// (both components) and reported through the error block as {1, table, id, n}; the reference raises on it.
//
// Design (HBM-bound, no MFMA), dlrm_emb_fwd's conventions (emb.hip): one launch covers every table (blockIdx.y = table, pointers by value
// in the kernarg), a group of LPB lanes owns a bag and a lane 4 columns (one 16-byte load per row), sums run IN INDEX ORDER per column per
// component from +0.0 (bit-identical to two F.embedding_bag calls on the CPU), the two sums are combined ONCE, and the pooled row is
// written.  The q-row and r-row loads of a lookup are issued together, and the first lookups of U = 2 bags (4 row loads per lane group)
// are in flight before the first dependent add; further lookups of a bag go two at a time (again 4 loads).  weight_r is c rows (2 KiB at
// c = 4, D = 128): every workgroup reads the same few lines, which stay in the vector L1 / L2 — it is not staged in LDS.
// A table with collisions == 0 is a plain table: one sum, no composition, the bits dlrm_emb_fwd gives.
#include "emb_lookup.h"
#include "qr_split.h"

namespace {

struct QrArgs {
    const float* wr[DLRM_MAX_TABLES_PER_LAUNCH];     // weight_r (nullptr: plain table)
    int          coll[DLRM_MAX_TABLES_PER_LAUNCH];   // collisions (0: plain table)
    int          qslot[DLRM_MAX_TABLES_PER_LAUNCH];  // position among the QR tables of the call: its sums go to saved[:, 2*qslot*D .. +2D)
    long long    rows_q[DLRM_MAX_TABLES_PER_LAUNCH]; // ceil(n / c) (plain: rows)
};

__device__ __forceinline__ void f4_add(float4& a, const float4& v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
__device__ __forceinline__ float4 f4_mul(const float4& a, const float4& b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 f4_sum(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// -------------------------------------------------------------------------------------------
// forward, 16-byte form: D % 4 == 0, every operand 16-byte aligned
// -------------------------------------------------------------------------------------------
template <int LPB, int NCH, typename IT, int U>
__global__ __launch_bounds__(256) void emb_fwd_qr_kernel(EmbArgs a, QrArgs qa, long long B, int D, int op_add,
                                                         float* __restrict__ out, long long out_ld,
                                                         float* __restrict__ saved, long long saved_ld) {
    if (a.pred.skip()) return;          // dlrm_emb_fwd_qr_pred (flag == nullptr: always run)
    const int t = blockIdx.y;
    const float* __restrict__ Wq = a.w[t];
    const float* __restrict__ Wr = qa.wr[t];
    const IT* __restrict__ idx = (const IT*)a.idx[t];
    const IT* __restrict__ off = (const IT*)a.off[t];
    const long long nnz = a.nnz[t];
    const long long n = a.rows[t];
    const long long rows_q = qa.rows_q[t];
    const int c = qa.coll[t];                        // workgroup-uniform: 0 = plain table
    const bool qr = c != 0;

    constexpr int GPB = 256 / LPB;
    const int g = threadIdx.x / LPB;
    const int lig = threadIdx.x % LPB;
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
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 accq[U][NCH], accr[U][NCH];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < NCH; ++k) { accq[u][k] = zero; accr[u][k] = zero; }

    // ---- phase 1: the first lookup of every bag: its q row and its r row, all bags' loads in flight together
    long long q0[U], r0[U];
    bool ok0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        q0[u] = 0; r0[u] = 0; ok0[u] = false;
        if (s[u] < e[u]) {
            const long long id = (long long)idx[s[u]];
            if (qr) ok0[u] = qr_split(id, n, c, rows_q, &q0[u], &r0[u]);
            else { ok0[u] = dlrm_index_ok(id, n); q0[u] = id; }
            if (!ok0[u]) dlrm_report_bad_index(a.err, a.slot[t], id, n);
        }
    }
    {
        float4 vq[U][NCH], vr[U][NCH];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                const int col = (k * LPB + lig) * 4;
                vq[u][k] = zero; vr[u][k] = zero;
                if (ok0[u] && col < D) {
                    vq[u][k] = *(const float4*)(Wq + q0[u] * D + col);
                    if (qr) vr[u][k] = *(const float4*)(Wr + r0[u] * D + col);
                }
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (ok0[u]) {
#pragma unroll
                for (int k = 0; k < NCH; ++k) { f4_add(accq[u][k], vq[u][k]); f4_add(accr[u][k], vr[u][k]); }
            }
    }

    // ---- phase 2: further lookups of multi-hot bags, two lookups (four row loads) in flight per bag
#pragma unroll
    for (int u = 0; u < U; ++u) {
        long long i = s[u] + 1;
        const long long end = e[u];
        for (; i < end; i += 2) {
            long long q[2], r[2];
            bool ok[2];
            float4 vq[2][NCH], vr[2][NCH];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                q[j] = 0; r[j] = 0; ok[j] = false;
                if (i + j < end) {
                    const long long id = (long long)idx[i + j];
                    if (qr) ok[j] = qr_split(id, n, c, rows_q, &q[j], &r[j]);
                    else { ok[j] = dlrm_index_ok(id, n); q[j] = id; }
                    if (!ok[j]) dlrm_report_bad_index(a.err, a.slot[t], id, n);
                }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    const int col = (k * LPB + lig) * 4;
                    vq[j][k] = zero; vr[j][k] = zero;
                    if (ok[j] && col < D) {
                        vq[j][k] = *(const float4*)(Wq + q[j] * D + col);
                        if (qr) vr[j][k] = *(const float4*)(Wr + r[j] * D + col);
                    }
                }
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (ok[j]) {
#pragma unroll
                    for (int k = 0; k < NCH; ++k) { f4_add(accq[u][k], vq[j][k]); f4_add(accr[u][k], vr[j][k]); }
                }
        }
    }

    // ---- combine once, store the pooled row (and the two sums for the backward pass)
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const long long b = b0 + u;
        if (b >= B) continue;
        float* o = out + b * out_ld + (long long)a.slot[t] * D;
        float* sv = (saved && qr) ? saved + b * saved_ld + (long long)qa.qslot[t] * 2 * D : nullptr;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int col = (k * LPB + lig) * 4;
            if (col >= D) continue;
            float4 y = accq[u][k];
            if (qr) y = op_add ? f4_sum(accq[u][k], accr[u][k]) : f4_mul(accq[u][k], accr[u][k]);
            *(float4*)(o + col) = y;
            if (sv) { *(float4*)(sv + col) = accq[u][k]; *(float4*)(sv + D + col) = accr[u][k]; }
        }
    }
}

// forward, scalar form (any D, any alignment): one wavefront per bag, a lane walks the bag once per column it owns.  Correct, not fast.
template <typename IT>
__global__ __launch_bounds__(256) void emb_fwd_qr_scalar_kernel(EmbArgs a, QrArgs qa, long long B, int D, int op_add,
                                                                float* __restrict__ out, long long out_ld,
                                                                float* __restrict__ saved, long long saved_ld) {
    if (a.pred.skip()) return;
    const int t = blockIdx.y;
    const float* __restrict__ Wq = a.w[t];
    const float* __restrict__ Wr = qa.wr[t];
    const IT* __restrict__ idx = (const IT*)a.idx[t];
    const IT* __restrict__ off = (const IT*)a.off[t];
    const long long n = a.rows[t], rows_q = qa.rows_q[t];
    const int c = qa.coll[t];
    const bool qr = c != 0;
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const long long s = (long long)off[b];
    const long long e = (b + 1 < B) ? (long long)off[b + 1] : a.nnz[t];
    for (int d = lane; d < D; d += 64) {
        float sq = 0.f, sr = 0.f;
        for (long long i = s; i < e; ++i) {
            const long long id = (long long)idx[i];
            long long q = id, r = 0;
            const bool ok = qr ? qr_split(id, n, c, rows_q, &q, &r) : dlrm_index_ok(id, n);
            if (!ok) { dlrm_report_bad_index(a.err, a.slot[t], id, n); continue; }
            sq += Wq[q * D + d];
            if (qr) sr += Wr[r * D + d];
        }
        out[b * out_ld + (long long)a.slot[t] * D + d] = qr ? (op_add ? sq + sr : sq * sr) : sq;
        if (saved && qr) {
            float* sv = saved + b * saved_ld + (long long)qa.qslot[t] * 2 * D;
            sv[d] = sq; sv[D + d] = sr;
        }
    }
}

// -------------------------------------------------------------------------------------------
// gradient split: dout [B, T*D] (+ the saved sums) -> the gradient buffer of the VIRTUAL table list [B, Tv*D]
// -------------------------------------------------------------------------------------------
struct SplitArgs {
    int vslot[DLRM_MAX_TABLES_PER_LAUNCH];           // virtual slot of the table (of its q component)
    int qslot[DLRM_MAX_TABLES_PER_LAUNCH];           // position among the QR tables, -1: plain table
    int slot[DLRM_MAX_TABLES_PER_LAUNCH];            // column block of the table in dout
    DlrmPred pred;                                   // launch predicate (dlrm_emb_qr_bwd_split_pred); flag == nullptr: always run
};

template <typename VT> struct SplitOps;
template <> struct SplitOps<float4> { static __device__ __forceinline__ float4 mul(const float4& a, const float4& b) { return f4_mul(a, b); } };
template <> struct SplitOps<float> { static __device__ __forceinline__ float mul(float a, float b) { return a * b; } };

template <typename VT>
__global__ __launch_bounds__(256) void emb_qr_bwd_split_kernel(SplitArgs sa, long long B, int Dv /* D in units of VT */, int op_add,
                                                               const VT* __restrict__ dout, long long dout_ld,
                                                               const VT* __restrict__ saved, long long saved_ld,
                                                               VT* __restrict__ gout, long long gout_ld) {
    if (sa.pred.skip()) return;
    const int t = blockIdx.y;
    const int vs = sa.vslot[t], qs = sa.qslot[t], ds = sa.slot[t];
    const long long total = B * Dv;
    for (long long x = (long long)blockIdx.x * 256 + threadIdx.x; x < total; x += (long long)gridDim.x * 256) {
        const long long b = x / Dv;
        const int d = (int)(x - b * Dv);
        const VT g = dout[b * dout_ld + (long long)ds * Dv + d];
        VT* o = gout + b * gout_ld + (long long)vs * Dv + d;
        if (qs < 0) { *o = g; continue; }
        if (op_add) { o[0] = g; o[Dv] = g; continue; }
        const VT* sv = saved + b * saved_ld + (long long)qs * 2 * Dv + d;
        const VT sq = sv[0], sr = sv[Dv];
        o[0] = SplitOps<VT>::mul(g, sr);             // d/d(sum q) = dout * (sum r): what every q-lookup of the bag receives
        o[Dv] = SplitOps<VT>::mul(g, sq);
    }
}

// -------------------------------------------------------------------------------------------
// index split: the q and r id arrays of a QR table, same width as the ids.  A lookup the forward skips gets -1 / -1, which the update
// kernels skip in turn (and report)
// -------------------------------------------------------------------------------------------
struct IdxSplitArgs {
    const void* idx[DLRM_MAX_TABLES_PER_LAUNCH];
    void*       q[DLRM_MAX_TABLES_PER_LAUNCH];
    void*       r[DLRM_MAX_TABLES_PER_LAUNCH];
    long long   nnz[DLRM_MAX_TABLES_PER_LAUNCH];
    long long   n[DLRM_MAX_TABLES_PER_LAUNCH];
    long long   rows_q[DLRM_MAX_TABLES_PER_LAUNCH];
    int         coll[DLRM_MAX_TABLES_PER_LAUNCH];
};

template <typename IT>
__global__ __launch_bounds__(256) void emb_qr_split_indices_kernel(IdxSplitArgs a) {
    const int t = blockIdx.y;
    const IT* __restrict__ idx = (const IT*)a.idx[t];
    IT* __restrict__ qo = (IT*)a.q[t];
    IT* __restrict__ ro = (IT*)a.r[t];
    const long long nnz = a.nnz[t];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nnz; i += (long long)gridDim.x * 256) {
        long long q = -1, r = -1;
        if (!qr_split((long long)idx[i], a.n[t], a.coll[t], a.rows_q[t], &q, &r)) { q = -1; r = -1; }
        qo[i] = (IT)q; ro[i] = (IT)r;
    }
}

int emb_fwd_qr_impl(int T, int64_t B, int D, const void* const* weight_host, const void* const* weight_r_host,
                    const int64_t* rows_host, const int32_t* collisions_host, int op,
                    const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host, int idx_bits,
                    float* out, int64_t out_ld, float* saved, int64_t saved_ld, int64_t* err, DlrmPred pred, void* stream) {
    const int rc = emb_check_lists(T, B, D, weight_host, rows_host, indices_host, offsets_host, nnz_host, idx_bits, weight_r_host && collisions_host);
    if (rc) return rc;
    if (op != DLRM_QR_MULT && op != DLRM_QR_ADD) return DLRM_E_MODE;
    if (!out || out_ld < (int64_t)T * D) return DLRM_E_ARG;
    DLRM_REQUIRE(D <= 512, DLRM_E_RANGE, "embedding dimension above 512");
    int n_qr = 0;
    bool vec_ok = D % 4 == 0 && dlrm_aligned16(out) && out_ld % 4 == 0;
    for (int t = 0; t < T; ++t) {
        if (emb_check_table(t, weight_host, rows_host, indices_host, offsets_host, nnz_host) || collisions_host[t] < 0) return DLRM_E_ARG;
        if (collisions_host[t] > 0) { if (!weight_r_host[t]) return DLRM_E_ARG; ++n_qr; vec_ok = vec_ok && dlrm_aligned16(weight_r_host[t]); }
        vec_ok = vec_ok && dlrm_aligned16(weight_host[t]);
    }
    if (saved) {
        if (saved_ld < (int64_t)2 * n_qr * D) return DLRM_E_ARG;
        vec_ok = vec_ok && dlrm_aligned16(saved) && saved_ld % 4 == 0;
    }
    hipStream_t st = (hipStream_t)stream;
    int lpb = 0, nch = 0;
    if (vec_ok) {
        const int d4 = D / 4;
        lpb = lanes_per_bag(d4);
        nch = (d4 + lpb - 1) / lpb;                  // 1 or 2 (D <= 512)
    }
    constexpr int U = 2;
    int qslot = 0;
    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
        EmbArgs a;
        QrArgs qa = {};
        emb_fill_args(a, t0, n, weight_host, rows_host, indices_host, offsets_host, nnz_host, nullptr, err, pred);
        for (int k = 0; k < n; ++k) {
            const int t = t0 + k;
            const int c = collisions_host[t];
            qa.coll[k] = c;
            qa.wr[k] = c ? (const float*)weight_r_host[t] : nullptr;
            qa.rows_q[k] = c ? (rows_host[t] + c - 1) / c : rows_host[t];
            qa.qslot[k] = c ? qslot++ : 0;
        }
        dim3 block(256, 1, 1);
#define QR_FWD(LPB_, NCH_)                                                                                                              \
    do {                                                                                                                                \
        const int bpb = (256 / LPB_) * U;                                                                                               \
        dim3 grid((unsigned)((B + bpb - 1) / bpb), (unsigned)n, 1);                                                                     \
        if (idx_bits == 64) hipLaunchKernelGGL((emb_fwd_qr_kernel<LPB_, NCH_, long long, U>), grid, block, 0, st, a, qa, (long long)B, D, \
                                               op, out, (long long)out_ld, saved, (long long)saved_ld);                                 \
        else hipLaunchKernelGGL((emb_fwd_qr_kernel<LPB_, NCH_, int, U>), grid, block, 0, st, a, qa, (long long)B, D, op, out,           \
                                (long long)out_ld, saved, (long long)saved_ld);                                                         \
    } while (0)
        if (!vec_ok) {
            dim3 grid((unsigned)((B + 3) / 4), (unsigned)n, 1);
            if (idx_bits == 64) hipLaunchKernelGGL(emb_fwd_qr_scalar_kernel<long long>, grid, block, 0, st, a, qa, (long long)B, D, op, out,
                                                   (long long)out_ld, saved, (long long)saved_ld);
            else hipLaunchKernelGGL(emb_fwd_qr_scalar_kernel<int>, grid, block, 0, st, a, qa, (long long)B, D, op, out, (long long)out_ld,
                                    saved, (long long)saved_ld);
        } else if (nch == 2) QR_FWD(64, 2);
        else if (lpb == 4) QR_FWD(4, 1);
        else if (lpb == 8) QR_FWD(8, 1);
        else if (lpb == 16) QR_FWD(16, 1);
        else if (lpb == 32) QR_FWD(32, 1);
        else QR_FWD(64, 1);
#undef QR_FWD
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}

int emb_qr_bwd_split_impl(int T, int64_t B, int D, const int32_t* collisions_host, int op, const float* dout, int64_t dout_ld,
                          const float* saved, int64_t saved_ld, float* gout, int64_t gout_ld, DlrmPred pred, void* stream) {
    if (T <= 0 || B <= 0 || D <= 0 || !collisions_host || !dout || !gout) return DLRM_E_ARG;
    if (op != DLRM_QR_MULT && op != DLRM_QR_ADD) return DLRM_E_MODE;
    int n_qr = 0;
    for (int t = 0; t < T; ++t) { if (collisions_host[t] < 0) return DLRM_E_ARG; n_qr += collisions_host[t] > 0; }
    const int Tv = T + n_qr;
    if (dout_ld < (int64_t)T * D || gout_ld < (int64_t)Tv * D) return DLRM_E_ARG;
    if (op == DLRM_QR_MULT && n_qr > 0 && (!saved || saved_ld < (int64_t)2 * n_qr * D)) return DLRM_E_ARG;
    bool vec_ok = D % 4 == 0 && dlrm_aligned16(dout) && dlrm_aligned16(gout) && dout_ld % 4 == 0 && gout_ld % 4 == 0;
    if (op == DLRM_QR_MULT && n_qr > 0) vec_ok = vec_ok && dlrm_aligned16(saved) && saved_ld % 4 == 0;
    hipStream_t st = (hipStream_t)stream;
    int vslot = 0, qslot = 0;
    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
        SplitArgs sa = {};
        sa.pred = pred;
        for (int k = 0; k < n; ++k) {
            const int c = collisions_host[t0 + k];
            sa.slot[k] = t0 + k; sa.vslot[k] = vslot; sa.qslot[k] = c ? qslot++ : -1;
            vslot += c ? 2 : 1;
        }
        const int Dv = vec_ok ? D / 4 : D;
        long long nb = ((long long)B * Dv + 255) / 256; if (nb > 2048) nb = 2048;
        dim3 grid((unsigned)nb, (unsigned)n, 1), block(256, 1, 1);
        if (vec_ok)
            hipLaunchKernelGGL(emb_qr_bwd_split_kernel<float4>, grid, block, 0, st, sa, (long long)B, Dv, op, (const float4*)dout,
                               (long long)(dout_ld / 4), (const float4*)saved, (long long)(saved_ld / 4), (float4*)gout, (long long)(gout_ld / 4));
        else
            hipLaunchKernelGGL(emb_qr_bwd_split_kernel<float>, grid, block, 0, st, sa, (long long)B, Dv, op, dout, (long long)dout_ld, saved,
                               (long long)saved_ld, gout, (long long)gout_ld);
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

extern "C" int dlrm_emb_fwd_qr(int T, int64_t B, int D, const void* const* weight_host, const void* const* weight_r_host,
                               const int64_t* rows_host, const int32_t* collisions_host, int op,
                               const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host, int idx_bits,
                               float* out, int64_t out_ld, float* saved, int64_t saved_ld, int64_t* err, void* stream) {
    return emb_fwd_qr_impl(T, B, D, weight_host, weight_r_host, rows_host, collisions_host, op, indices_host, offsets_host, nnz_host, idx_bits,
                           out, out_ld, saved, saved_ld, err, DlrmPred{nullptr, 0}, stream);
}

// dlrm_emb_fwd_qr behind a launch predicate (common.h DlrmPred): the same kernels, whose workgroups return at once unless
// (*pred_flag != 0) == (pred_nonzero != 0)
extern "C" int dlrm_emb_fwd_qr_pred(int T, int64_t B, int D, const void* const* weight_host, const void* const* weight_r_host,
                                    const int64_t* rows_host, const int32_t* collisions_host, int op,
                                    const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host, int idx_bits,
                                    float* out, int64_t out_ld, float* saved, int64_t saved_ld, int64_t* err,
                                    const int32_t* pred_flag, int pred_nonzero, void* stream) {
    return emb_fwd_qr_impl(T, B, D, weight_host, weight_r_host, rows_host, collisions_host, op, indices_host, offsets_host, nnz_host, idx_bits,
                           out, out_ld, saved, saved_ld, err, DlrmPred{(const int*)pred_flag, pred_nonzero}, stream);
}

extern "C" int dlrm_emb_qr_bwd_split(int T, int64_t B, int D, const int32_t* collisions_host, int op, const float* dout, int64_t dout_ld,
                                     const float* saved, int64_t saved_ld, float* gout, int64_t gout_ld, void* stream) {
    return emb_qr_bwd_split_impl(T, B, D, collisions_host, op, dout, dout_ld, saved, saved_ld, gout, gout_ld, DlrmPred{nullptr, 0}, stream);
}

extern "C" int dlrm_emb_qr_bwd_split_pred(int T, int64_t B, int D, const int32_t* collisions_host, int op, const float* dout,
                                          int64_t dout_ld, const float* saved, int64_t saved_ld, float* gout, int64_t gout_ld,
                                          const int32_t* pred_flag, int pred_nonzero, void* stream) {
    return emb_qr_bwd_split_impl(T, B, D, collisions_host, op, dout, dout_ld, saved, saved_ld, gout, gout_ld,
                                 DlrmPred{(const int*)pred_flag, pred_nonzero}, stream);
}

extern "C" int dlrm_emb_qr_split_indices(int T, const int64_t* rows_host, const int32_t* collisions_host, const void* const* indices_host,
                                         const int64_t* nnz_host, int idx_bits, void* const* q_out_host, void* const* r_out_host,
                                         void* stream) {
    if (T <= 0 || !rows_host || !collisions_host || !indices_host || !nnz_host || !q_out_host || !r_out_host) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    hipStream_t st = (hipStream_t)stream;
    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
        IdxSplitArgs a = {};
        long long max_nnz = 0;
        for (int k = 0; k < n; ++k) {
            const int t = t0 + k;
            const int c = collisions_host[t];
            if (c <= 0 || rows_host[t] <= 0 || nnz_host[t] < 0) return DLRM_E_ARG;
            if (nnz_host[t] > 0 && (!indices_host[t] || !q_out_host[t] || !r_out_host[t])) return DLRM_E_ARG;
            a.idx[k] = indices_host[t]; a.q[k] = q_out_host[t]; a.r[k] = r_out_host[t];
            a.nnz[k] = nnz_host[t]; a.n[k] = rows_host[t]; a.rows_q[k] = (rows_host[t] + c - 1) / c; a.coll[k] = c;
            if (nnz_host[t] > max_nnz) max_nnz = nnz_host[t];
        }
        if (max_nnz == 0) continue;
        long long nb = (max_nnz + 255) / 256; if (nb > 1024) nb = 1024;
        dim3 grid((unsigned)nb, (unsigned)n, 1), block(256, 1, 1);
        if (idx_bits == 64) hipLaunchKernelGGL(emb_qr_split_indices_kernel<long long>, grid, block, 0, st, a);
        else                hipLaunchKernelGGL(emb_qr_split_indices_kernel<int>, grid, block, 0, st, a);
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}
