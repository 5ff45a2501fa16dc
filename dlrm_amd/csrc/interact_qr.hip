// interact_qr.hip — fused lookup + pairwise-dot interaction, forward AND backward, over quotient-remainder (QR) embedding tables, gfx950.
//
// Replaces, for batches with ONE lookup per bag: dlrm_emb_fwd_qr + dlrm_interact_fwd (forward) and dlrm_interact_bwd over the pooled
//   [B, T*D] fp32 buffer + dlrm_emb_qr_bwd_split (backward).  Neither that buffer, nor its gradient, nor the [B, 2*Tq*D] pooled sums the
//   two-kernel forward keeps for its backward are written or read, and nothing has to live from forward to backward except x: the backward
//   fetches the weight_q / weight_r rows again.  A table list may mix QR tables (collisions > 0) and plain fp32 tables (collisions == 0).
//
// Contract (include/dlrm_hip.h):
//   forward : R is BIT-IDENTICAL to dlrm_emb_fwd_qr (saved = NULL) into a feature buffer + dlrm_interact_fwd, modes 0 / 1 / 2;
//   backward: dx is BIT-IDENTICAL to dlrm_interact_bwd over (x, that buffer), gout [B, Tv*D] to dlrm_emb_qr_bwd_split applied to that call's
//             embedding gradient and the sums the forward would have saved (virtual table list: q then r for a QR table, Tv = T + Tq).
//   * element = fmaf(1, Wq[q], +0) op fmaf(1, Wr[r], +0), op = * or +, each rounded once — the lookup's arithmetic from zero accumulators
//     (emb_qr.hip), so -0.0 in a table row becomes +0.0 before the composition; fmaf(1, W[id], +0) for a plain table.  q, r: qr_split
//     (qr_split.h, shared with emb_qr.hip: the FLOAT32 quotient).  A lookup emb_fwd_qr skips gives a row of +0.0 and is reported; its gout
//     rows are dout * (+0) (MULT) / dout (ADD), as the two-kernel form writes them;
//   * products = the summation order of the D = 128 interaction kernels (interact.hip): the kernels are gather_pipeline.h's, which compose
//     the rows into the LDS image of interact_{fwd,bwd}_dma_kernel and run those kernels' multiply sections on it.
//
// Row fetch: an fp32 row of D = 128 is 512 bytes; a lane owns 4 columns = ONE 16-byte load, 32 lanes cover a row, a wave fetches 2 rows per
//   pass, ceil((F - 1) / 2) <= 13 passes per sample; a QR row costs a second load, of weight_r, which is c rows (2 KiB at c = 4) and is read
//   through the caches like emb_qr.hip does — nothing is staged, so no shape depends on c.  Lane f (1 <= f < F) owns feature f's selector:
//   it loads idx[f][s] and off[f][s], checks them, splits the id and hands q and r to the 32 lanes of that row by lane shuffle.
//
// Backward, the virtual table list: the interaction kernel's row store of feature f goes to the q slot of table f - 1 in gout.  ADD: the same
//   row is stored a second time D columns further (the r slot).  MULT: interact_qr_mult_kernel, a second launch of the same call behind
//   the same predicate, gathers Wq[q] and Wr[r] again (half a wave per sample and table) and turns the row in place into dout * sr | dout * sq.
//   Keeping both components of every row in LDS beside the composed image instead would double the images: 281 KiB at F > 16, more than
//   the 160 KiB of a CU.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, 64-bit ids / 32-bit ids where they differ; no static
//   LDS, the dynamic LDS of a workgroup is what gather_lds<QrSource>() returns):
//                                            VGPRs      AGPRs      SGPRs  scratch  dynamic LDS
//   gather_fwd_kernel<QrSource, 1, IT>     202 / 204      8         106      0      67328 B   (F <= 16: two workgroups per CU)
//   gather_fwd_kernel<QrSource, 2, IT>     256         88 / 90      106      0     132864 B   (one workgroup per CU)
//   gather_bwd_kernel<QrSource, 1, IT>     221           16         106      0      83712 B   (F <= 16: one workgroup per CU)
//   gather_bwd_kernel<QrSource, 2, IT>     256          132         106      0     149248 B   (one workgroup per CU)
//   interact_qr_mult_kernel<IT>             30 / 28       0        44 / 36   0          0 B
//   One wave per SIMD may use 512 registers (the NB = 2 instantiations keep the 104 row registers of the next sample partly in AGPRs), so
//   registers limit no launch; LDS bounds the workgroups per CU, as the last column says.
#include "gather_pipeline.h"
#include "gather_qr.h"

namespace {

constexpr int BI_SRCB = BI_D * 4;           // bytes of a table row (fp32)

struct QrSource {
    using Args = QrArgs;
    using Row = QrRow;                      // gather_qr.h: the argument block, the LDS tables and the index split, shared with the narrow kernels
    static constexpr int NTAB = QR_NTAB;
    static constexpr bool DUP = true;
    static constexpr int passes(int nb) { return nb == 1 ? 8 : 13; }     // rows 1 .. 16 NB - 1 (F <= 27), two per pass

    template <int NP>
    struct Lane {
        const gchar* base[NP];      // the lane's 16 bytes of row 0 of weight_q (plain: of the table) behind image row 1 + 2 p + (lane >> 5)
        const gchar* baser[NP];     // the same of weight_r
        unsigned wofs[NP];          // byte offset of the lane's 16-byte slot inside the image
        bool on[NP];                // that row is a feature (< F)
        bool qr[NP];                // ... of a QR table
        const gchar* qsrc;          // lanes 1 .. F - 1: idx / off of feature `lane`
        const gchar* osrc;
        long long rows, rows_q;
        int coll;
        bool own;
    };
    // the rows of one sample, as loaded: weight_q (or the plain table) and weight_r, one 16-byte quad per lane and pass
    template <int NP> struct Regs { floatx4 q[NP], r[NP]; };

    static __device__ __forceinline__ void args_to_lds(const Args& ba, long long* tab, int F) { qr_args_to_lds(ba, tab, F); }

    template <int NP>
    static __device__ __forceinline__ void lane_init(Lane<NP>& bl, const long long* tab, int F, int lane) {
        const int g = lane >> 5, li = lane & 31;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int row = 1 + 2 * p + g;
            bl.on[p] = row < F;                                   // no lane loads a row for a feature slot >= F
            bl.qr[p] = bl.on[p] && (int)(tab[6 * GC_MAXF + row] & 0xFFFFFFFFLL) != 0;
            bl.base[p] = bl.on[p] ? (const gchar*)tab[0 * GC_MAXF + row] + 16 * li : nullptr;
            bl.baser[p] = bl.qr[p] ? (const gchar*)tab[1 * GC_MAXF + row] + 16 * li : nullptr;
            bl.wofs[p] = row * BI_ROWB + ((li ^ (row & 15)) * 16);
        }
        bl.own = lane >= 1 && lane < F;
        bl.qsrc = bl.own ? (const gchar*)tab[2 * GC_MAXF + lane] : nullptr;
        bl.osrc = bl.own ? (const gchar*)tab[3 * GC_MAXF + lane] : nullptr;
        bl.rows = bl.own ? tab[4 * GC_MAXF + lane] : 0;
        bl.rows_q = bl.own ? tab[5 * GC_MAXF + lane] : 0;
        bl.coll = bl.own ? (int)(tab[6 * GC_MAXF + lane] & 0xFFFFFFFFLL) : 0;
    }

    // the owner lane's checks and the index split (gather_qr.h)
    template <typename IT, int NP>
    static __device__ __forceinline__ Row sel_resolve(const Lane<NP>& bl, const Sel<IT>& sel, long long s, int lane, long long* err, bool live) {
        return qr_sel_resolve<IT>(bl, sel, s, lane, err, live);
    }

    // row loads of one sample into registers: NP passes, two rows per pass, nothing waits here.  weight_r is c rows: it stays in the caches
    template <int NP>
    static __device__ __forceinline__ void rows_issue(Regs<NP>& v, const Lane<NP>& bl, const Row& sel, int lane) {
        const int g = lane >> 5;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const unsigned mq = (unsigned)__shfl((int)sel.q, 1 + 2 * p + g, 64);      // (1 + 2 p + g <= 26: always a lane of this wave)
            const unsigned mr = (unsigned)__shfl((int)sel.r, 1 + 2 * p + g, 64);
            v.q[p] = (floatx4){0.f, 0.f, 0.f, 0.f};
            v.r[p] = (floatx4){0.f, 0.f, 0.f, 0.f};
            if (bl.on[p] && mq != GC_BAD) {
                v.q[p] = *(const gfloatx4*)(bl.base[p] + (unsigned long long)mq * BI_SRCB);       // 64-bit byte offset
                if (bl.qr[p]) v.r[p] = *(const gfloatx4*)(bl.baser[p] + (unsigned long long)mr * BI_SRCB);
            }
        }
    }

    // compose and write: sq = 0 + Wq[q], sr = 0 + Wr[r], one multiply / add — dlrm_emb_fwd_qr's element for a bag of one lookup (a skipped
    // lookup is 0 * 0 or 0 + 0 = +0)
    template <int NP>
    static __device__ __forceinline__ void image_write(char* img, const Regs<NP>& v, const Lane<NP>& bl, const float4& xv, int lane, const Args& ba) {
        if (lane < 32) *(float4*)(img + 16 * lane) = xv;                    // row 0: (row & 15) == 0, slot = quad
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (bl.on[p]) {
                float4 y = bag1(v.q[p]);
                if (bl.qr[p]) {
                    const float4 sr = bag1(v.r[p]);
                    if (ba.op_add) y = make_float4(y.x + sr.x, y.y + sr.y, y.z + sr.z, y.w + sr.w);
                    else           y = make_float4(y.x * sr.x, y.y * sr.y, y.z * sr.z, y.w * sr.w);
                }
                *(float4*)(img + bl.wofs[p]) = y;
            }
        }
    }

    // the interaction kernel's row store of feature i goes to the VIRTUAL slot of table i - 1 in gout: the q component of a QR table.  ADD:
    // the r component, D columns further, gets the same row (dup); MULT: interact_qr_mult_kernel multiplies in place afterwards
    static __device__ __forceinline__ long long dst_slot(const Args& ba, const long long* tab, int i, int F, bool& dup) {
        const long long cv = (i >= 1 && i < F) ? tab[6 * GC_MAXF + i] : 0;           // coll | vs << 32
        dup = ba.op_add && (int)(cv & 0xFFFFFFFFLL) != 0;
        return cv >> 32;
    }
};

// -------------------------------------------------------------------------------------------
// backward, MULT: gout[b, v] = dout * sr, gout[b, v + 1] = dout * sq, in place over the dout rows gather_bwd_kernel left in the q
// slots.  The two rows are gathered again (weight_q from HBM / L2, weight_r from the caches); no selector is reported twice.  Half a wave
// per (sample, table), a 16-byte quad per lane; blockIdx.y = feature - 1.
// -------------------------------------------------------------------------------------------
template <typename IT>
__global__ __launch_bounds__(256) void interact_qr_mult_kernel(QrArgs ba, long long B, float* __restrict__ gout, long long gout_ld) {
    if (ba.pred.skip()) return;
    const int f = 1 + blockIdx.y;                       // workgroup-uniform: the kernarg tables are read with scalar loads
    const int c = ba.coll[f];
    if (c == 0) return;                                 // a plain table: its row is final
    const IT* __restrict__ idx = (const IT*)ba.idx[f];
    const gchar* Wq = (const gchar*)ba.w[f];
    const gchar* Wr = (const gchar*)ba.wr[f];
    const long long n = ba.rows[f], rows_q = ba.rows_q[f];
    const int li = threadIdx.x & 31;
    const long long step = (long long)gridDim.x * 8;
    for (long long b = (long long)blockIdx.x * 8 + (threadIdx.x >> 5); b < B; b += step) {
        long long q = 0, r = 0;
        const bool ok = qr_split((long long)idx[b], n, c, rows_q, &q, &r);
        floatx4 vq = (floatx4){0.f, 0.f, 0.f, 0.f}, vr = vq;          // a skipped lookup: the sums are +0
        if (ok) {
            vq = *(const gfloatx4*)(Wq + (unsigned long long)q * BI_SRCB + 16 * li);
            vr = *(const gfloatx4*)(Wr + (unsigned long long)r * BI_SRCB + 16 * li);
        }
        float* o = gout + b * gout_ld + (long long)ba.vs[f] * BI_D + 4 * li;
        const float4 d = *(const float4*)o;
        const float4 sq = bag1(vq), sr = bag1(vr);
        *(float4*)o = make_float4(d.x * sr.x, d.y * sr.y, d.z * sr.z, d.w * sr.w);
        *(float4*)(o + BI_D) = make_float4(d.x * sq.x, d.y * sq.y, d.z * sq.z, d.w * sq.w);
    }
}

}  // namespace

extern "C" int dlrm_interact_gather_qr_ok(int F, int D) {
    return (D == BI_D && F < GC_MAXF && dlrm_interact_gather_ok(F, D)) ? 1 : 0;
}

extern "C" int dlrm_interact_fwd_gather_qr(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                           const void* const* weight_host, const void* const* weight_r_host, const int64_t* rows_host,
                                           const int32_t* collisions_host, int op,
                                           const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                           int self_interaction, float* R, int64_t ldr, int64_t* err,
                                           const int32_t* pred_flag, int pred_nonzero, void* stream) {
    if (op != DLRM_QR_MULT && op != DLRM_QR_ADD) return DLRM_E_ARG;
    QrArgs ba;
    ba.op_add = op == DLRM_QR_ADD;
    int n_qr = 0;
    const int rc = gather_check_fwd(B, F, D, x, x_ld, weight_host && weight_r_host && rows_host && collisions_host && index_host && offsets_host,
                                    idx_bits, dlrm_interact_gather_qr_ok(F, D), self_interaction, R, ldr, [&] {
        return fill_args(ba, F, weight_host, weight_r_host, rows_host, collisions_host, index_host, offsets_host, err, pred_flag, pred_nonzero,
                         &n_qr);
    });
    if (rc) return rc;
    gather_fwd<QrSource>(ba, x, x_ld, B, F, self_interaction & 3, R, ldr, idx_bits, (hipStream_t)stream);
    DLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int dlrm_interact_bwd_gather_qr(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                           const void* const* weight_host, const void* const* weight_r_host, const int64_t* rows_host,
                                           const int32_t* collisions_host, int op,
                                           const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                           int self_interaction, const float* dR, int64_t ldr,
                                           float* dx, int64_t dx_ld, float* gout, int64_t gout_ld, int64_t* err,
                                           const int32_t* pred_flag, int pred_nonzero, void* stream) {
    if (op != DLRM_QR_MULT && op != DLRM_QR_ADD) return DLRM_E_ARG;
    QrArgs ba;
    ba.op_add = op == DLRM_QR_ADD;
    int n_qr = 0;
    const int rc = gather_check_bwd(B, F, D, x, x_ld,
                                    weight_host && weight_r_host && rows_host && collisions_host && index_host && offsets_host && gout, idx_bits,
                                    dlrm_interact_gather_qr_ok(F, D), self_interaction, dR, ldr, dx, dx_ld, gout, gout_ld, INT64_MIN, BI_DRB, [&] {
        const int frc = fill_args(ba, F, weight_host, weight_r_host, rows_host, collisions_host, index_host, offsets_host, err, pred_flag,
                                  pred_nonzero, &n_qr);
        if (frc) return frc;
        return (F > 1 && gout_ld < (int64_t)(F - 1 + n_qr) * D) ? (int)DLRM_E_ARG : 0;      // the virtual table list: Tv = T + Tq
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    gather_bwd<QrSource>(ba, x, x_ld, B, F, self_interaction & 7, dR, ldr, dx, dx_ld, gout, gout_ld, idx_bits, st);
    DLRM_LAUNCH_CHECK();
    if (!ba.op_add && n_qr > 0) {
        long long nb = (B + 7) / 8; if (nb > 4096) nb = 4096;
        dim3 grid((unsigned)nb, (unsigned)(F - 1), 1), block(256, 1, 1);
        if (idx_bits == 64) hipLaunchKernelGGL(interact_qr_mult_kernel<long long>, grid, block, 0, st, ba, (long long)B, gout, (long long)gout_ld);
        else                hipLaunchKernelGGL(interact_qr_mult_kernel<int>, grid, block, 0, st, ba, (long long)B, gout, (long long)gout_ld);
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}
