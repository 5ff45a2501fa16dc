// interact_narrow_qr.hip — the fused lookup + pairwise-dot interaction kernels of interact_narrow.h over quotient-remainder (QR) embedding
// tables, forward AND backward, D = 16 / 32 / 64, gfx950.  The D = 128 form is interact_qr.hip.
//
// Replaces, for batches with ONE lookup per bag: dlrm_emb_fwd_qr + dlrm_interact_fwd (forward) and dlrm_interact_bwd over the pooled
//   [B, T*D] buffer + dlrm_emb_qr_bwd_split (backward) at the widths where the interaction kernels are the GENERIC ones.  Neither that
//   buffer, nor its gradient, nor the [B, 2*Tq*D] pooled sums the two-kernel forward keeps for its backward are written or read: nothing
//   lives from forward to backward except x, the backward fetches the weight_q / weight_r rows again.  A table list may mix QR tables
//   (collisions > 0) and plain fp32 tables (collisions == 0).
//
// Contract (include/dlrm_hip.h): R, dx and gout [B, Tv*D] are BIT-IDENTICAL to the two-kernel form (virtual table list: q then r for a QR
//   table, Tv = T + Tq).  Geometry, pipeline, MFMA order and stores are those of interact_narrow.hip (the kernels are the same templates);
//   QrRows changes the selector and the row source in front of image_write:
//   * selector: the owner lane of feature f loads idx[f][s] and off[f][s], checks them, splits the id (qr_split: the FLOAT32 quotient,
//     rows_q = ceil(n / c)) and hands q (GC_BAD: the zero row) and r to the D/4 lanes of that row by lane shuffle.  A lookup dlrm_emb_fwd_qr
//     skips (id outside [0, n), quotient >= rows_q) is reported as {1, table, id, n} and selects the zero row;
//   * rows: a lane's 4 columns of weight_q (or of a plain table) are ONE 16-byte load; a QR table costs a second 16-byte load of weight_r[r],
//     which is c rows and is read through the caches — nothing is staged, so no shape depends on c.  Row byte offsets are 64-bit;
//   * element = fmaf(1, Wq[q], +0) op fmaf(1, Wr[r], +0), op = * or +, each rounded once — emb_qr.hip's arithmetic from zero accumulators,
//     so -0.0 in a table row becomes +0.0 before the composition; fmaf(1, W[id], +0) for a plain table.
//
// Backward, the virtual table list: the interaction kernel's row store of feature f goes to the q slot of table f - 1 in gout (dst_slot).
//   ADD: the same registers are stored a second time D columns further, the r slot (DUP).  MULT: the q slot needs dout * sr and the r slot
//   dout * sq, and sq / sr have to reach the storing lane, which holds D/16 adjacent columns of rows 4 g + q — not the columns it fetched.
//   Chosen: a SECOND LAUNCH inside the same call, behind the same predicate (interact_narrow_qr_mult_kernel: D/4 lanes per (sample, table)
//   gather Wq[q] and Wr[r] again and turn the row in place into dout * sr | dout * sq), as interact_qr_mult_kernel does at D = 128.
//   Reason: it leaves everything behind image_write — LDS layout, fragment reads, the store section — and the LDS footprint of the shared
//   kernels untouched, so the fp32 / bf16 / packed instantiations and this one stay the same code; the alternative, two unpadded
//   single-buffered component images per wave beside the composed one, takes the D = 64, NB = 2 backward from 95232 B to 160768 B of the
//   163840 B a workgroup may have, adds a second and third LDS read per stored element with bank conflicts on the unpadded rows, and is
//   sound only while the component reads stay in front of the next sample's image_write.  The second launch re-reads B * Tq * D * 4 bytes
//   of gout and the weight_q rows, which at these widths are mostly L2 hits (they were fetched by the launch before).  The LDS route was
//   not built, so there is no measurement of it; what the chosen route costs against the two-kernel form is in
//   profiles/narrow_interact/fused_rates_qr.md.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no static LDS; the dynamic LDS of a workgroup is
//   narrow_lds(bwd, QR_NTAB): the fp32 kernels' plus 768 B for the three further kernarg tables).  Scratch is 0 everywhere.
//                                                       VGPRs (int / long long ids)  AGPRs  SGPRs  scratch  dynamic LDS
//   interact_fwd_narrow_kernel<QrRows, 16, 1, IT>         70 /  72                  8    106      0      12032 B
//   interact_fwd_narrow_kernel<QrRows, 16, 2, IT>        111 / 109                 24    106      0      22272 B
//   interact_fwd_narrow_kernel<QrRows, 32, 1, IT>         87 /  85                  8    106      0      20224 B
//   interact_fwd_narrow_kernel<QrRows, 32, 2, IT>        137 / 135                 24    106      0      38656 B
//   interact_fwd_narrow_kernel<QrRows, 64, 1, IT>        121 / 119                  8    106      0      36608 B
//   interact_fwd_narrow_kernel<QrRows, 64, 2, IT>        205 / 203                 24    106      0      71424 B
//   interact_bwd_narrow_kernel<QrRows, 16, 1, IT>         89 /  89                  8    106      0      20224 B
//   interact_bwd_narrow_kernel<QrRows, 16, 2, IT>        163 / 163                  8    106      0      46848 B
//   interact_bwd_narrow_kernel<QrRows, 32, 1, IT>        116 / 114                 16    106      0      28416 B
//   interact_bwd_narrow_kernel<QrRows, 32, 2, IT>        199 / 199                 16    106      0      63232 B
//   interact_bwd_narrow_kernel<QrRows, 64, 1, IT>        158 / 156                 32    106      0      44800 B
//   interact_bwd_narrow_kernel<QrRows, 64, 2, IT>        256 / 256                 62    106      0      96000 B   (one workgroup per CU)
//   interact_narrow_qr_mult_kernel<D, IT>, every D        28 /  30                  0   36 / 44    0          0 B
//   A lane keeps two 16-byte quads per pass (weight_q, weight_r) and two base pointers, which is what the figures above the fp32 kernels'
//   are.  At two workgroups per CU a wave may use 256 registers, VGPRs and AGPRs together: the widest such launch (forward, D = 64, NB = 2)
//   has 229; the D = 64, NB = 2 backward runs one workgroup per CU, as its fp32 sibling, where a wave may use 512.
#include "interact_narrow.h"
#include "gather_qr.h"

namespace {

// what a lane keeps across the sample loop (NLane plus the weight_r side)
template <int NP>
struct QrLane {
    const gchar* base[NP];      // the lane's 16 bytes of row 0 of weight_q (plain: of the table) behind image row 1 + RPP p + lane / LPR
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

// fp32 rows of QR tables: the row source AND the selector side
struct QrRows {
    using Args = QrArgs;
    using Row = QrRow;
    static constexpr int NTAB = QR_NTAB;
    static constexpr bool DUP = true;
    static constexpr unsigned long long pitch(int D) { return 4ull * D; }
    template <int NP> using Lane = QrLane<NP>;
    struct Regs { floatx4 q, r; };              // weight_q (or the plain table) and weight_r, one 16-byte quad per lane and pass
    static __device__ __forceinline__ Row none() { Row o; o.q = GC_BAD; o.r = 0u; return o; }

    static __device__ __forceinline__ void tables_to_lds(const Args& ba, long long* tab, int F) { qr_args_to_lds(ba, tab, F); }

    template <typename S, int D, int NB, int NP>
    static __device__ __forceinline__ void lane_init(QrLane<NP>& nl, const long long* tab, int F, int lane) {
        using G = NGeom<D, NB>;
        const int rg = lane / G::LPR, lc = lane % G::LPR;
#pragma unroll
        for (int p = 0; p < G::NP; ++p) {
            const int row = 1 + G::RPP * p + rg;
            nl.on[p] = row < F;                                   // no lane loads or writes a row for a feature slot >= F
            nl.qr[p] = nl.on[p] && (int)(tab[6 * GC_MAXF + row] & 0xFFFFFFFFLL) != 0;
            nl.base[p] = nl.on[p] ? (const gchar*)tab[0 * GC_MAXF + row] + 16 * lc : nullptr;
            nl.baser[p] = nl.qr[p] ? (const gchar*)tab[1 * GC_MAXF + row] + 16 * lc : nullptr;
            nl.wofs[p] = nl.on[p] ? (unsigned)(row * G::LS * 4 + 16 * lc) : 0u;
        }
        nl.own = lane >= 1 && lane < F;
        nl.qsrc = nl.own ? (const gchar*)tab[2 * GC_MAXF + lane] : nullptr;
        nl.osrc = nl.own ? (const gchar*)tab[3 * GC_MAXF + lane] : nullptr;
        nl.rows = nl.own ? tab[4 * GC_MAXF + lane] : 0;
        nl.rows_q = nl.own ? tab[5 * GC_MAXF + lane] : 0;
        nl.coll = nl.own ? (int)(tab[6 * GC_MAXF + lane] & 0xFFFFFFFFLL) : 0;
    }

    template <typename IT, int NP>
    static __device__ __forceinline__ Row resolve(const QrLane<NP>& nl, const Sel<IT>& sel, long long s, int lane, long long* err) {
        return qr_sel_resolve<IT>(nl, sel, s, lane, err, true);
    }

    // row loads of one sample into registers: NP passes, nothing waits here.  weight_r is c rows: it stays in the caches
    template <typename S, int D, int NB, int NP>
    static __device__ __forceinline__ void rows_issue(Regs (&v)[NP], const QrLane<NP>& nl, const Row& sel, int lane) {
        using G = NGeom<D, NB>;
        const int rg = lane / G::LPR;
#pragma unroll
        for (int p = 0; p < G::NP; ++p) {
            const int src = (1 + G::RPP * p + rg) & 63;                    // (rows that are features are < 32: a lane of this wave)
            const unsigned mq = (unsigned)__shfl((int)sel.q, src, 64);
            const unsigned mr = (unsigned)__shfl((int)sel.r, src, 64);
            v[p].q = (floatx4){0.f, 0.f, 0.f, 0.f};
            v[p].r = (floatx4){0.f, 0.f, 0.f, 0.f};
            if (nl.on[p] && mq != GC_BAD) {
                v[p].q = *(const gfloatx4*)(nl.base[p] + (unsigned long long)mq * pitch(D));       // 64-bit byte offset
                if (nl.qr[p]) v[p].r = *(const gfloatx4*)(nl.baser[p] + (unsigned long long)mr * pitch(D));
            }
        }
    }

    // compose and write: sq = 0 + Wq[q], sr = 0 + Wr[r], one multiply / add — dlrm_emb_fwd_qr's element for a bag of one lookup (a skipped
    // lookup is 0 * 0 or 0 + 0 = +0)
    template <typename S, int D, int NB, int NP>
    static __device__ __forceinline__ void image_write(char* img, const Regs (&v)[NP], const QrLane<NP>& nl, const float4& xv, int lane,
                                                       const Args& ba) {
        using G = NGeom<D, NB>;
        if (lane < G::LPR) *(float4*)(img + 16 * lane) = xv;                // row 0
#pragma unroll
        for (int p = 0; p < G::NP; ++p) {
            if (nl.on[p]) {
                float4 y = bag1(v[p].q);
                if (nl.qr[p]) {
                    const float4 sr = bag1(v[p].r);
                    if (ba.op_add) y = make_float4(y.x + sr.x, y.y + sr.y, y.z + sr.z, y.w + sr.w);
                    else           y = make_float4(y.x * sr.x, y.y * sr.y, y.z * sr.z, y.w * sr.w);
                }
                *(float4*)(img + nl.wofs[p]) = y;
            }
        }
    }

    // the row store of feature i goes to the VIRTUAL slot of table i - 1 in gout: the q component of a QR table.  ADD: the r component,
    // D columns further, gets the same row (dup); MULT: interact_narrow_qr_mult_kernel multiplies in place afterwards
    static __device__ __forceinline__ long long dst_slot(const Args& ba, const long long* tab, int i, int F, bool& dup) {
        const long long cv = (i >= 1 && i < F) ? tab[6 * GC_MAXF + i] : 0;           // coll | vs << 32
        dup = ba.op_add && (int)(cv & 0xFFFFFFFFLL) != 0;
        return cv >> 32;
    }
};

// -------------------------------------------------------------------------------------------
// backward, MULT: gout[b, v] = dout * sr, gout[b, v + 1] = dout * sq, in place over the dout rows interact_bwd_narrow_kernel left in the q
// slots.  The two rows are gathered again (weight_q from L2 / HBM, weight_r from the caches); no selector is reported twice.  D/4 lanes
// per (sample, table), a 16-byte quad per lane; blockIdx.y = feature - 1.
// -------------------------------------------------------------------------------------------
template <int D, typename IT>
__global__ __launch_bounds__(256) void interact_narrow_qr_mult_kernel(QrArgs ba, long long B, float* __restrict__ gout, long long gout_ld) {
    if (ba.pred.skip()) return;
    constexpr int LPR = D / 4, SPB = 256 / LPR;         // lanes per row, samples of a workgroup per step
    const int f = 1 + blockIdx.y;                       // workgroup-uniform: the kernarg tables are read with scalar loads
    const int c = ba.coll[f];
    if (c == 0) return;                                 // a plain table: its row is final
    const IT* __restrict__ idx = (const IT*)ba.idx[f];
    const gchar* Wq = (const gchar*)ba.w[f];
    const gchar* Wr = (const gchar*)ba.wr[f];
    const long long n = ba.rows[f], rows_q = ba.rows_q[f];
    const int lc = threadIdx.x % LPR;
    const long long step = (long long)gridDim.x * SPB;
    for (long long b = (long long)blockIdx.x * SPB + threadIdx.x / LPR; b < B; b += step) {
        long long q = 0, r = 0;
        const bool ok = qr_split((long long)idx[b], n, c, rows_q, &q, &r);
        floatx4 vq = (floatx4){0.f, 0.f, 0.f, 0.f}, vr = vq;          // a skipped lookup: the sums are +0
        if (ok) {
            vq = *(const gfloatx4*)(Wq + (unsigned long long)q * (4ull * D) + 16 * lc);
            vr = *(const gfloatx4*)(Wr + (unsigned long long)r * (4ull * D) + 16 * lc);
        }
        float* o = gout + b * gout_ld + (long long)ba.vs[f] * D + 4 * lc;
        const float4 d = *(const float4*)o;
        const float4 sq = bag1(vq), sr = bag1(vr);
        *(float4*)o = make_float4(d.x * sr.x, d.y * sr.y, d.z * sr.z, d.w * sr.w);
        *(float4*)(o + D) = make_float4(d.x * sq.x, d.y * sq.y, d.z * sq.z, d.w * sq.w);
    }
}

template <int D, typename IT>
void launch_mult(const QrArgs& ba, long long B, int F, float* gout, long long gout_ld, hipStream_t st) {
    constexpr int SPB = 256 / (D / 4);
    long long nb = (B + SPB - 1) / SPB; if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL((interact_narrow_qr_mult_kernel<D, IT>), dim3((unsigned)nb, (unsigned)(F - 1), 1), dim3(256, 1, 1), 0, st, ba, B, gout, gout_ld);
}

}  // namespace

extern "C" int dlrm_interact_gather_narrow_qr_ok(int F, int D) {
    return dlrm_interact_gather_narrow_ok(F, D);
}

extern "C" int dlrm_interact_fwd_gather_narrow_qr(int64_t B, int F, int D, const float* x, int64_t x_ld,
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
                                    idx_bits, dlrm_interact_gather_narrow_qr_ok(F, D), self_interaction, R, ldr, [&] {
        return fill_args(ba, F, weight_host, weight_r_host, rows_host, collisions_host, index_host, offsets_host, err, pred_flag, pred_nonzero,
                         &n_qr);
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 3;
    NARROW_DISPATCH(launch_fwd, QrRows, ba, x, (long long)x_ld, (long long)B, F, self, R, (long long)ldr, st);
    DLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int dlrm_interact_bwd_gather_narrow_qr(int64_t B, int F, int D, const float* x, int64_t x_ld,
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
                                    dlrm_interact_gather_narrow_qr_ok(F, D), self_interaction, dR, ldr, dx, dx_ld, gout, gout_ld, INT64_MIN, 0, [&] {
        const int frc = fill_args(ba, F, weight_host, weight_r_host, rows_host, collisions_host, index_host, offsets_host, err, pred_flag,
                                  pred_nonzero, &n_qr);
        if (frc) return frc;
        return (F > 1 && gout_ld < (int64_t)(F - 1 + n_qr) * D) ? (int)DLRM_E_ARG : 0;      // the virtual table list: Tv = T + Tq
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 7;
    NARROW_DISPATCH(launch_bwd, QrRows, ba, x, (long long)x_ld, (long long)B, F, self, dR, (long long)ldr, dx, (long long)dx_ld, gout,
                    (long long)gout_ld, st);
    DLRM_LAUNCH_CHECK();
    if (!ba.op_add && n_qr > 0) {
        const int key = D * 2 + (idx_bits == 64 ? 1 : 0);
        switch (key) {
            case 16 * 2 + 0: launch_mult<16, int>(ba, (long long)B, F, gout, (long long)gout_ld, st); break;
            case 16 * 2 + 1: launch_mult<16, long long>(ba, (long long)B, F, gout, (long long)gout_ld, st); break;
            case 32 * 2 + 0: launch_mult<32, int>(ba, (long long)B, F, gout, (long long)gout_ld, st); break;
            case 32 * 2 + 1: launch_mult<32, long long>(ba, (long long)B, F, gout, (long long)gout_ld, st); break;
            case 64 * 2 + 0: launch_mult<64, int>(ba, (long long)B, F, gout, (long long)gout_ld, st); break;
            case 64 * 2 + 1: launch_mult<64, long long>(ba, (long long)B, F, gout, (long long)gout_ld, st); break;
            default: return DLRM_E_MODE;
        }
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}
