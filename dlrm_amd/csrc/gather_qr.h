// gather_qr.h — what the fused lookup + interaction kernels over quotient-remainder (QR) tables share between D = 128 (interact_qr.hip) and
// D = 16 / 32 / 64 (interact_narrow_qr.hip): the argument block, its way into LDS, the owner lane's index split and the host-side fill.
#pragma once
#include "gather_common.h"
#include "qr_split.h"

namespace {

// feature f >= 1 is table f - 1; slot 0 is unused (feature 0 = x)
struct QrArgs {
    const void* w[GC_MAXF];                 // weight_q of a QR table, the rows of a plain one
    const void* wr[GC_MAXF];                // weight_r (nullptr: plain table)
    const void* idx[GC_MAXF];
    const void* off[GC_MAXF];               // bag starts: verified to be 0, 1, 2, ... (one lookup per bag)
    long long   rows[GC_MAXF];              // n: the categories of the table
    long long   rows_q[GC_MAXF];            // ceil(n / c) (plain: n)
    int         coll[GC_MAXF];              // collisions (0: plain table)
    int         vs[GC_MAXF];                // backward: virtual slot of the table (of its q component) in gout
    long long*  err;
    DlrmPred    pred;
    int         op_add;                     // the composition: + (DLRM_QR_ADD) or *
};

// what the owner lane hands to the lanes of a row: the weight_q row (GC_BAD: the zero row) and the weight_r row
struct QrRow { unsigned q, r; };

constexpr int QR_NTAB = 7;                  // LDS tables: [0] w  [1] wr  [2] idx  [3] off  [4] rows  [5] rows_q  [6] coll | vs << 32

// the kernarg tables into LDS with compile-time kernarg offsets (a lane-indexed read of a by-value struct would go to scratch)
__device__ __forceinline__ void qr_args_to_lds(const QrArgs& ba, long long* tab, int F) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int f = 1; f < GC_MAXF; ++f)
        if (tid == f && f < F) {
            tab[0 * GC_MAXF + f] = (long long)ba.w[f];   tab[1 * GC_MAXF + f] = (long long)ba.wr[f];
            tab[2 * GC_MAXF + f] = (long long)ba.idx[f]; tab[3 * GC_MAXF + f] = (long long)ba.off[f];
            tab[4 * GC_MAXF + f] = ba.rows[f];           tab[5 * GC_MAXF + f] = ba.rows_q[f];
            tab[6 * GC_MAXF + f] = (long long)(((unsigned long long)(unsigned)ba.vs[f] << 32) | (unsigned)ba.coll[f]);
        }
}

// the owner lane's checks and the index split (emb_qr.hip's: a lookup dlrm_emb_fwd_qr skips selects the zero row and is reported).
// L is the per-lane state of the kernel: own, rows, rows_q, coll.
template <typename IT, typename L>
__device__ __forceinline__ QrRow qr_sel_resolve(const L& bl, const Sel<IT>& sel, long long s, int lane, long long* err, bool live) {
    QrRow o; o.q = GC_BAD; o.r = 0u;
    if (bl.own && live) {
        const long long id = (long long)sel.id, of = (long long)sel.off;
        if (of != s) dlrm_report_bad_index(err, lane - 1, -(of + 1), -1);               // not a one-lookup-per-bag batch (rows = -1 marks it)
        long long q = id, r = 0;
        const bool ok = bl.coll ? qr_split(id, bl.rows, bl.coll, bl.rows_q, &q, &r) : dlrm_index_ok(id, bl.rows);
        if (!ok) dlrm_report_bad_index(err, lane - 1, id, bl.rows);
        else { o.q = (unsigned)q; o.r = (unsigned)r; }
    }
    return o;
}

// the argument block shared by the entry points; 0 or a DLRM_E_* code.  *n_qr: the QR tables of the call (Tv = F - 1 + *n_qr)
int fill_args(QrArgs& ba, int F, const void* const* weight_host, const void* const* weight_r_host, const int64_t* rows_host,
              const int32_t* collisions_host, const void* const* index_host, const void* const* offsets_host, int64_t* err,
              const int32_t* pred_flag, int pred_nonzero, int* n_qr) {
    ba.err = (long long*)err;
    ba.pred = DlrmPred{(const int*)pred_flag, pred_nonzero};
    int vslot = 0;
    *n_qr = 0;
    for (int f = 0; f < GC_MAXF; ++f) {
        const bool live = f >= 1 && f < F;
        const int t = live ? f - 1 : (F > 1 ? 0 : -1);                   // unused slots repeat table 0 (never dereferenced)
        const int c = t >= 0 ? collisions_host[t] : 0;
        ba.w[f] = t >= 0 ? weight_host[t] : nullptr;
        ba.wr[f] = (t >= 0 && c > 0) ? weight_r_host[t] : nullptr;
        ba.idx[f] = t >= 0 ? index_host[t] : nullptr;
        ba.off[f] = t >= 0 ? offsets_host[t] : nullptr;
        ba.rows[f] = t >= 0 ? rows_host[t] : 0;
        ba.rows_q[f] = (t >= 0 && c > 0) ? (rows_host[t] + c - 1) / c : ba.rows[f];
        ba.coll[f] = c;
        ba.vs[f] = live ? vslot : 0;
        if (live) {
            if (!ba.w[f] || !ba.idx[f] || !ba.off[f] || ba.rows[f] <= 0 || c < 0 || (c > 0 && !ba.wr[f])) return DLRM_E_ARG;
            if (ba.rows_q[f] > 0xFFFFFFFFLL) return DLRM_E_RANGE;         // row selectors travel as 32-bit values inside the kernels
            if (!dlrm_aligned16(ba.w[f]) || (c > 0 && !dlrm_aligned16(ba.wr[f]))) return DLRM_E_MODE;      // a lane's 4 columns are one 16-byte load
            vslot += c > 0 ? 2 : 1;
            *n_qr += c > 0;
        }
    }
    return 0;
}

}  // namespace
