// gather_common.h — what the fused lookup + interaction kernels of interact_bf16.hip, interact_quant.hip, interact_qr.hip and
// the interact_narrow*.hip files share: the selector hand-off, the kernarg tables' way into LDS, the dR row staging, the grid rule and the host-side
// argument checks.  The D = 128 pipeline built on these is gather_pipeline.h; the narrow kernels use this header alone.
#pragma once
#include "interact_tiles.h"      // the typedefs, pair_pos and the forward MFMA section

namespace {

constexpr int GC_MAXF = 32;                 // feature slots of an argument block
constexpr int GC_WAVES = 4;                 // waves of a workgroup: one per SIMD
constexpr unsigned GC_BAD = 0xFFFFFFFFu;    // row selector of an out-of-range id (tables have at most 0xFFFFFFFF rows: never a valid row)

// fma(1, v, +0): the lookup kernels' sum of a bag of one row without per-sample weights (-0.0 becomes +0.0)
__device__ __forceinline__ float bag1(float v) { return __builtin_fmaf(1.0f, v, 0.f); }
__device__ __forceinline__ float4 bag1(const floatx4& v) { return make_float4(bag1(v.x), bag1(v.y), bag1(v.z), bag1(v.w)); }

// the argument block of one-array tables (bf16, quantised, narrow fp32): feature f >= 1 is table f - 1; slot 0 is unused (feature 0 = x)
struct GatherArgs {
    const void* w[GC_MAXF];                 // table rows
    const void* idx[GC_MAXF];
    const void* off[GC_MAXF];               // bag starts: verified to be 0, 1, 2, ... (one lookup per bag)
    long long   rows[GC_MAXF];
    long long*  err;
    DlrmPred    pred;
};

// the kernarg tables into LDS with compile-time kernarg offsets (a lane-indexed read of a by-value struct would go to scratch)
__device__ __forceinline__ void args_to_lds(const GatherArgs& a, long long* tw, long long* tq, long long* to, long long* tr, int F) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int f = 1; f < GC_MAXF; ++f)
        if (tid == f && f < F) { tw[f] = (long long)a.w[f]; tq[f] = (long long)a.idx[f]; to[f] = (long long)a.off[f]; tr[f] = a.rows[f]; }
}

// Lane f (1 <= f < F) owns feature f's selector.  L is the per-lane state of the kernel: own, qsrc, osrc (idx / off of feature `lane`), rows.
template <typename IT>
struct Sel { IT id, off; };

template <typename IT, typename L>
__device__ __forceinline__ Sel<IT> sel_load(const L& bl, long long s) {
    Sel<IT> r; r.id = 0; r.off = 0;
    if (bl.own) {
        r.id = *(const __attribute__((address_space(1))) IT*)(bl.qsrc + s * (long long)sizeof(IT));
        r.off = *(const __attribute__((address_space(1))) IT*)(bl.osrc + s * (long long)sizeof(IT));
    }
    return r;
}

// the owner lane's checks (as gather_rows_issue of interact.hip, except that a bad id selects the zero row, as the lookup kernels skip it)
template <typename IT, typename L>
__device__ __forceinline__ unsigned sel_resolve(const L& bl, const Sel<IT>& sel, long long s, int lane, long long* err) {
    unsigned idu = GC_BAD;
    if (bl.own) {
        const long long id = (long long)sel.id, o = (long long)sel.off;
        if (o != s) dlrm_report_bad_index(err, lane - 1, -(o + 1), -1);                 // not a one-lookup-per-bag batch (rows = -1 marks it)
        if (!dlrm_index_ok(id, bl.rows)) dlrm_report_bad_index(err, lane - 1, id, bl.rows);
        else idu = (unsigned)id;
    }
    return idu;
}

// the lane's share of a dR row: bytes [1024 c + 16 lane, +16), c < NC, where they lie inside the first rowb bytes of the row
template <int NC> struct DrRegs { float4 v[NC]; };
template <int NC, typename RB>
__device__ __forceinline__ DrRegs<NC> dr_load(const float* __restrict__ row, RB rowb, int lane) {
    DrRegs<NC> d;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        d.v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((RB)(1024 * c + 16 * lane) < rowb) d.v[c] = *(const float4*)((const char*)row + 1024 * c + 16 * lane);
    }
    return d;
}
template <int NC, typename RB>
__device__ __forceinline__ void dr_write(char* img, const DrRegs<NC>& d, RB rowb, int lane) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if ((RB)(1024 * c + 16 * lane) < rowb) *(float4*)(img + 1024 * c + 16 * lane) = d.v[c];
}

// workgroups of one pass: 256 CUs x min(2, workgroups whose LDS fits the 160 KiB of a CU); a wave takes one sample per pass
static inline long long gather_grid(long long B, size_t lds) {
    const long long per_cu = (160 * 1024) / (long long)lds >= 2 ? 2 : 1;
    long long nb = (B + GC_WAVES - 1) / GC_WAVES;
    if (nb > 256 * per_cu) nb = 256 * per_cu;
    return nb;
}

// the argument block of an entry point; 0 or a DLRM_E_* code.  w_align: mask of the address bits a table must have clear (one lane's load)
static inline int fill_args(GatherArgs& a, int F, const void* const* weight_host, const int64_t* rows_host, const void* const* index_host,
                            const void* const* offsets_host, int64_t* err, const int32_t* pred_flag, int pred_nonzero, uintptr_t w_align) {
    a.err = (long long*)err;
    a.pred = DlrmPred{(const int*)pred_flag, pred_nonzero};
    for (int f = 0; f < GC_MAXF; ++f) {
        const int t = (f >= 1 && f < F) ? f - 1 : (F > 1 ? 0 : -1);      // unused slots repeat table 0 (never dereferenced)
        a.w[f] = t >= 0 ? weight_host[t] : nullptr;
        a.idx[f] = t >= 0 ? index_host[t] : nullptr;
        a.off[f] = t >= 0 ? offsets_host[t] : nullptr;
        a.rows[f] = t >= 0 ? rows_host[t] : 0;
        if (f >= 1 && f < F) {
            if (!a.w[f] || !a.idx[f] || !a.off[f] || a.rows[f] <= 0) return DLRM_E_ARG;
            if (a.rows[f] > 0xFFFFFFFFLL) return DLRM_E_RANGE;             // row selectors travel as 32-bit values inside the kernels
            if (((uintptr_t)a.w[f]) & w_align) return DLRM_E_MODE;
        }
    }
    return 0;
}

// The checks at the head of a forward entry point, in the order the codes are documented in: 0 or a DLRM_E_* code.  tables: every host
// array of the table list is there; kind_ok: the kind's dlrm_interact_gather_*_ok(F, D); fill(): the kind's fill_args, run between the
// shape checks and the alignment checks.
template <typename Fill>
static inline int gather_check_fwd(int64_t B, int F, int D, const float* x, int64_t x_ld, bool tables, int idx_bits, bool kind_ok,
                                   int self_interaction, const float* R, int64_t ldr, Fill&& fill) {
    if (B <= 0 || F <= 0 || D <= 0 || !x || !R) return DLRM_E_ARG;
    if (F > 1 && !tables) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    if (!kind_ok) return DLRM_E_MODE;
    if (self_interaction < 0 || self_interaction > 2) return DLRM_E_MODE;     // 0 tril, 1 tril + diagonal, 2 torchrec triu order
    const int P = (self_interaction & 1) ? F * (F + 1) / 2 : F * (F - 1) / 2;
    if (ldr < D + P || x_ld < D) return DLRM_E_ARG;
    const int rc = fill();
    if (rc) return rc;
    if (!dlrm_aligned16(x) || x_ld % 4 != 0 || !dlrm_aligned16(R) || ldr % 4 != 0) return DLRM_E_MODE;
    return 0;
}

// ... and of a backward entry point.  tables includes dE; dE_min: least dE_ld (INT64_MIN where fill() checks it, as QR's virtual table
// list is counted there); drb: bytes of the dR row image, which the row must stay below (0: the kernel sizes it from F).
template <typename Fill>
static inline int gather_check_bwd(int64_t B, int F, int D, const float* x, int64_t x_ld, bool tables, int idx_bits, bool kind_ok,
                                   int self_interaction, const float* dR, int64_t ldr, const float* dx, int64_t dx_ld, const float* dE,
                                   int64_t dE_ld, int64_t dE_min, int64_t drb, Fill&& fill) {
    if (B <= 0 || F <= 0 || D <= 0 || !x || !dR || !dx) return DLRM_E_ARG;
    if (F > 1 && !tables) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    if (!kind_ok) return DLRM_E_MODE;
    // bits 0-1 as the forward; bit 2 (DLRM_INTERACT_RELU_X): x is the output of a ReLU and dx is multiplied by [x > 0]
    if (self_interaction < 0 || self_interaction > 7 || (self_interaction & 3) > 2) return DLRM_E_MODE;
    const int P = (self_interaction & 1) ? F * (F + 1) / 2 : F * (F - 1) / 2;
    if (ldr < D + P || x_ld < D || dx_ld < D || (F > 1 && dE_ld < dE_min)) return DLRM_E_ARG;
    const int rc = fill();
    if (rc) return rc;
    if (!dlrm_aligned16(x) || x_ld % 4 != 0 || !dlrm_aligned16(dR) || ldr % 4 != 0 || !dlrm_aligned16(dx) || dx_ld % 4 != 0) return DLRM_E_MODE;
    if (F > 1 && (!dlrm_aligned16(dE) || dE_ld % 4 != 0)) return DLRM_E_MODE;
    if (drb && ldr * 4 >= drb) return DLRM_E_MODE;             // (strictly: the dR image's last word stays zero)
    return 0;
}

}  // namespace
