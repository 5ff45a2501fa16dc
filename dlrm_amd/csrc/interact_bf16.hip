// interact_bf16.hip — fused lookup + pairwise-dot interaction, forward AND backward, over bfloat16 embedding tables, gfx950.
//
// Replaces, for batches with ONE lookup per bag and no per-sample weights: dlrm_emb_fwd_bf16 + dlrm_interact_fwd (forward) and
//   dlrm_interact_bwd over the pooled [B, T*D] fp32 buffer (backward).  That buffer is neither written nor read, and nothing has to live
//   from forward to backward except x: the backward fetches the bf16 rows again.
//
// Contract (include/dlrm_hip.h):
//   forward : R is BIT-IDENTICAL to dlrm_emb_fwd_bf16 (psw_host = NULL) into a feature buffer + dlrm_interact_fwd, modes 0 / 1 / 2;
//   backward: dx, dE are BIT-IDENTICAL to dlrm_interact_bwd over (x, that buffer); dE[b, t*D : (t+1)*D] is the gradient row of table t.
//   * element = fmaf(1.0f, upcast(bits), +0.0f) — the lookup's arithmetic from a zero accumulator (emb_bf16.hip), so -0.0 becomes +0.0;
//     an out-of-range id gives a row of +0.0 and is reported (NOT row 0, which the fp32 fused kernels read); its gradient row is written
//     like any other;
//   * products = the summation order of the D = 128 interaction kernels (interact.hip): the kernels are gather_pipeline.h's, which widen
//     the rows into the LDS image of interact_{fwd,bwd}_dma_kernel and run those kernels' multiply sections on it.
//
// Row fetch: a bf16 row of D = 128 is 256 bytes; a lane owns 8 columns = ONE 16-byte load, 16 lanes cover a row, a wave fetches 4 rows per
//   pass, ceil((F - 1) / 4) <= 7 passes per sample.  Lane f (1 <= f < F) owns feature f's selector: it loads idx[f][s] and off[f][s], checks
//   them and hands the row number to the 16 lanes of that row by lane shuffle.  Widening is a 16-bit shift / mask: 2 VALU per pair of
//   elements plus the fma.  Feature 0 (x) is one float4 load in lanes 0..31; the backward's dR row is at most two 16-byte loads per lane.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, the same for 32- and 64-bit ids; no static LDS, the
//   dynamic LDS of a workgroup is what gather_lds<Bf16Source>() returns):
//                                              VGPRs  AGPRs  SGPRs  scratch  dynamic LDS
//   gather_fwd_kernel<Bf16Source, 1, IT>         118      8     90      0      66560 B   (F <= 16: two workgroups per CU)
//   gather_fwd_kernel<Bf16Source, 2, IT>         196     24     90      0     132096 B   (one workgroup per CU)
//   gather_bwd_kernel<Bf16Source, 1, IT>         128     20     90      0      82944 B   (F <= 16: one workgroup per CU)
//   gather_bwd_kernel<Bf16Source, 2, IT>         240     28     92      0     148480 B   (one workgroup per CU)
//   One wave per SIMD may use 512 registers, so none of these limits the launch; LDS does.
#include "gather_pipeline.h"

namespace {

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

constexpr int BI_SRCB = BI_D * 2;           // bytes of a table row

// bf16 -> fp32 is exact: the 16 bits are the high half of the fp32 pattern
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }

struct Bf16Source {
    using Args = GatherArgs;
    using Row = unsigned;
    static constexpr int NTAB = 4;          // w, idx, off, rows
    static constexpr bool DUP = false;
    static constexpr int passes(int nb) { return nb == 1 ? 4 : 7; }      // rows 1 .. 16 NB - 1 (F <= 27), four per pass

    template <int NP>
    struct Lane {
        const gchar* base[NP];      // the lane's 16 bytes of row 0 of the table behind image row 1 + 4 p + (lane >> 4)
        unsigned wofs[NP][2];       // byte offsets of the lane's two 16-byte slots inside the image
        bool on[NP];                // that row is a feature (< F)
        const gchar* qsrc;          // lanes 1 .. F - 1: idx / off of feature `lane`
        const gchar* osrc;
        long long rows;
        bool own;
    };
    template <int NP> struct Regs { uint4 v[NP]; };

    static __device__ __forceinline__ void args_to_lds(const Args& a, long long* tab, int F) {
        ::args_to_lds(a, tab, tab + GC_MAXF, tab + 2 * GC_MAXF, tab + 3 * GC_MAXF, F);
    }

    template <int NP>
    static __device__ __forceinline__ void lane_init(Lane<NP>& bl, const long long* tab, int F, int lane) {
        const int g = lane >> 4, li = lane & 15;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int row = 1 + 4 * p + g;
            bl.on[p] = row < F;                                   // no lane loads a row for a feature slot >= F
            bl.base[p] = bl.on[p] ? (const gchar*)tab[row] + 16 * li : nullptr;
            bl.wofs[p][0] = row * BI_ROWB + (((2 * li) ^ (row & 15)) * 16);
            bl.wofs[p][1] = row * BI_ROWB + (((2 * li + 1) ^ (row & 15)) * 16);
        }
        bl.own = lane >= 1 && lane < F;
        bl.qsrc = bl.own ? (const gchar*)tab[GC_MAXF + lane] : nullptr;
        bl.osrc = bl.own ? (const gchar*)tab[2 * GC_MAXF + lane] : nullptr;
        bl.rows = bl.own ? tab[3 * GC_MAXF + lane] : 0;
    }

    template <typename IT, int NP>
    static __device__ __forceinline__ Row sel_resolve(const Lane<NP>& bl, const Sel<IT>& sel, long long s, int lane, long long* err, bool live) {
        return live ? ::sel_resolve(bl, sel, s, lane, err) : GC_BAD;
    }

    // row loads of one sample into registers: NP passes, one 16-byte load each, nothing waits here
    template <int NP>
    static __device__ __forceinline__ void rows_issue(Regs<NP>& v, const Lane<NP>& bl, unsigned idu, int lane) {
        const int g = lane >> 4;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const unsigned mine = (unsigned)__shfl((int)idu, 1 + 4 * p + g, 64);      // (1 + 4 p + g <= 28: always a lane of this wave)
            v.v[p] = make_uint4(0u, 0u, 0u, 0u);
            if (bl.on[p] && mine != GC_BAD) {
                const uintx4 q = *(const __attribute__((address_space(1))) uintx4*)(bl.base[p] + (unsigned long long)mine * BI_SRCB);   // 64-bit byte offset
                v.v[p] = make_uint4(q.x, q.y, q.z, q.w);
            }
        }
    }

    template <int NP>
    static __device__ __forceinline__ void image_write(char* img, const Regs<NP>& v, const Lane<NP>& bl, const float4& xv, int lane, const Args&) {
        if (lane < 32) *(float4*)(img + 16 * lane) = xv;                    // row 0: (row & 15) == 0, slot = quad
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (bl.on[p]) {
                const uint4 q = v.v[p];
                *(float4*)(img + bl.wofs[p][0]) = make_float4(bag1(bf_lo(q.x)), bag1(bf_hi(q.x)), bag1(bf_lo(q.y)), bag1(bf_hi(q.y)));
                *(float4*)(img + bl.wofs[p][1]) = make_float4(bag1(bf_lo(q.z)), bag1(bf_hi(q.z)), bag1(bf_lo(q.w)), bag1(bf_hi(q.w)));
            }
        }
    }

    static __device__ __forceinline__ long long dst_slot(const Args&, const long long*, int i, int, bool&) { return i - 1; }
};

}  // namespace

extern "C" int dlrm_interact_gather_bf16_ok(int F, int D) {
    return (D == BI_D && F < GC_MAXF && dlrm_interact_gather_ok(F, D)) ? 1 : 0;
}

extern "C" int dlrm_interact_fwd_gather_bf16(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                             const void* const* weight_host, const int64_t* rows_host,
                                             const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                             int self_interaction, float* R, int64_t ldr, int64_t* err,
                                             const int32_t* pred_flag, int pred_nonzero, void* stream) {
    GatherArgs ba;
    // a lane's 8 columns are one 16-byte load; rows are 256 bytes apart
    const int rc = gather_check_fwd(B, F, D, x, x_ld, weight_host && rows_host && index_host && offsets_host, idx_bits,
                                    dlrm_interact_gather_bf16_ok(F, D), self_interaction, R, ldr, [&] {
        return fill_args(ba, F, weight_host, rows_host, index_host, offsets_host, err, pred_flag, pred_nonzero, 15u);
    });
    if (rc) return rc;
    gather_fwd<Bf16Source>(ba, x, x_ld, B, F, self_interaction & 3, R, ldr, idx_bits, (hipStream_t)stream);
    DLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int dlrm_interact_bwd_gather_bf16(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                             const void* const* weight_host, const int64_t* rows_host,
                                             const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                             int self_interaction, const float* dR, int64_t ldr,
                                             float* dx, int64_t dx_ld, float* dE, int64_t dE_ld, int64_t* err,
                                             const int32_t* pred_flag, int pred_nonzero, void* stream) {
    GatherArgs ba;
    const int rc = gather_check_bwd(B, F, D, x, x_ld, weight_host && rows_host && index_host && offsets_host && dE, idx_bits,
                                    dlrm_interact_gather_bf16_ok(F, D), self_interaction, dR, ldr, dx, dx_ld, dE, dE_ld,
                                    (int64_t)(F - 1) * D, BI_DRB, [&] {
        return fill_args(ba, F, weight_host, rows_host, index_host, offsets_host, err, pred_flag, pred_nonzero, 15u);
    });
    if (rc) return rc;
    gather_bwd<Bf16Source>(ba, x, x_ld, B, F, self_interaction & 7, dR, ldr, dx, dx_ld, dE, dE_ld, idx_bits, (hipStream_t)stream);
    DLRM_LAUNCH_CHECK();
    return 0;
}
