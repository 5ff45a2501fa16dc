// interact_quant.hip — fused lookup + pairwise-dot interaction, forward only, over row-wise QUANTISED embedding tables, gfx950.
//
// Reference call sites replaced: the quantised branch of DLRM_Net.apply_emb (ops.quantized.embedding_bag_{byte,4bit}_rowwise_offsets,
//   dlrm_s_pytorch.py:430-450) followed by DLRM_Net.interact_features, arch_interaction_op == "dot" (dlrm_s_pytorch.py:483-504), for batches
//   with ONE lookup per bag.  The [B, T*D] fp32 pooled buffer that dlrm_emb_fwd_quant writes and dlrm_interact_fwd reads back never exists.
//
// Contract: R is BIT-IDENTICAL to dlrm_emb_fwd_quant (no per-sample weights, one lookup per bag) + dlrm_interact_fwd:
//   * element  = fmaf(1.0f, fmaf(scale, (float)q, bias), +0.0f)      — the lookup's arithmetic from a zero accumulator (emb_quant.hip); the
//                fp16 scale / bias of the 4-bit form convert exactly; an out-of-range id gives a row of +0.0 and is reported;
//   * dot      = the summation order of every version of the interaction kernel (interact.hip): v_mfma_f32_16x16x4_f32, k-step s outermost,
//                element e of the lane's quad = column 16 s + 4 (lane >> 4) + e, even e into one accumulator and odd e into a second one,
//                the two added at the end, lower-triangle tile pairs only.
//   Both follow from gather_pipeline.h's forward kernel, which dequantises the rows into the wave-private swizzled fp32 LDS image of
//   interact_fwd_dma_kernel and runs its fragment-read / MFMA / store section on it unchanged.
//
// Row fetch.  Packed rows cannot ride the LDS-DMA into an fp32 image; they go through registers.  A lane owns 8 consecutive columns of a
//   row: one 8-byte (8 bits) or 4-byte (4 bits) load of codes plus the row's scale / bias word; 16 lanes cover a row, a wave 4 rows per
//   pass, ceil((F - 1) / 4) <= 7 passes per sample.  Lane f (1 <= f < F) owns feature f's selector: it loads idx[f][s] and off[f][s], checks
//   them and hands the row number to the 16 lanes of that row by ds_bpermute.  Feature 0 (x) is one float4 load in lanes 0..31.
//
// Launch shape: four waves per workgroup, one per SIMD, as the fp32 kernel.  What was weighed:
//   * LDS: two 16 NB-row images per wave = 32 KiB (F > 16) -> 4 waves = 128 KiB + tables: one workgroup per CU; a fifth wave would fit but
//     shares a SIMD with another (the fp32 kernel measured 245 vs 211 us with five).  F <= 16: 16 KiB per wave, two workgroups per CU.
//     The staging registers already are a second buffer, so a single image per wave (8 waves in 115 KiB) would be legal; it is not what
//     is built here — the double-buffered form was asked for and is the one measured (profiles/quant_emb/fused_interact_rates.md).
//   * the exposed VALU dequantise: ~3 (8 bits) / 4 (4 bits) VALU per element, 8 elements per lane and pass: ~170-220 VALU per sample
//     beside 96 MFMAs.  With one wave per SIMD nothing else covers it except the MFMA pipe's own latency (the dequantise is independent
//     of the MFMAs in flight and is placed behind them in program order); the sample time is bounded below by the gather latency of one
//     sample per wave either way, which is what the measurement shows (0.239 / 0.247 ms at 8 / 4 bits against 0.513 / 0.498 ms for the two kernels and 0.214 ms for the fp32
//     fused forward, Criteo-Terabyte shapes).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, 64-bit ids / 32-bit ids where they differ; no static
//   LDS, the dynamic LDS of a workgroup is what gather_lds<QuantSource<BITS>>() returns):
//                                                  VGPRs    AGPRs  SGPRs  scratch  dynamic LDS
//   gather_fwd_kernel<QuantSource<8>, 1, IT>     120 / 118     8     90      0      66560 B   (F <= 16: two workgroups per CU)
//   gather_fwd_kernel<QuantSource<8>, 2, IT>     196          24     90      0     132096 B   (one workgroup per CU)
//   gather_fwd_kernel<QuantSource<4>, 1, IT>     114           8     90      0      66560 B
//   gather_fwd_kernel<QuantSource<4>, 2, IT>     186          24     90      0     132096 B
#include "gather_pipeline.h"

namespace {

typedef unsigned uintx2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float f16_bits_to_f32(unsigned h) {
    union { unsigned short u; _Float16 f; } c; c.u = (unsigned short)h; return (float)c.f;
}

// a lane's 8 columns of one packed row, as emb_quant.hip loads them
template <int BITS> struct QRow;
template <> struct QRow<8> { uint2 q; float2 sb; };
template <> struct QRow<4> { unsigned q; unsigned sb; };
__device__ __forceinline__ void q_zero(QRow<8>& v) { v.q = make_uint2(0u, 0u); v.sb = make_float2(0.f, 0.f); }
__device__ __forceinline__ void q_zero(QRow<4>& v) { v.q = 0u; v.sb = 0u; }
// row: start of the packed row; li: the lane's position inside the row (columns 8 li .. 8 li + 7)
__device__ __forceinline__ void q_load(QRow<8>& v, const gchar* row, int li) {
    const uintx2 q = *(const __attribute__((address_space(1))) uintx2*)(row + 8 * li);
    const floatx2 sb = *(const __attribute__((address_space(1))) floatx2*)(row + BI_D);
    v.q = make_uint2(q.x, q.y); v.sb = make_float2(sb.x, sb.y);
}
__device__ __forceinline__ void q_load(QRow<4>& v, const gchar* row, int li) {
    v.q = *(const __attribute__((address_space(1))) unsigned*)(row + 4 * li);
    v.sb = *(const __attribute__((address_space(1))) unsigned*)(row + BI_D / 2);
}
// out[j] = fma(1, fma(scale, q[j], bias), +0): dlrm_emb_fwd_quant's element for a bag of one row without per-sample weights
__device__ __forceinline__ void q_dequant(float (&o)[8], const QRow<8>& v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = bag1(__builtin_fmaf(v.sb.x, (float)((v.q.x >> (8 * j)) & 0xFFu), v.sb.y));
        o[4 + j] = bag1(__builtin_fmaf(v.sb.x, (float)((v.q.y >> (8 * j)) & 0xFFu), v.sb.y));
    }
}
__device__ __forceinline__ void q_dequant(float (&o)[8], const QRow<4>& v) {
    const float scale = f16_bits_to_f32(v.sb & 0xFFFFu), bias = f16_bits_to_f32(v.sb >> 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = bag1(__builtin_fmaf(scale, (float)((v.q >> (4 * j)) & 0xFu), bias));
}

template <int BITS>
struct QuantSource {          // forward only: no dst_slot / DUP
    using Args = GatherArgs;
    using Row = unsigned;
    static constexpr int NTAB = 4;          // w, idx, off, rows
    static constexpr int passes(int nb) { return nb == 1 ? 4 : 7; }      // rows 1 .. 16 NB - 1 (F <= 27), four per pass

    template <int NP>
    struct Lane {
        const gchar* base[NP];      // packed rows of the table behind image row 1 + 4 p + (lane >> 4)
        unsigned wofs[NP][2];       // byte offsets of the lane's two 16-byte slots inside the image
        bool on[NP];                // that row is a feature (< F)
        const gchar* qsrc;          // lanes 1 .. F - 1: idx / off of feature `lane`
        const gchar* osrc;
        long long rows;
        bool own;
    };
    template <int NP> struct Regs { QRow<BITS> v[NP]; };

    static __device__ __forceinline__ void args_to_lds(const Args& a, long long* tab, int F) {
        ::args_to_lds(a, tab, tab + GC_MAXF, tab + 2 * GC_MAXF, tab + 3 * GC_MAXF, F);
    }

    template <int NP>
    static __device__ __forceinline__ void lane_init(Lane<NP>& ql, const long long* tab, int F, int lane) {
        const int g = lane >> 4, li = lane & 15;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int row = 1 + 4 * p + g;
            ql.on[p] = row < F;                                   // no lane loads a row for a feature slot >= F
            ql.base[p] = ql.on[p] ? (const gchar*)tab[row] : nullptr;
            ql.wofs[p][0] = row * BI_ROWB + (((2 * li) ^ (row & 15)) * 16);
            ql.wofs[p][1] = row * BI_ROWB + (((2 * li + 1) ^ (row & 15)) * 16);
        }
        ql.own = lane >= 1 && lane < F;
        ql.qsrc = ql.own ? (const gchar*)tab[GC_MAXF + lane] : nullptr;
        ql.osrc = ql.own ? (const gchar*)tab[2 * GC_MAXF + lane] : nullptr;
        ql.rows = ql.own ? tab[3 * GC_MAXF + lane] : 0;
    }

    template <typename IT, int NP>
    static __device__ __forceinline__ Row sel_resolve(const Lane<NP>& ql, const Sel<IT>& sel, long long s, int lane, long long* err, bool live) {
        return live ? ::sel_resolve(ql, sel, s, lane, err) : GC_BAD;
    }

    // row loads of one sample into registers: NP passes, two loads each, nothing waits here
    template <int NP>
    static __device__ __forceinline__ void rows_issue(Regs<NP>& v, const Lane<NP>& ql, unsigned idu, int lane) {
        constexpr unsigned long long RB = BITS == 8 ? BI_D + 8 : BI_D / 2 + 4;
        const int g = lane >> 4, li = lane & 15;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const unsigned mine = (unsigned)__shfl((int)idu, 1 + 4 * p + g, 64);      // (1 + 4 p + g <= 28: always a lane of this wave)
            q_zero(v.v[p]);
            if (ql.on[p] && mine != GC_BAD) q_load(v.v[p], ql.base[p] + (unsigned long long)mine * RB, li);      // 64-bit byte offset
        }
    }

    template <int NP>
    static __device__ __forceinline__ void image_write(char* img, const Regs<NP>& v, const Lane<NP>& ql, const float4& xv, int lane, const Args&) {
        if (lane < 32) *(float4*)(img + 16 * lane) = xv;                    // row 0: (row & 15) == 0, slot = quad
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (ql.on[p]) {
                float o[8];
                q_dequant(o, v.v[p]);
                *(float4*)(img + ql.wofs[p][0]) = make_float4(o[0], o[1], o[2], o[3]);
                *(float4*)(img + ql.wofs[p][1]) = make_float4(o[4], o[5], o[6], o[7]);
            }
        }
    }
};

}  // namespace

extern "C" int dlrm_interact_gather_quant_ok(int F, int D, int bits) {
    return (D == BI_D && (bits == 4 || bits == 8) && F < GC_MAXF && dlrm_interact_gather_ok(F, D)) ? 1 : 0;
}

extern "C" int dlrm_interact_fwd_gather_quant(int64_t B, int F, int D, int bits, const float* x, int64_t x_ld,
                                              const void* const* qweight_host, const int64_t* rows_host,
                                              const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                              int self_interaction, float* R, int64_t ldr, int64_t* err,
                                              const int32_t* pred_flag, int pred_nonzero, void* stream) {
    GatherArgs qa;
    const int rc = gather_check_fwd(B, F, D, x, x_ld, qweight_host && rows_host && index_host && offsets_host, idx_bits,
                                    dlrm_interact_gather_quant_ok(F, D, bits), self_interaction, R, ldr, [&] {
        // a lane's codes are one 8-byte / 4-byte load; rows are 136 / 68 bytes apart
        return fill_args(qa, F, qweight_host, rows_host, index_host, offsets_host, err, pred_flag, pred_nonzero, bits == 8 ? 7u : 3u);
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 3;
    if (bits == 8) gather_fwd<QuantSource<8>>(qa, x, x_ld, B, F, self, R, ldr, idx_bits, st);
    else           gather_fwd<QuantSource<4>>(qa, x, x_ld, B, F, self, R, ldr, idx_bits, st);
    DLRM_LAUNCH_CHECK();
    return 0;
}
