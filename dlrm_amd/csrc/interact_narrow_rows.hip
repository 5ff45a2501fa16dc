// interact_narrow_rows.hip — the fused lookup + pairwise-dot interaction kernels of interact_narrow.h over bfloat16 tables (forward AND
// backward) and over 8- / 4-bit row-wise quantised tables (forward only), D = 16 / 32 / 64, gfx950.
//
// Replaces, for batches with ONE lookup per bag and no per-sample weights: dlrm_emb_fwd_bf16 / dlrm_emb_fwd_quant + dlrm_interact_fwd
//   (forward) and dlrm_interact_bwd over the pooled [B, T*D] buffer (backward, bf16) at the widths where those are the GENERIC interaction
//   kernels.  The pooled fp32 buffer is neither written nor read.  The D = 128 forms are interact_bf16.hip and interact_quant.hip.
//
// Contract (include/dlrm_hip.h): R, dx, dE are BIT-IDENTICAL to the two-kernel form.  Geometry, pipeline, MFMA order and stores are those of
//   interact_narrow.hip (the kernels are the same templates); a row source changes what a lane loads of a row and the widen / dequantise
//   step in front of image_write:
//   * bf16 : a row is 2 D bytes; a lane's 4 columns are ONE 8-byte load at row * 2D + 8 lc;
//            element = fmaf(1.0f, upcast(bits), +0.0f) — emb_bf16.hip's lookup from a zero accumulator, so -0.0 becomes +0.0;
//   * 8 bit: a row is D + 8 bytes (dlrm_emb_quantize_rows: D codes, fp32 scale, fp32 bias); a lane's 4 codes are ONE 4-byte load at
//            row * (D + 8) + 4 lc, plus the row's 8-byte (scale, bias) at byte D;
//            element = fmaf(1.0f, fmaf(scale, (float)q, bias), +0.0f) — interact_quant.hip's q_dequant;
//   * 4 bit: a row is D/2 + 4 bytes (D/2 bytes of codes, low nibble first, fp16 scale | fp16 bias); a lane's 4 codes are ONE 2-byte load at
//            row * (D/2 + 4) + 2 lc, plus the row's 4-byte (scale | bias) at byte D/2, converted exactly; element as at 8 bits.
//   Row byte offsets are 64-bit.  An out-of-range id or a broken bag start is reported and gives a row of +0.0 (staged zeros: code 0, scale 0,
//   bias 0); the backward writes such a feature's gradient row like any other.  The table bases must be 8- (bf16, 8 bit) / 4-byte (4 bit)
//   aligned: every load of a lane is then naturally aligned (row pitches 2 D, D + 8 and D/2 + 4 are multiples of 8, 8 and 4).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no static LDS; the dynamic LDS of a workgroup is what
//   narrow_lds() returns: it depends on D and NB only, so it is the fp32 kernels').  Scratch is 0 everywhere.
//                                                       VGPRs (int / long long ids)  AGPRs  SGPRs  scratch  dynamic LDS
//   interact_fwd_narrow_kernel<Bf16Rows, 16, 1, IT>       56 /  56                  8     90      0      11264 B
//   interact_fwd_narrow_kernel<Bf16Rows, 16, 2, IT>       86 /  86                 24     90      0      21504 B
//   interact_fwd_narrow_kernel<Bf16Rows, 32, 1, IT>       62 /  64                  8     90      0      19456 B
//   interact_fwd_narrow_kernel<Bf16Rows, 32, 2, IT>       98 /  98                 24     90      0      37888 B
//   interact_fwd_narrow_kernel<Bf16Rows, 64, 1, IT>       82 /  82                  8     90      0      35840 B
//   interact_fwd_narrow_kernel<Bf16Rows, 64, 2, IT>      134 / 134                 24     90      0      70656 B
//   interact_bwd_narrow_kernel<Bf16Rows, 16, 1, IT>       76 /  77                  8     90      0      19456 B
//   interact_bwd_narrow_kernel<Bf16Rows, 16, 2, IT>      140 / 141                  8     90      0      46080 B
//   interact_bwd_narrow_kernel<Bf16Rows, 32, 1, IT>       94 /  94                 16     90      0      27648 B
//   interact_bwd_narrow_kernel<Bf16Rows, 32, 2, IT>      160 / 162                 16     92      0      62464 B
//   interact_bwd_narrow_kernel<Bf16Rows, 64, 1, IT>      118 / 118                 32     90      0      44032 B
//   interact_bwd_narrow_kernel<Bf16Rows, 64, 2, IT>      216 / 218                 32     92      0      95232 B   (one workgroup per CU)
//   interact_fwd_narrow_kernel<QuantRows<8>, 16, 1, IT>   56 /  56                  8     90      0      11264 B
//   interact_fwd_narrow_kernel<QuantRows<8>, 16, 2, IT>   86 /  86                 24     90      0      21504 B
//   interact_fwd_narrow_kernel<QuantRows<8>, 32, 1, IT>   64 /  66                  8     90      0      19456 B
//   interact_fwd_narrow_kernel<QuantRows<8>, 32, 2, IT>  100 / 100                 24     90      0      37888 B
//   interact_fwd_narrow_kernel<QuantRows<8>, 64, 1, IT>   84 /  84                  8     90      0      35840 B
//   interact_fwd_narrow_kernel<QuantRows<8>, 64, 2, IT>  140 / 140                 24     90      0      70656 B
//   interact_fwd_narrow_kernel<QuantRows<4>, 16, 1, IT>   54 /  54                  8     90      0      11264 B
//   interact_fwd_narrow_kernel<QuantRows<4>, 16, 2, IT>   86 /  86                 24     90      0      21504 B
//   interact_fwd_narrow_kernel<QuantRows<4>, 32, 1, IT>   62 /  64                  8     90      0      19456 B
//   interact_fwd_narrow_kernel<QuantRows<4>, 32, 2, IT>   98 /  98                 24     90      0      37888 B
//   interact_fwd_narrow_kernel<QuantRows<4>, 64, 1, IT>   80 /  82                  8     90      0      35840 B
//   interact_fwd_narrow_kernel<QuantRows<4>, 64, 2, IT>  132 / 134                 24     90      0      70656 B
#include "interact_narrow.h"

namespace {

typedef unsigned uintx2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
__device__ __forceinline__ float f16_bits_to_f32(unsigned h) {
    union { unsigned short u; _Float16 f; } c; c.u = (unsigned short)h; return (float)c.f;
}

// bfloat16 rows: 4 columns = one 8-byte load
struct Bf16Rows : OneArraySide {
    static constexpr int LB = 8;
    static constexpr unsigned long long pitch(int D) { return 2ull * D; }
    using Regs = uint2;
    static __device__ __forceinline__ void zero(Regs& v) { v = make_uint2(0u, 0u); }
    template <int D>
    static __device__ __forceinline__ void load(Regs& v, const gchar* slot, int) {
        const uintx2 q = *(const __attribute__((address_space(1))) uintx2*)slot;
        v = make_uint2(q.x, q.y);
    }
    static __device__ __forceinline__ float4 widen(const Regs& q) {
        return make_float4(bag1(bf_lo(q.x)), bag1(bf_hi(q.x)), bag1(bf_lo(q.y)), bag1(bf_hi(q.y)));
    }
};

// packed rows of dlrm_emb_quantize_rows
template <int BITS> struct QuantRows;
template <> struct QuantRows<8> : OneArraySide {
    static constexpr int LB = 4;
    static constexpr unsigned long long pitch(int D) { return (unsigned long long)D + 8; }
    struct Regs { unsigned q; float2 sb; };
    static __device__ __forceinline__ void zero(Regs& v) { v.q = 0u; v.sb = make_float2(0.f, 0.f); }
    template <int D>
    static __device__ __forceinline__ void load(Regs& v, const gchar* slot, int lc) {
        v.q = *(const __attribute__((address_space(1))) unsigned*)slot;
        const floatx2 sb = *(const gfloatx2*)(slot + (D - LB * lc));                // the row's (scale, bias) at byte D
        v.sb = make_float2(sb.x, sb.y);
    }
    static __device__ __forceinline__ float4 widen(const Regs& v) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = bag1(__builtin_fmaf(v.sb.x, (float)((v.q >> (8 * j)) & 0xFFu), v.sb.y));
        return make_float4(o[0], o[1], o[2], o[3]);
    }
};
template <> struct QuantRows<4> : OneArraySide {
    static constexpr int LB = 2;
    static constexpr unsigned long long pitch(int D) { return (unsigned long long)D / 2 + 4; }
    struct Regs { unsigned q; unsigned sb; };
    static __device__ __forceinline__ void zero(Regs& v) { v.q = 0u; v.sb = 0u; }
    template <int D>
    static __device__ __forceinline__ void load(Regs& v, const gchar* slot, int lc) {
        v.q = *(const __attribute__((address_space(1))) unsigned short*)slot;
        v.sb = *(const __attribute__((address_space(1))) unsigned*)(slot + (D / 2 - LB * lc));      // the row's fp16 scale | bias at byte D/2
    }
    static __device__ __forceinline__ float4 widen(const Regs& v) {
        const float scale = f16_bits_to_f32(v.sb & 0xFFFFu), bias = f16_bits_to_f32(v.sb >> 16);
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = bag1(__builtin_fmaf(scale, (float)((v.q >> (4 * j)) & 0xFu), bias));      // low nibble first
        return make_float4(o[0], o[1], o[2], o[3]);
    }
};

}  // namespace

extern "C" int dlrm_interact_gather_narrow_bf16_ok(int F, int D) {
    return dlrm_interact_gather_narrow_ok(F, D);
}

extern "C" int dlrm_interact_gather_narrow_quant_ok(int F, int D, int bits) {
    return ((bits == 4 || bits == 8) && dlrm_interact_gather_narrow_ok(F, D)) ? 1 : 0;
}

extern "C" int dlrm_interact_fwd_gather_narrow_bf16(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                                    const void* const* weight_host, const int64_t* rows_host,
                                                    const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                                    int self_interaction, float* R, int64_t ldr, int64_t* err,
                                                    const int32_t* pred_flag, int pred_nonzero, void* stream) {
    GatherArgs na;
    // a lane's 4 columns are one 8-byte load; rows are 2 D bytes apart
    const int rc = gather_check_fwd(B, F, D, x, x_ld, weight_host && rows_host && index_host && offsets_host, idx_bits,
                                    dlrm_interact_gather_narrow_bf16_ok(F, D), self_interaction, R, ldr, [&] {
        return fill_args(na, F, weight_host, rows_host, index_host, offsets_host, err, pred_flag, pred_nonzero, 7u);
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 3;
    NARROW_DISPATCH(launch_fwd, Bf16Rows, na, x, (long long)x_ld, (long long)B, F, self, R, (long long)ldr, st);
    DLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int dlrm_interact_bwd_gather_narrow_bf16(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                                    const void* const* weight_host, const int64_t* rows_host,
                                                    const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                                    int self_interaction, const float* dR, int64_t ldr,
                                                    float* dx, int64_t dx_ld, float* dE, int64_t dE_ld, int64_t* err,
                                                    const int32_t* pred_flag, int pred_nonzero, void* stream) {
    GatherArgs na;
    const int rc = gather_check_bwd(B, F, D, x, x_ld, weight_host && rows_host && index_host && offsets_host && dE, idx_bits,
                                    dlrm_interact_gather_narrow_bf16_ok(F, D), self_interaction, dR, ldr, dx, dx_ld, dE, dE_ld,
                                    (int64_t)(F - 1) * D, 0, [&] {
        return fill_args(na, F, weight_host, rows_host, index_host, offsets_host, err, pred_flag, pred_nonzero, 7u);
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 7;
    NARROW_DISPATCH(launch_bwd, Bf16Rows, na, x, (long long)x_ld, (long long)B, F, self, dR, (long long)ldr, dx, (long long)dx_ld, dE,
                    (long long)dE_ld, st);
    DLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int dlrm_interact_fwd_gather_narrow_quant(int64_t B, int F, int D, int bits, const float* x, int64_t x_ld,
                                                     const void* const* qweight_host, const int64_t* rows_host,
                                                     const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                                     int self_interaction, float* R, int64_t ldr, int64_t* err,
                                                     const int32_t* pred_flag, int pred_nonzero, void* stream) {
    GatherArgs na;
    const int rc = gather_check_fwd(B, F, D, x, x_ld, qweight_host && rows_host && index_host && offsets_host, idx_bits,
                                    dlrm_interact_gather_narrow_quant_ok(F, D, bits), self_interaction, R, ldr, [&] {
        // the widest load of a lane is the 8-byte (scale, bias) pair (8 bits) / the 4-byte scale | bias word (4 bits); rows are D + 8 /
        // D/2 + 4 bytes apart
        return fill_args(na, F, qweight_host, rows_host, index_host, offsets_host, err, pred_flag, pred_nonzero, bits == 8 ? 7u : 3u);
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 3;
    if (bits == 8) NARROW_DISPATCH(launch_fwd, QuantRows<8>, na, x, (long long)x_ld, (long long)B, F, self, R, (long long)ldr, st);
    else           NARROW_DISPATCH(launch_fwd, QuantRows<4>, na, x, (long long)x_ld, (long long)B, F, self, R, (long long)ldr, st);
    DLRM_LAUNCH_CHECK();
    return 0;
}
