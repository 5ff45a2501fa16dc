// emb_quant.hip — row-wise quantised embedding tables (8 and 4 bits) for gfx950: the prepack and the batched EmbeddingBag(sum) lookup.
//
// Reference call sites replaced (see include/dlrm_hip.h):
//   prepack : DLRM_Net.quantize_embedding -> ops.quantized.embedding_bag_{byte,4bit}_prepack     dlrm_s_pytorch.py:465-481
//   lookup  : DLRM_Net.apply_emb          -> ops.quantized.embedding_bag_{byte,4bit}_rowwise_offsets   dlrm_s_pytorch.py:430-450
// The reference has these for the CPU only; here both run on the device.
//
// Packed row (torch's fused row-wise format, byte for byte):
//   8 bits: D bytes q[0..D), fp32 scale, fp32 bias                      -> D + 8 bytes
//   4 bits: D/2 bytes (column 2k in the low nibble, 2k+1 in the high nibble of byte k), fp16 scale, fp16 bias   -> D/2 + 4 bytes
//
// Prepack arithmetic (fp32, IEEE division, round to nearest even; no step of it can contract into an FMA):
//   8 bits: range = max - min; scale = range / 255; bias = min; inv = 255 / (range + 1e-8); q = clamp(rint((x - min) * inv), 0, 255)
//   4 bits: min = fp16(min); range = max - min; scale = fp16(range == 0 ? 1 : range / 15); scale == 0 -> 1; inv = 1 / scale,
//           inv infinite -> scale = inv = 1; bias = min; q = clamp(rint((x - min) * inv), 0, 15)
//
// Lookup arithmetic, per output element, rows of the bag in index order:
//   term = fmaf(scale_r, (float)q_r[d], bias_r)            one rounding (the fp16 scale / bias of the 4-bit form convert exactly)
//   acc  = fmaf(psw_i, term, acc)                          one rounding; psw_i = 1.0f when the bag has no per-sample weights, i.e. acc + term
// from acc = +0.0.  A lane owns its columns and sums the rows itself: no cross-lane reduction, so the result does not depend on the
// launch shape and two runs give the same bits.
//
// Lookup design (HBM-bound gather of 136 / 68 byte rows at D = 128):
//   * one launch covers every table (blockIdx.y = table, EmbArgs by value), as emb_fwd_kernel;
//   * D % 8 == 0: a lane owns 8 consecutive columns — one 8-byte (8 bits) or 4-byte (4 bits) load per row — and a group of D/8 lanes
//     owns a bag (16 lanes at D = 128: a wavefront works on 4 groups);  the scale/bias pair is one more load of the same row, issued
//     together with it;
//   * each group takes U bags at once and issues the U first-row loads back to back before any dependent arithmetic (the one-hot Criteo
//     case is latency-bound otherwise); longer bags continue with four row loads in flight;
//   * any other D (and unaligned operands): a byte-wise kernel, 16 lanes per bag, that only has to be correct.
#include "emb_lookup.h"

namespace {

__device__ __forceinline__ float f16_bits_to_f32(unsigned h) {
    union { unsigned short u; _Float16 f; } c; c.u = (unsigned short)h; return (float)c.f;
}
__device__ __forceinline__ unsigned f32_to_f16_bits(float x) {
    union { unsigned short u; _Float16 f; } c; c.f = (_Float16)x; return c.u;       // round to nearest even
}

// -------------------------------------------------------------------------------------------
// prepack
// -------------------------------------------------------------------------------------------
struct RowQuant { float bias, inv; unsigned scale_bits; };      // scale_bits: fp32 bits (8-bit form) or fp16 bits (4-bit form)

template <int BITS>
__device__ __forceinline__ RowQuant row_quant(float mn, float mx) {
    RowQuant q;
    if constexpr (BITS == 8) {
        const float range = mx - mn;
        q.bias = mn;
        q.scale_bits = __float_as_uint(range / 255.0f);
        q.inv = 255.0f / (range + 1e-8f);
    } else {
        mn = f16_bits_to_f32(f32_to_f16_bits(mn));
        const float range = mx - mn;
        float scale = range == 0.f ? 1.0f : range / 15.0f;
        unsigned sb = f32_to_f16_bits(scale);
        scale = f16_bits_to_f32(sb);
        if (scale == 0.f) { scale = 1.0f; sb = 0x3C00u; }
        float inv = 1.0f / scale;
        if (__builtin_isinf(inv)) { inv = 1.0f; sb = 0x3C00u; }
        q.bias = mn; q.inv = inv; q.scale_bits = sb;
    }
    return q;
}

template <int BITS>
__device__ __forceinline__ unsigned quant1(float x, const RowQuant& q) {
    constexpr float top = BITS == 8 ? 255.f : 15.f;
    const float v = rintf((x - q.bias) * q.inv);
    return (unsigned)fminf(fmaxf(v, 0.f), top);
}

__device__ __forceinline__ void store_le(uint8_t* p, unsigned v, int nbytes) {
    for (int k = 0; k < nbytes; ++k) p[k] = (uint8_t)(v >> (8 * k));
}

// A group of LPR lanes (a power of two, 4..64) owns a row: pass 1 takes min / max (xor shuffles inside the group), pass 2 reads the row
// again (from cache) and writes the codes; lane 0 of the group writes scale and bias.  VEC: four columns per lane and step (D % 4 == 0,
// 16-byte aligned table, 4-byte aligned output).
template <int BITS, bool VEC>
__global__ __launch_bounds__(256) void emb_quantize_rows_kernel(const float* __restrict__ W, uint8_t* __restrict__ out, long long rows,
                                                                int D, int LPR) {
    const long long RB = BITS == 8 ? (long long)D + 8 : (long long)D / 2 + 4;
    const int lig = threadIdx.x % LPR;
    const long long gpb = 256 / LPR;
    for (long long r = (long long)blockIdx.x * gpb + threadIdx.x / LPR; r < rows; r += (long long)gridDim.x * gpb) {
        const float* __restrict__ w = W + r * D;
        uint8_t* __restrict__ o = out + r * RB;
        float mn = __builtin_inff(), mx = -__builtin_inff();
        if constexpr (VEC) {
            for (int c = lig; c < D / 4; c += LPR) {
                const float4 v = *(const float4*)(w + 4 * c);
                mn = fminf(fminf(fminf(mn, v.x), fminf(v.y, v.z)), v.w);
                mx = fmaxf(fmaxf(fmaxf(mx, v.x), fmaxf(v.y, v.z)), v.w);
            }
        } else {
            for (int d = lig; d < D; d += LPR) { mn = fminf(mn, w[d]); mx = fmaxf(mx, w[d]); }
        }
        for (int s = 1; s < LPR; s <<= 1) {
            mn = fminf(mn, __shfl_xor(mn, s, 64));
            mx = fmaxf(mx, __shfl_xor(mx, s, 64));
        }
        const RowQuant q = row_quant<BITS>(mn, mx);
        if constexpr (VEC) {
            for (int c = lig; c < D / 4; c += LPR) {
                const float4 v = *(const float4*)(w + 4 * c);
                const unsigned a = quant1<BITS>(v.x, q), b = quant1<BITS>(v.y, q), cc = quant1<BITS>(v.z, q), d = quant1<BITS>(v.w, q);
                if constexpr (BITS == 8) *(unsigned*)(o + 4 * c) = a | (b << 8) | (cc << 16) | (d << 24);
                else *(unsigned short*)(o + 2 * c) = (unsigned short)(a | (b << 4) | (cc << 8) | (d << 12));
            }
        } else if constexpr (BITS == 8) {
            for (int d = lig; d < D; d += LPR) o[d] = (uint8_t)quant1<8>(w[d], q);
        } else {
            for (int p = lig; p < D / 2; p += LPR) o[p] = (uint8_t)(quant1<4>(w[2 * p], q) | (quant1<4>(w[2 * p + 1], q) << 4));
        }
        if (lig == 0) {
            if constexpr (BITS == 8) { store_le(o + D, q.scale_bits, 4); store_le(o + D + 4, __float_as_uint(q.bias), 4); }
            else { store_le(o + D / 2, q.scale_bits, 2); store_le(o + D / 2 + 2, f32_to_f16_bits(q.bias), 2); }
        }
    }
}

// -------------------------------------------------------------------------------------------
// lookup, D % 8 == 0: a lane owns columns [8 * lig, 8 * lig + 8)
// -------------------------------------------------------------------------------------------
template <int BITS> struct QRow;
template <> struct QRow<8> { uint2 q; float2 sb; };
template <> struct QRow<4> { unsigned q; unsigned sb; };

__device__ __forceinline__ void q_zero(QRow<8>& v) { v.q = make_uint2(0u, 0u); v.sb = make_float2(0.f, 0.f); }
__device__ __forceinline__ void q_zero(QRow<4>& v) { v.q = 0u; v.sb = 0u; }
// row: start of the packed row; col: first of the lane's 8 columns
__device__ __forceinline__ void q_load(QRow<8>& v, const uint8_t* __restrict__ row, int D, int col) {
    v.q = *(const uint2*)(row + col); v.sb = *(const float2*)(row + D);
}
__device__ __forceinline__ void q_load(QRow<4>& v, const uint8_t* __restrict__ row, int D, int col) {
    v.q = *(const unsigned*)(row + (col >> 1)); v.sb = *(const unsigned*)(row + (D >> 1));
}
// acc[j] = fma(w, fma(scale, q[j], bias), acc[j])
__device__ __forceinline__ void q_accum(float (&acc)[8], float w, const QRow<8>& v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[j] = __builtin_fmaf(w, __builtin_fmaf(v.sb.x, (float)((v.q.x >> (8 * j)) & 0xFFu), v.sb.y), acc[j]);
        acc[4 + j] = __builtin_fmaf(w, __builtin_fmaf(v.sb.x, (float)((v.q.y >> (8 * j)) & 0xFFu), v.sb.y), acc[4 + j]);
    }
}
__device__ __forceinline__ void q_accum(float (&acc)[8], float w, const QRow<4>& v) {
    const float scale = f16_bits_to_f32(v.sb & 0xFFFFu), bias = f16_bits_to_f32(v.sb >> 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(w, __builtin_fmaf(scale, (float)((v.q >> (4 * j)) & 0xFu), bias), acc[j]);
}

// emb_lookup.h's row source: the packed row's bytes, the lane's 8 codes and the row's scale / bias pair loaded together
template <int BITS>
struct QuantRows {
    using Elem = uint8_t;
    using Staged = QRow<BITS>;
    using Acc = float[8];
    static constexpr int COLS = 8;
    static __device__ __forceinline__ long long pitch(int D) { return BITS == 8 ? (long long)D + 8 : (long long)D / 2 + 4; }
    static __device__ __forceinline__ void zero(Staged& v) { q_zero(v); }
    static __device__ __forceinline__ void clear(Acc& a) {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = 0.f;
    }
    static __device__ __forceinline__ void load(Staged& v, const uint8_t* __restrict__ row, int D, int col) { q_load(v, row, D, col); }
    static __device__ __forceinline__ void accum(Acc& a, float w, const Staged& v) { q_accum(a, w, v); }
    static __device__ __forceinline__ void store(float* o, const Acc& a) { store8(o, a); }
};

template <int BITS, int LPB, typename IT, int U>
__global__ __launch_bounds__(256) void emb_fwd_quant_kernel(EmbArgs a, long long B, int D, float* __restrict__ out, long long out_ld) {
    emb_lookup_body<QuantRows<BITS>, LPB, 1, IT, U, false>(a, B, D, out, out_ld);
}

// -------------------------------------------------------------------------------------------
// lookup, any D (even D for 4 bits), any alignment: 16 lanes per bag, a lane walks its columns one after the other and, per column, the
// rows of the bag in index order — the same two FMAs per element as above, so both kernels give the same bits.
// -------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned load_le(const uint8_t* __restrict__ p, int nbytes) {
    unsigned v = 0;
    for (int k = 0; k < nbytes; ++k) v |= (unsigned)p[k] << (8 * k);
    return v;
}

template <int BITS, typename IT>
__global__ __launch_bounds__(256) void emb_fwd_quant_bytes_kernel(EmbArgs a, long long B, int D, float* __restrict__ out, long long out_ld) {
    if (a.pred.skip()) return;
    const int t = blockIdx.y;
    const uint8_t* __restrict__ W = (const uint8_t*)a.w[t];
    const IT* __restrict__ idx = (const IT*)a.idx[t];
    const IT* __restrict__ off = (const IT*)a.off[t];
    const float* __restrict__ psw = a.psw[t];
    const long long rows = a.rows[t];
    const long long RB = BITS == 8 ? (long long)D + 8 : (long long)D / 2 + 4;
    const long long b = (long long)blockIdx.x * 16 + threadIdx.x / 16;
    if (b >= B) return;
    const long long s = (long long)off[b];
    const long long e = (b + 1 < B) ? (long long)off[b + 1] : a.nnz[t];
    float* o = out + b * out_ld + (long long)a.slot[t] * D;
    for (int d = threadIdx.x % 16; d < D; d += 16) {
        float acc = 0.f;
        for (long long i = s; i < e; ++i) {
            const long long r = (long long)idx[i];
            if (!dlrm_index_ok(r, rows)) { dlrm_report_bad_index(a.err, a.slot[t], r, rows); continue; }
            const uint8_t* __restrict__ row = W + r * RB;
            float scale, bias, q;
            if constexpr (BITS == 8) {
                scale = __uint_as_float(load_le(row + D, 4)); bias = __uint_as_float(load_le(row + D + 4, 4));
                q = (float)row[d];
            } else {
                scale = f16_bits_to_f32(load_le(row + D / 2, 2)); bias = f16_bits_to_f32(load_le(row + D / 2 + 2, 2));
                q = (float)((row[d >> 1] >> ((d & 1) * 4)) & 0xFu);
            }
            acc = __builtin_fmaf(psw ? psw[i] : 1.f, __builtin_fmaf(scale, q, bias), acc);
        }
        o[d] = acc;
    }
}

constexpr int kU = 4;  // bags per lane group

template <int BITS, typename IT>
int launch_fwd_quant(int lpb, const EmbArgs& a, int n, long long B, int D, float* out, long long out_ld, hipStream_t st) {
    const dim3 block(256, 1, 1);
    if (lpb == 0) {
        const dim3 grid((unsigned)((B + 15) / 16), (unsigned)n, 1);
        hipLaunchKernelGGL((emb_fwd_quant_bytes_kernel<BITS, IT>), grid, block, 0, st, a, B, D, out, out_ld);
        return 0;
    }
    const long long bpb = (long long)(256 / lpb) * kU;
    const dim3 grid((unsigned)((B + bpb - 1) / bpb), (unsigned)n, 1);
    switch (lpb) {
        case 4:  hipLaunchKernelGGL((emb_fwd_quant_kernel<BITS, 4, IT, kU>), grid, block, 0, st, a, B, D, out, out_ld); break;
        case 8:  hipLaunchKernelGGL((emb_fwd_quant_kernel<BITS, 8, IT, kU>), grid, block, 0, st, a, B, D, out, out_ld); break;
        case 16: hipLaunchKernelGGL((emb_fwd_quant_kernel<BITS, 16, IT, kU>), grid, block, 0, st, a, B, D, out, out_ld); break;
        case 32: hipLaunchKernelGGL((emb_fwd_quant_kernel<BITS, 32, IT, kU>), grid, block, 0, st, a, B, D, out, out_ld); break;
        case 64: hipLaunchKernelGGL((emb_fwd_quant_kernel<BITS, 64, IT, kU>), grid, block, 0, st, a, B, D, out, out_ld); break;
        default: return DLRM_E_RANGE;
    }
    return 0;
}

}  // namespace

extern "C" int dlrm_emb_quantize_rows(int64_t rows, int D, int bits, const float* weight, void* packed, void* stream) {
    if (rows <= 0 || D <= 0 || !weight || !packed) return DLRM_E_ARG;
    if (bits != 4 && bits != 8) return DLRM_E_MODE;
    DLRM_REQUIRE(bits == 8 || D % 2 == 0, DLRM_E_ARG, "the 4-bit row format needs an even embedding dimension");
    hipStream_t st = (hipStream_t)stream;
    const bool vec = D % 4 == 0 && dlrm_aligned16(weight) && (((uintptr_t)packed) & 3u) == 0;
    const int lpr = lanes_per_bag(vec ? D / 4 : (bits == 4 ? D / 2 : D));
    const long long gpb = 256 / lpr;
    long long nb = (rows + gpb - 1) / gpb;
    if (nb > (1LL << 20)) nb = 1LL << 20;            // grid stride beyond that
    const dim3 grid((unsigned)nb), block(256);
    uint8_t* o = (uint8_t*)packed;
    if (bits == 8) {
        if (vec) hipLaunchKernelGGL((emb_quantize_rows_kernel<8, true>), grid, block, 0, st, weight, o, (long long)rows, D, lpr);
        else     hipLaunchKernelGGL((emb_quantize_rows_kernel<8, false>), grid, block, 0, st, weight, o, (long long)rows, D, lpr);
    } else {
        if (vec) hipLaunchKernelGGL((emb_quantize_rows_kernel<4, true>), grid, block, 0, st, weight, o, (long long)rows, D, lpr);
        else     hipLaunchKernelGGL((emb_quantize_rows_kernel<4, false>), grid, block, 0, st, weight, o, (long long)rows, D, lpr);
    }
    DLRM_LAUNCH_CHECK();
    return 0;
}

static int emb_fwd_quant_impl(int T, int64_t B, int D, int bits, const void* const* weight_host, const int64_t* rows_host,
                              const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                              const void* const* psw_host, int idx_bits, float* out, int64_t out_ld, int64_t* err, DlrmPred pred, void* stream);

extern "C" int dlrm_emb_fwd_quant(int T, int64_t B, int D, int bits, const void* const* weight_host, const int64_t* rows_host,
                                  const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                                  const void* const* psw_host, int idx_bits, float* out, int64_t out_ld, int64_t* err, void* stream) {
    return emb_fwd_quant_impl(T, B, D, bits, weight_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, idx_bits, out, out_ld, err,
                              DlrmPred{nullptr, 0}, stream);
}

// the same kernels behind a launch predicate (as dlrm_emb_fwd_pred beside dlrm_emb_fwd): the two-kernel form of a quantised forward whose
// fused form (dlrm_interact_fwd_gather_quant) was enqueued with the opposite predicate
extern "C" int dlrm_emb_fwd_quant_pred(int T, int64_t B, int D, int bits, const void* const* weight_host, const int64_t* rows_host,
                                       const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                                       const void* const* psw_host, int idx_bits, float* out, int64_t out_ld, int64_t* err,
                                       const int32_t* pred_flag, int pred_nonzero, void* stream) {
    return emb_fwd_quant_impl(T, B, D, bits, weight_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, idx_bits, out, out_ld, err,
                              DlrmPred{(const int*)pred_flag, pred_nonzero}, stream);
}

static int emb_fwd_quant_impl(int T, int64_t B, int D, int bits, const void* const* weight_host, const int64_t* rows_host,
                              const void* const* indices_host, const void* const* offsets_host, const int64_t* nnz_host,
                              const void* const* psw_host, int idx_bits, float* out, int64_t out_ld, int64_t* err, DlrmPred pred, void* stream) {
    int rc = emb_check_lists(T, B, D, weight_host, rows_host, indices_host, offsets_host, nnz_host, idx_bits);
    if (rc) return rc;
    if (bits != 4 && bits != 8) return DLRM_E_MODE;
    DLRM_REQUIRE(bits == 8 || D % 2 == 0, DLRM_E_ARG, "the 4-bit row format needs an even embedding dimension");
    if (emb_check_tables(T, weight_host, rows_host, indices_host, offsets_host, nnz_host)) return DLRM_E_ARG;
    if (!out || out_ld < (int64_t)T * D) return DLRM_E_ARG;
    hipStream_t st = (hipStream_t)stream;

    // the 8-columns-per-lane kernel: rows that start on an 8-byte (8 bits) / 4-byte (4 bits) boundary, float4 stores into out
    const uintptr_t row_align = bits == 8 ? 7u : 3u;
    bool vec_ok = D % 8 == 0 && D <= 512 && dlrm_aligned16(out) && (out_ld % 4 == 0);
    for (int t = 0; t < T; ++t) vec_ok = vec_ok && (((uintptr_t)weight_host[t]) & row_align) == 0;
    int lpb = 0;                                     // 0: the byte-wise kernel
    if (vec_ok) lpb = lanes_per_bag(D / 8);

    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
        EmbArgs a;
        emb_fill_args(a, t0, n, weight_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, err, pred);
        if (bits == 8) rc = idx_bits == 64 ? launch_fwd_quant<8, long long>(lpb, a, n, B, D, out, out_ld, st)
                                           : launch_fwd_quant<8, int>(lpb, a, n, B, D, out, out_ld, st);
        else           rc = idx_bits == 64 ? launch_fwd_quant<4, long long>(lpb, a, n, B, D, out, out_ld, st)
                                           : launch_fwd_quant<4, int>(lpb, a, n, B, D, out, out_ld, st);
        if (rc) return rc;
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}
