// gemm_q8.hip — dynamically quantised int8 Linear layers for inference (the reference's --quantize-mlp-with-bit 8:
// torch.quantization.quantize_dynamic(dlrm, {nn.Linear}, qint8), dlrm_s_pytorch.py:1473-1480), on the int8 MFMA of gfx950.
//
//   weight, once    : s_w = max(max|W| / 127.5, eps), wq = clamp(rint(W * (1 / s_w)), -128, 127)            (dlrm_q8_pack_weight)
//   activation, call: per-tensor range over the whole [M, K] input, reduced range 0..127, zero point as fbgemm's ChooseQuantizationParams,
//                     xq = clamp(rint(x * (1 / s_x)) + zp, 0, 127); stored SHIFTED (xq - zp, in [-127, 127])   (dlrm_q8_quantize_act)
//   output          : out = act(float(sum_k (xq - zp) wq) * (s_x * s_w) + bias)                              (dlrm_gemm_q8)
// Every step is exact (min / max, one rounding per element, integer accumulation), so the results do not depend on tiling, grid or order:
// they are the bits of the numpy restatement in tests/test_quant_mlp_host.py.  The quantisation parameters never leave the device.
//
// Operand layout: both operands are int8 row-major with the reduction index contiguous and padded with zero codes to a multiple of 64
// (K64) — [M, K64] activations, [N, K64] weights — so each lane of an MFMA takes 16 consecutive k of one row with one 16-byte read, from
// the SAME k positions for A and for B.  Whatever order the instruction gives those 16 bytes inside its k-step, both operands share it and
// the integer sum is the same (tests: identity against an asymmetric matrix, both ways).
#include "common.h"
#include <math.h>

// Every fp32 operation of this file is rounded on its own: the contract of these kernels is one rounding per operation (float(acc) * scale,
// then + bias).  hipcc contracts a * b + c into one fma by default, and __fmul_rn / __fadd_rn do not stop it: they are plain `*` / `+` in
// a header compiled before this pragma, so their instructions still carry the permission to fuse once inlined.  The products and sums
// below are therefore written through q8_mul / q8_add, which are compiled under the pragma.
#pragma clang fp contract(off)

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int Q8_PARTIAL_BLOCKS = 1024;                 // range partials: 2 floats per block of the range pass
constexpr float Q8_WEIGHT_EPS = 1.1920928955078125e-07f; // torch's observer floor of a scale (finfo(float32).eps)

__device__ __forceinline__ float q8_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float q8_add(float a, float b) { return a + b; }

__host__ __device__ inline int q8_k64(int K) { return (K + 63) & ~63; }

__device__ __forceinline__ float q8_act(float v, int act) {
    if (act == DLRM_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == DLRM_ACT_SIGMOID) return 1.f / (1.f + expf(-v));
    return v;
}

__device__ __forceinline__ int q8_clampi(float v, float lo, float hi) {
    // (a NaN comes out as lo: fmaxf returns the other operand)
    return (int)fminf(fmaxf(v, lo), hi);
}

// ------------------------------------------------------------------------------------------------ weights
// one workgroup: max |W| over [N, K] (row stride ldw) -> s_w[0] = scale, s_w[1] = 1 / scale
__global__ __launch_bounds__(1024) void q8_weight_scale_kernel(int N, int K, const float* __restrict__ W, long long ldw, float* __restrict__ s_w) {
    __shared__ float red[16];
    float m = 0.f;
    const long long total = (long long)N * K;
    for (long long e = threadIdx.x; e < total; e += 1024) {
        const long long r = e / K;
        m = fmaxf(m, fabsf(W[r * ldw + (e - r * K)]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]);
        const float s = fmaxf(__fdiv_rn(m, 127.5f), Q8_WEIGHT_EPS);
        s_w[0] = s;
        s_w[1] = __fdiv_rn(1.0f, s);
    }
}

// wq[n, k] = clamp(rint(W[n, k] * inv), -128, 127) for k < K, 0 for K <= k < K64; four codes per thread, one 4-byte store
__global__ __launch_bounds__(256) void q8_weight_codes_kernel(int N, int K, int K64, const float* __restrict__ W, long long ldw,
                                                              const float* __restrict__ s_w, int* __restrict__ wq) {
    const float inv = s_w[1];
    const int qpr = K64 >> 2;
    const long long total = (long long)N * qpr;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
        const long long n = q / qpr;
        const int k0 = (int)(q - n * qpr) << 2;
        unsigned packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + j;
            int c = 0;
            if (k < K) c = q8_clampi(rintf(q8_mul(W[n * ldw + k], inv)), -128.f, 127.f);
            packed |= (unsigned)(c & 255) << (8 * j);
        }
        wq[q] = (int)packed;
    }
}

// ------------------------------------------------------------------------------------------------ activations
// Lane map of the two activation passes: a wave takes `64 / P` rows at a time, P = min(64, next power of two >= items per row); lane l is
// item (l & (P - 1)) + j * P of row (l / P).  Narrow inputs (13 dense features) keep their lanes busy, wide ones read a row coalesced.
__device__ __forceinline__ int q8_pow2_items(int items) {
    int p = 1;
    while (p < items && p < 64) p <<= 1;
    return p;
}

__host__ inline int q8_range_blocks(long long M, int K) {
    int p = 1;
    while (p < K && p < 64) p <<= 1;
    const long long passes = (M + (64 / p) - 1) / (64 / p);         // wave passes over the rows
    long long nb = (passes + 3) / 4;
    if (nb > Q8_PARTIAL_BLOCKS) nb = Q8_PARTIAL_BLOCKS;
    return nb < 1 ? 1 : (int)nb;
}

// partial[2 b] = min, partial[2 b + 1] = max over the rows block b visits (seeded with 0: the range always contains 0)
__global__ __launch_bounds__(256) void q8_range_kernel(long long M, int K, const float* __restrict__ X, long long ldx, float* __restrict__ partial) {
    __shared__ float red[8];
    const int P = q8_pow2_items(K), rpw = 64 / P, shift = __builtin_ctz(P);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float mn = 0.f, mx = 0.f;
    const long long stride = (long long)gridDim.x * 4 * rpw;
    for (long long r = ((long long)blockIdx.x * 4 + wave) * rpw + (lane >> shift); r < M; r += stride) {
        const float* row = X + r * ldx;
        for (int k = lane & (P - 1); k < K; k += P) {
            const float v = row[k];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) { red[2 * wave] = mn; red[2 * wave + 1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { mn = fminf(mn, red[2 * w]); mx = fmaxf(mx, red[2 * w + 1]); }
        partial[2 * blockIdx.x] = mn;
        partial[2 * blockIdx.x + 1] = mx;
    }
}

// torch's dynamic Linear (reduce_range: codes 0..127) -> {s_x, zero point, 1 / s_x}: ATen's ChooseQuantizationParams in double
__device__ inline void q8_choose_params(float mnf, float mxf, float* s_out, float* zp_out, float* inv_out) {
    const double mn = (double)fminf(mnf, 0.f), mx = (double)fmaxf(mxf, 0.f);
    double s = (mx - mn) / 127.0;
    const float sf = (float)s;
    if (sf == 0.0f || isinf(__fdiv_rn(1.0f, sf))) s = 0.1;
    const double z_min = 0.0 - mn / s, z_max = 127.0 - mx / s;
    const double e_min = fabs(mn / s), e_max = 127.0 + fabs(mx / s);
    const double z = e_min < e_max ? z_min : z_max;
    double zp = 0.0;
    if (z >= 127.0) zp = 127.0;
    else if (z > 0.0) zp = rint(z);                      // (a NaN range gives 0)
    const float sx = (float)s;
    *s_out = sx;
    *zp_out = (float)zp;
    *inv_out = __fdiv_rn(1.0f, sx);
}

// every workgroup folds the range partials itself (at most 1024 pairs), derives the parameters, and writes shifted codes:
// xq[m, k] = clamp(rint(x * inv) + zp, 0, 127) - zp for k < K, 0 up to K64.  Workgroup 0 publishes the parameters for the GEMM.
__global__ __launch_bounds__(256) void q8_quantize_kernel(long long M, int K, int K64, const float* __restrict__ X, long long ldx,
                                                          const float* __restrict__ partial, int npartial, int* __restrict__ xq,
                                                          float* __restrict__ qparams) {
    __shared__ float red[8];
    __shared__ float prm[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float mn = 0.f, mx = 0.f;
    for (int b = threadIdx.x; b < npartial; b += 256) {
        mn = fminf(mn, partial[2 * b]);
        mx = fmaxf(mx, partial[2 * b + 1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) { red[2 * wave] = mn; red[2 * wave + 1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { mn = fminf(mn, red[2 * w]); mx = fmaxf(mx, red[2 * w + 1]); }
        q8_choose_params(mn, mx, &prm[0], &prm[1], &prm[2]);
        if (blockIdx.x == 0) { qparams[0] = prm[0]; qparams[1] = prm[1]; qparams[2] = prm[2]; qparams[3] = 0.f; }
    }
    __syncthreads();
    const float zp = prm[1], inv = prm[2];
    const int qpr = K64 >> 2;                                        // 4-code words per row
    const int P = q8_pow2_items(qpr), rpw = 64 / P, shift = __builtin_ctz(P);
    const long long stride = (long long)gridDim.x * 4 * rpw;
    for (long long r = ((long long)blockIdx.x * 4 + wave) * rpw + (lane >> shift); r < M; r += stride) {
        const float* row = X + r * ldx;
        int* dst = xq + r * qpr;
        for (int q = lane & (P - 1); q < qpr; q += P) {
            unsigned packed = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 4 * q + j;
                if (k < K) {
                    const float c = fminf(fmaxf(q8_add(rintf(q8_mul(row[k], inv)), zp), 0.f), 127.f);
                    packed |= (unsigned)((int)(c - zp) & 255) << (8 * j);
                }
            }
            dst[q] = (int)packed;
        }
    }
}

// ------------------------------------------------------------------------------------------------ GEMM on v_mfma_i32_32x32x32_i8
// 128 x 128 outputs per workgroup of 4 waves (each 64 x 64 = 2 x 2 MFMA tiles), k-tiles of 64 codes staged in LDS.  LDS rows are 80 bytes
// (64 + 16): the 16-byte reads of 16 consecutive rows then fall into 16 different 16-byte bank groups.  The next k-tile's global loads
// are issued before the MFMAs of the current one.
constexpr int Q8_BM = 128, Q8_BN = 128, Q8_BK = 64, Q8_LDS_ROW = 80;

__global__ __launch_bounds__(256) void q8_gemm_kernel(long long M, int N, int K64, const int8_t* __restrict__ A, const int8_t* __restrict__ B,
                                                     const float* __restrict__ qparams, const float* __restrict__ s_w,
                                                     const float* __restrict__ bias, int act, float* __restrict__ out, long long ldo,
                                                     int blocks_n) {
    __shared__ __attribute__((aligned(16))) int8_t sA[Q8_BM * Q8_LDS_ROW];
    __shared__ __attribute__((aligned(16))) int8_t sB[Q8_BN * Q8_LDS_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)(blockIdx.x / blocks_n) * Q8_BM;
    const int n0 = (int)(blockIdx.x % blocks_n) * Q8_BN;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

    // staging: 128 rows x 4 chunks of 16 bytes per operand; thread t takes chunks t and t + 256
    const int srow0 = tid >> 2, srow1 = srow0 + 64, schunk = tid & 3;
    const bool a_ok0 = m0 + srow0 < M, a_ok1 = m0 + srow1 < M;
    const bool b_ok0 = n0 + srow0 < N, b_ok1 = n0 + srow1 < N;
    const int8_t* ga0 = A + (m0 + srow0) * K64 + schunk * 16;
    const int8_t* ga1 = A + (m0 + srow1) * K64 + schunk * 16;
    const int8_t* gb0 = B + (long long)(n0 + srow0) * K64 + schunk * 16;
    const int8_t* gb1 = B + (long long)(n0 + srow1) * K64 + schunk * 16;
    const v4i zero4 = {0, 0, 0, 0};
    v4i ra0, ra1, rb0, rb1;
    auto load_tile = [&](int k) {
        ra0 = a_ok0 ? *reinterpret_cast<const v4i*>(ga0 + k) : zero4;
        ra1 = a_ok1 ? *reinterpret_cast<const v4i*>(ga1 + k) : zero4;
        rb0 = b_ok0 ? *reinterpret_cast<const v4i*>(gb0 + k) : zero4;
        rb1 = b_ok1 ? *reinterpret_cast<const v4i*>(gb1 + k) : zero4;
    };

    v16i acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    const int frow = lane & 31, fk = (lane >> 5) * 16;               // fragment: row (lane & 31), 16 codes from k = 16 (lane >> 5)
    load_tile(0);
    for (int k = 0; k < K64; k += Q8_BK) {
        *reinterpret_cast<v4i*>(sA + srow0 * Q8_LDS_ROW + schunk * 16) = ra0;
        *reinterpret_cast<v4i*>(sA + srow1 * Q8_LDS_ROW + schunk * 16) = ra1;
        *reinterpret_cast<v4i*>(sB + srow0 * Q8_LDS_ROW + schunk * 16) = rb0;
        *reinterpret_cast<v4i*>(sB + srow1 * Q8_LDS_ROW + schunk * 16) = rb1;
        __syncthreads();
        if (k + Q8_BK < K64) load_tile(k + Q8_BK);
#pragma unroll
        for (int ks = 0; ks < Q8_BK; ks += 32) {
            v4i fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *reinterpret_cast<const v4i*>(sA + (wm + i * 32 + frow) * Q8_LDS_ROW + ks + fk);
                fb[i] = *reinterpret_cast<const v4i*>(sB + (wn + i * 32 + frow) * Q8_LDS_ROW + ks + fk);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // D[i][j]: column j = lane & 31 (the weight row), row i = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (the activation row)
    const float scale = q8_mul(qparams[0], s_w[0]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn + j * 32 + (lane & 31);
        if (n >= N) continue;
        const float bv = bias ? bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m < M) {
                    float y = q8_mul((float)acc[i][j][r], scale);
                    if (bias) y = q8_add(y, bv);
                    out[m * ldo + n] = q8_act(y, act);
                }
            }
        }
    }
}

// narrow layers (N <= 8: the 256 -> 1 head): one thread per output, 4-way int8 dot products over the row pair
__global__ __launch_bounds__(256) void q8_dot_kernel(long long M, int N, int K64, const int8_t* __restrict__ A, const int8_t* __restrict__ B,
                                                    const float* __restrict__ qparams, const float* __restrict__ s_w,
                                                    const float* __restrict__ bias, int act, float* __restrict__ out, long long ldo) {
    const float scale = q8_mul(qparams[0], s_w[0]);
    const long long total = M * N;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long m = e / N;
        const int n = (int)(e - m * N);
        const v4i* a = reinterpret_cast<const v4i*>(A + m * K64);
        const v4i* b = reinterpret_cast<const v4i*>(B + (long long)n * K64);
        int acc = 0;
        for (int c = 0; c < (K64 >> 4); ++c) {
            const v4i av = a[c], bv = b[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_sdot4(av[j], bv[j], acc, false);
        }
        float y = q8_mul((float)acc, scale);
        if (bias) y = q8_add(y, bias[n]);
        out[m * ldo + n] = q8_act(y, act);
    }
}

}  // namespace

extern "C" {

int dlrm_q8_pack_weight(int N, int K, const float* W, int64_t ldw, void* wq, float* s_w, void* stream) {
    DLRM_REQUIRE(W && wq && s_w, DLRM_E_ARG, "null pointer");
    DLRM_REQUIRE(N >= 1 && K >= 1 && ldw >= K, DLRM_E_ARG, "bad size");
    DLRM_REQUIRE((((uintptr_t)wq) & 15u) == 0, DLRM_E_ALIGN, "packed weights must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int K64 = q8_k64(K);
    hipLaunchKernelGGL(q8_weight_scale_kernel, dim3(1), dim3(1024), 0, st, N, K, W, (long long)ldw, s_w);
    DLRM_LAUNCH_CHECK();
    long long nb = ((long long)N * (K64 >> 2) + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(q8_weight_codes_kernel, dim3((unsigned)nb), dim3(256), 0, st, N, K, K64, W, (long long)ldw, (const float*)s_w, (int*)wq);
    DLRM_LAUNCH_CHECK();
    return 0;
}

int64_t dlrm_q8_workspace_bytes(int64_t M, int K) {
    (void)M; (void)K;
    return (int64_t)Q8_PARTIAL_BLOCKS * 2 * sizeof(float);
}

int dlrm_q8_quantize_act(int64_t M, int K, const float* X, int64_t ldx, void* xq, float* qparams, void* workspace, int64_t workspace_bytes,
                         int phases, void* stream) {
    DLRM_REQUIRE(X && xq && qparams && workspace, DLRM_E_ARG, "null pointer");
    DLRM_REQUIRE(M >= 1 && K >= 1 && ldx >= K, DLRM_E_ARG, "bad size");
    DLRM_REQUIRE(workspace_bytes >= dlrm_q8_workspace_bytes(M, K), DLRM_E_ARG, "workspace too small");
    DLRM_REQUIRE((((uintptr_t)xq) & 15u) == 0 && (((uintptr_t)workspace) & 3u) == 0, DLRM_E_ALIGN, "codes must be 16-byte aligned");
    DLRM_REQUIRE(phases >= 1 && phases <= 3, DLRM_E_MODE, "phases is 1 (range), 2 (quantize) or 3 (both)");
    hipStream_t st = (hipStream_t)stream;
    const int K64 = q8_k64(K);
    const int nb = q8_range_blocks(M, K);
    if (phases & DLRM_Q8_RANGE) {
        hipLaunchKernelGGL(q8_range_kernel, dim3(nb), dim3(256), 0, st, (long long)M, K, X, (long long)ldx, (float*)workspace);
        DLRM_LAUNCH_CHECK();
    }
    if (phases & DLRM_Q8_QUANTIZE) {
        int p = 1;
        while (p < (K64 >> 2) && p < 64) p <<= 1;
        long long qb = ((M + (64 / p) - 1) / (64 / p) + 3) / 4;
        if (qb > 8192) qb = 8192;
        hipLaunchKernelGGL(q8_quantize_kernel, dim3((unsigned)qb), dim3(256), 0, st, (long long)M, K, K64, X, (long long)ldx,
                           (const float*)workspace, nb, (int*)xq, qparams);
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}

int dlrm_gemm_q8(int64_t M, int N, int K, const void* xq, const void* wq, const float* qparams, const float* s_w, const float* bias,
                 int act, float* out, int64_t ld_out, void* stream) {
    DLRM_REQUIRE(xq && wq && qparams && s_w && out, DLRM_E_ARG, "null pointer");
    DLRM_REQUIRE(M >= 1 && N >= 1 && K >= 1 && ld_out >= N, DLRM_E_ARG, "bad size");
    if (act < DLRM_ACT_NONE || act > DLRM_ACT_SIGMOID) return DLRM_E_MODE;
    DLRM_REQUIRE(dlrm_aligned16(xq) && dlrm_aligned16(wq), DLRM_E_ALIGN, "int8 operands must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int K64 = q8_k64(K);
    if (N <= 8) {
        long long nb = (M * N + 255) / 256;
        if (nb > 65536) nb = 65536;
        hipLaunchKernelGGL(q8_dot_kernel, dim3((unsigned)nb), dim3(256), 0, st, (long long)M, N, K64, (const int8_t*)xq, (const int8_t*)wq,
                           qparams, s_w, bias, act, out, (long long)ld_out);
        DLRM_LAUNCH_CHECK();
        return 0;
    }
    const long long blocks_m = (M + Q8_BM - 1) / Q8_BM;
    const int blocks_n = (N + Q8_BN - 1) / Q8_BN;
    DLRM_REQUIRE(blocks_m * blocks_n < (1ll << 31), DLRM_E_RANGE, "too many output tiles");
    hipLaunchKernelGGL(q8_gemm_kernel, dim3((unsigned)(blocks_m * blocks_n)), dim3(256), 0, st, (long long)M, N, K64, (const int8_t*)xq,
                       (const int8_t*)wq, qparams, s_w, bias, act, out, (long long)ld_out, blocks_n);
    DLRM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
