// interact_proj.hip — the projected interaction of torchrec's DLRM_Projection: per sample Z = A . Bm with A = P1[b] viewed [I1, D] and
// Bm = P2[b] viewed [D, I2], R[b] = [x[b] | Z row-major | zero padding]; backward dA = dZ . Bm^T, dBm = A^T . dZ, dx = dR[:, :D].
//
// Two paths inside each entry point (the caller never chooses):
//   fast    : one WAVE (a 64-thread workgroup) per sample.  The sample's A (row stride D + 4: the MFMA operand reads of 16 rows then fall
//             into 16 different bank groups), Bm (as it lies in memory) and, in backward, dZ (row stride I2 + 1) are staged in LDS with
//             16-byte loads; every 16 x 16 tile of an output is one chain of v_mfma_f32_16x16x4_f32 split over TWO accumulators (k-steps
//             alternate between them: the instruction's 40-cycle dependent latency is hidden behind its 32-cycle issue), summed at the end.
//             Lanes beyond a matrix edge feed results nobody stores and k beyond the sum is fed as zeros, so any I1, I2 <= 32 and any
//             D % 4 == 0 take this path.  LDS per workgroup is 16.6 KB forward / 17.7 KB backward at (16, 16, 128): nine workgroups per
//             CU fit, the loads of one overlap the products and stores of the others.  The kernels are memory-bound.
//   generic : one thread per output element, operands from global memory, scalar loads: any D, I1, I2, alignment and pitch.
// fp32 throughout (the f32 MFMA is an exact fma chain), no atomics; sample b's outputs depend on sample b's inputs only and the order of
// every sum is fixed by (D, I1, I2) and the path, so results do not depend on B or on the sample's position in the batch.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PROJ_MAX_I = 32;                 // fast path: I1, I2 <= 32
constexpr int PROJ_MAX_LDS = 64 * 1024;        // fast path: staged operands of one sample fit the default per-workgroup LDS limit
constexpr unsigned PROJ_MAX_GRID = 1u << 20;   // workgroups stride over the batch beyond this

// acc[16 x 16 tile at (m0, n0)] = sum_k a[m, k] * b[k, n] over k in [0, K), both operands in LDS: a[m, k] = A[m * ars + k * aks] (M rows),
// b[k, n] = Bp[n * bcs + k * bks] (N columns).  Lane l feeds a[m0 + (l & 15), k0 + (l >> 4)] and b[k0 + (l >> 4), n0 + (l & 15)]; result
// register r of lane l is row m0 + 4 * (l >> 4) + r, column n0 + (l & 15).  A lane whose row (column) lies beyond the matrix reads the last
// row (column) instead: it only feeds results the caller does not store.  k beyond K is fed as zeros on both sides (the tail step).
// k-steps alternate between two accumulators; the loop carries two pointers and no other address arithmetic.
__device__ __forceinline__ f32x4 proj_tile(const float* A, int ars, int aks, int M, const float* Bp, int bcs, int bks, int N, int K, int m0, int n0,
                                           int lane) {
    const int r = lane & 15, q = lane >> 4;
    const float* pa = A + min(m0 + r, M - 1) * ars + q * aks;
    const float* pb = Bp + min(n0 + r, N - 1) * bcs + q * bks;
    const int a4 = 4 * aks, b4 = 4 * bks;
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
    int k0 = 0;
    for (; k0 + 16 <= K; k0 += 16) {                      // eight operand reads in flight in front of four products
        const float a0 = pa[0], b0 = pb[0], a1 = pa[a4], b1 = pb[b4], a2 = pa[2 * a4], b2 = pb[2 * b4], a3 = pa[3 * a4], b3 = pb[3 * b4];
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b3, c1, 0, 0, 0);
        pa += 4 * a4;
        pb += 4 * b4;
    }
    for (; k0 + 8 <= K; k0 += 8) {
        const float a0 = pa[0], b0 = pb[0], a1 = pa[a4], b1 = pb[b4];
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, c1, 0, 0, 0);
        pa += 2 * a4;
        pb += 2 * b4;
    }
    if (k0 < K) {                                        // 1 .. 7 values of k are left
        const bool v0 = k0 + q < K, v1 = k0 + 4 + q < K;
        const float a0 = pa[v0 ? 0 : -q * aks], b0 = pb[v0 ? 0 : -q * bks];          // (an address inside the matrix either way)
        const float a1 = pa[v1 ? a4 : -q * aks], b1 = pb[v1 ? b4 : -q * bks];
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v0 ? a0 : 0.f, v0 ? b0 : 0.f, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v1 ? a1 : 0.f, v1 ? b1 : 0.f, c1, 0, 0, 0);
    }
    return c0 + c1;
}

// rows x cols floats (cols % 4 == 0, 16-byte aligned source) -> LDS at row stride `stride` (stride % 4 == 0)
__device__ __forceinline__ void proj_stage(float* __restrict__ dst, int stride, const float* __restrict__ src, int rows, int cols, int lane) {
    const int c4 = cols >> 2, n4 = rows * c4;
#pragma unroll 8
    for (int e = lane; e < n4; e += DLRM_WAVE) {
        const int row = e / c4, c = e - row * c4;
        const float4 v = reinterpret_cast<const float4*>(src)[e];
        *reinterpret_cast<float4*>(dst + row * stride + 4 * c) = v;
    }
}

__global__ __launch_bounds__(DLRM_WAVE) void proj_interact_fwd_kernel(long long B, int D, int I1, int I2, const float* __restrict__ x,
                                                                      long long x_ld, const float* __restrict__ P1, long long p1_ld,
                                                                      const float* __restrict__ P2, long long p2_ld, float* __restrict__ R,
                                                                      long long ldr) {
    extern __shared__ float4 proj_lds4[];
    float* sA = reinterpret_cast<float*>(proj_lds4);      // [I1][D + 4]
    const int SA = D + 4;
    float* sB = sA + I1 * SA;                             // [D][I2]
    const int lane = threadIdx.x;
    const int W = D + I1 * I2;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        proj_stage(sA, SA, P1 + b * p1_ld, I1, D, lane);
        proj_stage(sB, D * I2, P2 + b * p2_ld, 1, D * I2, lane);
        float* Rb = R + b * ldr;
        const float* xb = x + b * x_ld;
        for (int c = lane; c < (D >> 2); c += DLRM_WAVE) reinterpret_cast<float4*>(Rb)[c] = reinterpret_cast<const float4*>(xb)[c];
        for (long long c = W + lane; c < ldr; c += DLRM_WAVE) Rb[c] = 0.f;
        __syncthreads();
        for (int m0 = 0; m0 < I1; m0 += 16)
            for (int n0 = 0; n0 < I2; n0 += 16) {
                const f32x4 z = proj_tile(sA, SA, 1, I1, sB, 1, I2, I2, D, m0, n0, lane);       // a[i, k] = A[i, k], b[k, j] = Bm[k, j]
                const int j = n0 + (lane & 15), i0 = m0 + 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (i0 + r < I1 && j < I2) Rb[D + (i0 + r) * I2 + j] = z[r];
            }
        __syncthreads();                                  // the next sample's staging overwrites the operands
    }
}

__global__ __launch_bounds__(DLRM_WAVE) void proj_interact_bwd_kernel(long long B, int D, int I1, int I2, const float* __restrict__ P1,
                                                                      long long p1_ld, const float* __restrict__ P2, long long p2_ld,
                                                                      const float* __restrict__ dR, long long ldr, float* __restrict__ dx,
                                                                      long long dx_ld, float* __restrict__ dP1, long long dp1_ld,
                                                                      float* __restrict__ dP2, long long dp2_ld) {
    extern __shared__ float4 proj_lds4[];
    float* sA = reinterpret_cast<float*>(proj_lds4);      // [I1][D + 4]
    const int SA = D + 4, SZ = I2 + 1;
    float* sB = sA + I1 * SA;                             // [D][I2]
    float* sZ = sB + D * I2;                              // [I1][I2 + 1]
    const int lane = threadIdx.x;
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        proj_stage(sA, SA, P1 + b * p1_ld, I1, D, lane);
        proj_stage(sB, D * I2, P2 + b * p2_ld, 1, D * I2, lane);
        const float* dRb = dR + b * ldr;
        for (int e = lane; e < I1 * I2; e += DLRM_WAVE) {
            const int i = e / I2;
            sZ[i * SZ + (e - i * I2)] = dRb[D + e];
        }
        float* dxb = dx + b * dx_ld;
        for (int c = lane; c < (D >> 2); c += DLRM_WAVE) reinterpret_cast<float4*>(dxb)[c] = reinterpret_cast<const float4*>(dRb)[c];
        __syncthreads();
        // dA[i, d] = sum_j dZ[i, j] * Bm[d, j]:  a[i, j] = dZ[i, j], b[j, d] = Bm[d, j]
        float* dA = dP1 + b * dp1_ld;
        for (int m0 = 0; m0 < I1; m0 += 16)
            for (int n0 = 0; n0 < D; n0 += 16) {
                const f32x4 g = proj_tile(sZ, SZ, 1, I1, sB, I2, 1, D, I2, m0, n0, lane);
                const int d = n0 + (lane & 15), i0 = m0 + 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (i0 + r < I1 && d < D) dA[(i0 + r) * D + d] = g[r];
            }
        // dBm[d, j] = sum_i A[i, d] * dZ[i, j]:  a[d, i] = A[i, d], b[i, j] = dZ[i, j]
        float* dBm = dP2 + b * dp2_ld;
        for (int m0 = 0; m0 < D; m0 += 16)
            for (int n0 = 0; n0 < I2; n0 += 16) {
                const f32x4 g = proj_tile(sA, 1, SA, D, sZ, 1, SZ, I2, I1, m0, n0, lane);
                const int j = n0 + (lane & 15), d0 = m0 + 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (d0 + r < D && j < I2) dBm[(d0 + r) * I2 + j] = g[r];
            }
        __syncthreads();
    }
}

// generic forward: one thread per element of R's [B, ldr] image
__global__ __launch_bounds__(256) void proj_interact_fwd_generic_kernel(long long B, int D, int I1, int I2, const float* __restrict__ x,
                                                                        long long x_ld, const float* __restrict__ P1, long long p1_ld,
                                                                        const float* __restrict__ P2, long long p2_ld, float* __restrict__ R,
                                                                        long long ldr) {
    const long long total = B * ldr, W = (long long)D + (long long)I1 * I2;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long b = e / ldr, c = e - b * ldr;
        float v = 0.f;
        if (c < D) {
            v = x[b * x_ld + c];
        } else if (c < W) {
            const int i = (int)((c - D) / I2), j = (int)((c - D) - (long long)i * I2);
            const float* a = P1 + b * p1_ld + (long long)i * D;
            const float* bm = P2 + b * p2_ld + j;
            for (int d = 0; d < D; ++d) v = fmaf(a[d], bm[(long long)d * I2], v);
        }
        R[e] = v;
    }
}

// generic backward: one thread per element of [dx | dP1 | dP2] of a sample
__global__ __launch_bounds__(256) void proj_interact_bwd_generic_kernel(long long B, int D, int I1, int I2, const float* __restrict__ P1,
                                                                        long long p1_ld, const float* __restrict__ P2, long long p2_ld,
                                                                        const float* __restrict__ dR, long long ldr, float* __restrict__ dx,
                                                                        long long dx_ld, float* __restrict__ dP1, long long dp1_ld,
                                                                        float* __restrict__ dP2, long long dp2_ld) {
    const long long n1 = (long long)I1 * D, n2 = (long long)D * I2, per = D + n1 + n2, total = B * per;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long b = e / per;
        long long c = e - b * per;
        const float* dZ = dR + b * ldr + D;
        if (c < D) {
            dx[b * dx_ld + c] = dR[b * ldr + c];
        } else if ((c -= D) < n1) {
            const int i = (int)(c / D), d = (int)(c - (long long)i * D);
            const float* bm = P2 + b * p2_ld + (long long)d * I2;
            float v = 0.f;
            for (int j = 0; j < I2; ++j) v = fmaf(dZ[(long long)i * I2 + j], bm[j], v);
            dP1[b * dp1_ld + c] = v;
        } else {
            c -= n1;
            const int d = (int)(c / I2), j = (int)(c - (long long)d * I2);
            const float* a = P1 + b * p1_ld + d;
            float v = 0.f;
            for (int i = 0; i < I1; ++i) v = fmaf(a[(long long)i * D], dZ[(long long)i * I2 + j], v);
            dP2[b * dp2_ld + c] = v;
        }
    }
}

inline bool proj_ld4(int64_t ld) { return (ld & 3) == 0; }

inline unsigned proj_grid(long long n) { return (unsigned)(n < (long long)PROJ_MAX_GRID ? n : (long long)PROJ_MAX_GRID); }

}  // namespace

extern "C" int dlrm_proj_interact_fwd(int64_t B, int D, int I1, int I2, const float* x, int64_t x_ld, const float* P1, int64_t p1_ld,
                                      const float* P2, int64_t p2_ld, float* R, int64_t ldr, void* stream) {
    DLRM_REQUIRE(B >= 0 && D >= 1 && I1 >= 1 && I2 >= 1, DLRM_E_ARG, "B < 0 or D, I1, I2 < 1");
    const int64_t n1 = (int64_t)I1 * D, n2 = (int64_t)D * I2, W = (int64_t)D + (int64_t)I1 * I2;
    DLRM_REQUIRE(x_ld >= D && p1_ld >= n1 && p2_ld >= n2 && ldr >= W, DLRM_E_ARG, "a leading dimension is smaller than its row");
    if (B == 0) return 0;
    DLRM_REQUIRE(x && P1 && P2 && R, DLRM_E_ARG, "null operand");
    hipStream_t st = (hipStream_t)stream;
    const int64_t lds = ((int64_t)I1 * (D + 4) + n2) * 4;
    const bool fast = (D & 3) == 0 && I1 <= PROJ_MAX_I && I2 <= PROJ_MAX_I && lds <= PROJ_MAX_LDS && dlrm_aligned16(x) && dlrm_aligned16(P1) &&
                      dlrm_aligned16(P2) && dlrm_aligned16(R) && proj_ld4(x_ld) && proj_ld4(p1_ld) && proj_ld4(p2_ld) && proj_ld4(ldr);
    if (fast) {
        hipLaunchKernelGGL(proj_interact_fwd_kernel, dim3(proj_grid(B)), dim3(DLRM_WAVE), (size_t)lds, st, (long long)B, D, I1, I2, x,
                           (long long)x_ld, P1, (long long)p1_ld, P2, (long long)p2_ld, R, (long long)ldr);
    } else {
        hipLaunchKernelGGL(proj_interact_fwd_generic_kernel, dim3(proj_grid((B * ldr + 255) / 256)), dim3(256), 0, st, (long long)B, D, I1, I2, x,
                           (long long)x_ld, P1, (long long)p1_ld, P2, (long long)p2_ld, R, (long long)ldr);
    }
    DLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int dlrm_proj_interact_bwd(int64_t B, int D, int I1, int I2, const float* P1, int64_t p1_ld, const float* P2, int64_t p2_ld,
                                      const float* dR, int64_t ldr, float* dx, int64_t dx_ld, float* dP1, int64_t dp1_ld, float* dP2,
                                      int64_t dp2_ld, void* stream) {
    DLRM_REQUIRE(B >= 0 && D >= 1 && I1 >= 1 && I2 >= 1, DLRM_E_ARG, "B < 0 or D, I1, I2 < 1");
    const int64_t n1 = (int64_t)I1 * D, n2 = (int64_t)D * I2, W = (int64_t)D + (int64_t)I1 * I2;
    DLRM_REQUIRE(p1_ld >= n1 && p2_ld >= n2 && ldr >= W && dx_ld >= D && dp1_ld >= n1 && dp2_ld >= n2, DLRM_E_ARG,
                 "a leading dimension is smaller than its row");
    if (B == 0) return 0;
    DLRM_REQUIRE(P1 && P2 && dR && dx && dP1 && dP2, DLRM_E_ARG, "null operand");
    hipStream_t st = (hipStream_t)stream;
    const int64_t lds = ((int64_t)I1 * (D + 4) + n2 + (int64_t)I1 * (I2 + 1)) * 4;
    const bool fast = (D & 3) == 0 && I1 <= PROJ_MAX_I && I2 <= PROJ_MAX_I && lds <= PROJ_MAX_LDS && dlrm_aligned16(P1) && dlrm_aligned16(P2) &&
                      dlrm_aligned16(dR) && dlrm_aligned16(dx) && dlrm_aligned16(dP1) && dlrm_aligned16(dP2) && proj_ld4(p1_ld) &&
                      proj_ld4(p2_ld) && proj_ld4(ldr) && proj_ld4(dx_ld) && proj_ld4(dp1_ld) && proj_ld4(dp2_ld);
    if (fast) {
        hipLaunchKernelGGL(proj_interact_bwd_kernel, dim3(proj_grid(B)), dim3(DLRM_WAVE), (size_t)lds, st, (long long)B, D, I1, I2, P1,
                           (long long)p1_ld, P2, (long long)p2_ld, dR, (long long)ldr, dx, (long long)dx_ld, dP1, (long long)dp1_ld, dP2,
                           (long long)dp2_ld);
    } else {
        const int64_t per = (int64_t)D + n1 + n2;
        hipLaunchKernelGGL(proj_interact_bwd_generic_kernel, dim3(proj_grid((B * per + 255) / 256)), dim3(256), 0, st, (long long)B, D, I1, I2,
                           P1, (long long)p1_ld, P2, (long long)p2_ld, dR, (long long)ldr, dx, (long long)dx_ld, dP1, (long long)dp1_ld, dP2,
                           (long long)dp2_ld);
    }
    DLRM_LAUNCH_CHECK();
    return 0;
}
