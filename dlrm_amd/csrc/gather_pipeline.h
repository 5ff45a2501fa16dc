// gather_pipeline.h — the D = 128 fused lookup + pairwise-dot interaction kernels, forward and backward, over a ROW SOURCE, gfx950.
//
// The kernels widen / dequantise / compose the table rows of a sample into the wave-private swizzled fp32 LDS image of
//   interact_{fwd,bwd}_dma_kernel (interact.hip: 16-byte slot q of row r holds quad q ^ (r & 15); row 0 is x, rows F.. are zero) and run
//   those kernels' fragment-read / MFMA / store sections on it unchanged (the forward's MFMA section IS theirs: tile_fwd_mfma of
//   interact_tiles.h), so the products have the summation order of every D = 128 interaction kernel.  What a table kind is — bf16
//   (interact_bf16.hip), row-wise quantised (interact_quant.hip), quotient-remainder (interact_qr.hip) — is the source type S; everything
//   here is the same for all of them.
//
// Pipeline (per wave, four waves per workgroup = one per SIMD, no barrier in the sample loop, two images per wave): at the top of sample
//   n the rows (and x, and the dR row) of sample n + 1 are issued into registers from selectors that were loaded during sample n - 1, then
//   the selectors of sample n + 2 are issued; sample n is multiplied from image[cur]; only then are the registers converted and written
//   into image[cur ^ 1] and the selectors checked.  Look-ahead past the last sample is clamped to B - 1.  Every memory operation is an
//   ordinary global load / store or LDS access that the compiler counts: no inline-asm loads, no LDS-DMA, no hand-placed waits.
//
// Three rules keep scratch at 0 and the loads in flight; each has been broken once:
//   * the wait for the next sample's rows (and for the selectors behind them) sits behind the multiplication and IN FRONT of this sample's
//     stores: vmcnt counts stores too, and a wait placed behind them would wait for their acknowledgement.  So image_write and the
//     selector check come first, the stores last, and they drain beside the next sample's loads and MFMAs;
//   * the x quad of lanes >= 32 is an assignment under `if`, not a ?: between a load and a zero constant: that selects between two
//     ADDRESSES and keeps the constant in scratch;
//   * the kernarg pointer tables are copied to LDS with compile-time kernarg offsets (S::args_to_lds): a lane-indexed read of a by-value
//     struct would go to scratch.  For the same reason nothing of S::Args is ever indexed by lane.
//   The only flat_* instructions are the volatile stores of the error report.
//
// The source type S, all members static, __device__ __forceinline__ and resolved at compile time:
//   Args                       the kernarg struct: the table list, `err`, `pred`, and whatever runtime value the source needs
//   NTAB                       8-byte LDS table words per feature slot (GC_MAXF slots each)
//   passes(NB)                 row-fetch passes per sample
//   Lane<NP>                   what a lane keeps across the sample loop; has own, qsrc, osrc, rows for sel_load (gather_common.h)
//   Row, Regs<NP>              the selector the owner lane hands to the lanes of a row; the rows of one sample as loaded
//   args_to_lds(a, tab, F)     the kernarg tables into LDS
//   lane_init(bl, tab, F, lane)
//   sel_resolve<IT>(bl, sel, s, lane, err, live) -> Row     the owner lane's checks; !live (look-ahead past the end): the zero row, no report
//   rows_issue(v, bl, row, lane)                            NP passes of loads into registers, nothing waits
//   image_write(img, v, bl, xv, lane, a)                    convert and write the image (row 0 = xv)
//   DUP, dst_slot(a, tab, i, F, dup) -> slot               backward: feature i's gradient row goes to columns slot * D .. of dE, and, if
//                                                           DUP and dup comes back set, a second time D columns further
#pragma once
#include "gather_common.h"

namespace {

constexpr int BI_D = 128;
constexpr int BI_ROWB = BI_D * 4;           // bytes of an image row
constexpr int BI_DRB = 2048;                // dR row image of the backward (as the fp32 gather backward); its last word stays zero

// -------------------------------------------------------------------------------------------
// forward
// -------------------------------------------------------------------------------------------
template <typename S, int NB, typename IT>          // NB = 16-row tiles of the image: 1 (F <= 16) or 2
__global__ __launch_bounds__(256) void gather_fwd_kernel(typename S::Args ba, const float* __restrict__ x, long long x_ld, long long B,
                                                         int F, int self, float* __restrict__ R, long long ldr) {
    if (ba.pred.skip()) return;                              // (the two-kernel form runs instead)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NP = S::passes(NB);
    constexpr int IMGB = 16 * NB * BI_ROWB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6));
    long long* tab = (long long*)lds;
    char* img0 = (char*)(tab + S::NTAB * GC_MAXF) + (size_t)wave * 2 * IMGB;

    S::args_to_lds(ba, tab, F);
    for (int e = lane; e < 2 * IMGB / 16; e += 64) ((float4*)img0)[e] = make_float4(0.f, 0.f, 0.f, 0.f);      // rows F.. stay zero
    __syncthreads();

    const long long b_stride = (long long)gridDim.x * W;
    long long b = (long long)blockIdx.x * W + wave;
    if (b >= B) return;

    const int g = lane >> 4, li = lane & 15;
    typename S::template Lane<NP> bl;
    S::template lane_init<NP>(bl, tab, F, lane);

    const int P = (self & 1) ? F * (F + 1) / 2 : F * (F - 1) / 2;
    // where this lane's four results of tile pair (r, c) go inside the R row (float index; -1 = not part of the output):
    // output row i = 16 r + 4 g + q, column j = 16 c + li — a function of the lane only, computed once
    int opos[NB * (NB + 1) / 2][4];
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = 16 * r + 4 * g + q, j = 16 * c + li;
                const bool ok = i < F && ((self & 1) ? (j <= i) : (j < i));
                opos[r * (r + 1) / 2 + c][q] = ok ? BI_D + pair_pos(i, j, F, self) : -1;
            }
    constexpr int NPAIR = NB * (NB + 1) / 2;
    const long long last = B - 1;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // prologue: the first sample's image, and the second sample's (checked) selectors
    typename S::Row idun;
    {
        const typename S::Row idu = S::template sel_resolve<IT, NP>(bl, sel_load<IT>(bl, b), b, lane, ba.err, true);
        typename S::template Regs<NP> v;
        S::template rows_issue<NP>(v, bl, idu, lane);
        float4 xv = zero4;
        if (lane < 32) xv = *(const float4*)(x + b * x_ld + 4 * lane);
        const long long s1 = b + b_stride;
        const Sel<IT> sel1 = sel_load<IT>(bl, s1 < B ? s1 : last);
        S::template image_write<NP>(img0, v, bl, xv, lane, ba);
        idun = S::template sel_resolve<IT, NP>(bl, sel1, s1, lane, ba.err, s1 < B);
    }
    int cur = 0;
    for (; b < B; b += b_stride) {
        // the next sample (clamped past the end: its image is written and never multiplied): rows out now from the selectors that were
        // loaded and checked one sample ago, then the selectors two samples ahead
        const long long s1 = b + b_stride, s2 = s1 + b_stride;
        typename S::template Regs<NP> vn;
        S::template rows_issue<NP>(vn, bl, idun, lane);
        float4 xn = zero4;
        if (lane < 32) xn = *(const float4*)(x + (s1 < B ? s1 : last) * x_ld + 4 * lane);
        const Sel<IT> seln = sel_load<IT>(bl, s2 < B ? s2 : last);

        const char* my = img0 + cur * IMGB;
        // ---- the fragment reads of interact_fwd_dma_kernel (interact.hip), then the MFMA section both share ----
        float4 fr[NB][BI_D / 16];
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int s = 0; s < BI_D / 16; ++s)
                fr[r][s] = *(const float4*)(my + (16 * r + li) * BI_ROWB + (((4 * s + g) ^ li) * 16));      // (row & 15) == li
        const float4 xrow = *(const float4*)(my + (lane & 31) * 16);
        __builtin_amdgcn_sched_barrier(0);      // all fragment reads (and the next sample's loads) in front of the first MFMA
        floatx4 acc[NPAIR][2];
        tile_fwd_mfma<NB, BI_D / 16>(acc, fr);      // interact_tiles.h: the summation order of every one of these kernels

        // only now are the next sample's registers touched (the first rule of the header)
        S::template image_write<NP>(img0 + (cur ^ 1) * IMGB, vn, bl, xn, lane, ba);
        idun = S::template sel_resolve<IT, NP>(bl, seln, s2, lane, ba.err, s2 < B);

        // ---- the store section of interact_fwd_dma_kernel ----
        float* Rb = R + b * ldr;
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) {
            const floatx4 sum = acc[p][0] + acc[p][1];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (opos[p][q] >= 0) Rb[opos[p][q]] = sum[q];
        }
        // R[:, 0:D] = x (row 0 of the image, un-swizzled: row & 15 == 0), then the alignment padding
        if (lane < 32) *(float4*)(Rb + 4 * lane) = xrow;
        for (long long d = BI_D + P + lane; d < ldr; d += 64) Rb[d] = 0.f;
        cur ^= 1;
    }
}

// -------------------------------------------------------------------------------------------
// backward: dT = (dZ + dZ^T) . T per sample (interact_bwd_dma_kernel, non-UPD), T rebuilt from the table rows
// -------------------------------------------------------------------------------------------
template <typename S, int NB, typename IT>
__global__ __launch_bounds__(256) void gather_bwd_kernel(typename S::Args ba, const float* __restrict__ x, long long x_ld, long long B,
                                                         int F, int self, const float* __restrict__ dR, long long ldr,
                                                         float* __restrict__ dx, long long dx_ld, float* __restrict__ dE, long long dE_ld) {
    if (ba.pred.skip()) return;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NP = S::passes(NB);
    constexpr int IMGB = 16 * NB * BI_ROWB;
    constexpr int DRB = BI_DRB;
    constexpr int NDR = DRB / 1024;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    long long* tab = (long long*)lds;
    char* img0 = (char*)(tab + S::NTAB * GC_MAXF) + (size_t)wave * (2 * IMGB + 2 * DRB);
    char* drow0 = img0 + 2 * IMGB;

    S::args_to_lds(ba, tab, F);
    for (int e = lane; e < (2 * IMGB + 2 * DRB) / 16; e += 64) ((float4*)img0)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();

    const long long b_stride = (long long)gridDim.x * 4;
    long long b = (long long)blockIdx.x * 4 + wave;
    if (b >= B) return;

    const int g = lane >> 4, li = lane & 15;
    typename S::template Lane<NP> bl;
    S::template lane_init<NP>(bl, tab, F, lane);
    const long long rowb = ldr * 4;                      // bytes of a dR row (the entry point requires rowb < DRB)

    // A-fragment sources inside the dR row (float index; structural zeros read the image's LAST word: the row never reaches it and it was
    // zeroed with the images), doubled on the diagonal when self pairs exist — computed once per lane
    int a_off[NB][4 * NB];
    float a_scale[NB][4 * NB];
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int kk = 0; kk < 4 * NB; ++kk) {
            const int i = 16 * r + li, j = 4 * kk + g;
            int off = DRB / 4 - 1; float sc = 1.f;
            if (i < F && j < F) {
                if (i == j) { if (self & 1) { off = BI_D + pair_pos(i, i, F, self); sc = 2.f; } }
                else {
                    const int hi = i > j ? i : j, lo = i > j ? j : i;
                    off = BI_D + pair_pos(hi, lo, F, self);
                }
            }
            a_off[r][kk] = off * 4; a_scale[r][kk] = sc;
        }
    // destination rows of this lane: i = 16 r + 4 g + q — feature 0 is dx, feature f >= 1 the columns of S::dst_slot in dE (dupbits: and a
    // second time D columns further).  GLOBAL pointers.
    gchar* orow[NB][4];
    long long ostep[NB][4];
    unsigned rowbits = 0u, dupbits = 0u;
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 16 * r + 4 * g + q;
            if (i < F) rowbits |= 1u << (4 * r + q);
            bool dup = false;
            const long long slot = S::dst_slot(ba, tab, i, F, dup);
            if (dup) dupbits |= 1u << (4 * r + q);
            const long long ld = i == 0 ? dx_ld : dE_ld;
            float* base = i == 0 ? dx : dE + slot * BI_D;
            orow[r][q] = (i < F) ? (gchar*)(base + b * ld + 4 * li) : nullptr;
            ostep[r][q] = b_stride * ld * 4;
        }

    const long long last = B - 1;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // prologue: the first sample's images, and the second sample's (checked) selectors
    typename S::Row idun;
    {
        const typename S::Row idu = S::template sel_resolve<IT, NP>(bl, sel_load<IT>(bl, b), b, lane, ba.err, true);
        typename S::template Regs<NP> v;
        S::template rows_issue<NP>(v, bl, idu, lane);
        float4 xv = zero4;
        if (lane < 32) xv = *(const float4*)(x + b * x_ld + 4 * lane);
        const DrRegs<NDR> d = dr_load<NDR>(dR + b * ldr, rowb, lane);
        const long long s1 = b + b_stride;
        const Sel<IT> sel1 = sel_load<IT>(bl, s1 < B ? s1 : last);
        S::template image_write<NP>(img0, v, bl, xv, lane, ba);
        dr_write<NDR>(drow0, d, rowb, lane);
        idun = S::template sel_resolve<IT, NP>(bl, sel1, s1, lane, ba.err, s1 < B);
    }
    int cur = 0;
    for (; b < B; b += b_stride) {
        // the next sample (clamped past the end): rows, x and the dR row out now, then the selectors two samples ahead
        const long long s1 = b + b_stride, s2 = s1 + b_stride;
        const long long n1 = s1 < B ? s1 : last;
        typename S::template Regs<NP> vn;
        S::template rows_issue<NP>(vn, bl, idun, lane);
        float4 xn = zero4;
        if (lane < 32) xn = *(const float4*)(x + n1 * x_ld + 4 * lane);
        const DrRegs<NDR> dn = dr_load<NDR>(dR + n1 * ldr, rowb, lane);
        const Sel<IT> seln = sel_load<IT>(bl, s2 < B ? s2 : last);

        const char* my = img0 + cur * IMGB;
        const char* dr = drow0 + cur * DRB;
        // ---- the A-fragment / B-fragment / MFMA / store section of interact_bwd_dma_kernel (interact.hip, non-UPD) ----
        float aS[NB][4 * NB];
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int kk = 0; kk < 4 * NB; ++kk) {
                const float v = *(const float*)(dr + a_off[r][kk]);
                aS[r][kk] = a_scale[r][kk] * v;
            }
        __builtin_amdgcn_sched_barrier(0);      // the next sample's loads stay in front of the multiplication
#pragma unroll
        for (int dq = 0; dq < BI_D / 64; ++dq) {
            float4 bT[4 * NB];
#pragma unroll
            for (int kk = 0; kk < 4 * NB; ++kk) {
                const int jr = 4 * kk + g;                 // rows >= F of the image are zero
                bT[kk] = *(const float4*)(my + jr * BI_ROWB + (((16 * dq + li) ^ (jr & 15)) * 16));
            }
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                // feature 0's two extra operands (the x part of dR; x itself for the ReLU derivative), read by every lane in front of the MFMAs
                float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), y0 = x0;
                if (r == 0) {
                    x0 = *(const float4*)(dr + (64 * dq + 4 * li) * 4);
                    y0 = *(const float4*)(my + (16 * dq + li) * 16);
                }
                floatx4 acc[4];
#pragma unroll
                for (int s_ = 0; s_ < 4; ++s_) acc[s_] = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 4 * NB; ++kk) {
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(aS[r][kk], bT[kk].x, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aS[r][kk], bT[kk].y, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(aS[r][kk], bT[kk].z, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(aS[r][kk], bT[kk].w, acc[3], 0, 0, 0);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if ((rowbits >> (4 * r + q)) & 1u) {
                        float4 v = make_float4(acc[0][q], acc[1][q], acc[2][q], acc[3][q]);
                        if (r == 0 && q == 0 && g == 0) {       // feature 0 also feeds R[:, 0:D]
                            v.x += x0.x; v.y += x0.y; v.z += x0.z; v.w += x0.w;
                            if (self & 4) {                     // feature 0 is a ReLU output: its derivative is applied here (image row 0 = x)
                                v.x = y0.x > 0.f ? v.x : 0.f; v.y = y0.y > 0.f ? v.y : 0.f;
                                v.z = y0.z > 0.f ? v.z : 0.f; v.w = y0.w > 0.f ? v.w : 0.f;
                            }
                        }
                        *(gfloatx4*)(orow[r][q] + dq * 256) = (floatx4){v.x, v.y, v.z, v.w};
                        if constexpr (S::DUP)
                            if ((dupbits >> (4 * r + q)) & 1u) *(gfloatx4*)(orow[r][q] + dq * 256 + BI_ROWB) = (floatx4){v.x, v.y, v.z, v.w};
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) if ((rowbits >> (4 * r + q)) & 1u) orow[r][q] += ostep[r][q];

        // only now are the next sample's registers touched (the first rule of the header)
        S::template image_write<NP>(img0 + (cur ^ 1) * IMGB, vn, bl, xn, lane, ba);
        dr_write<NDR>(drow0 + (cur ^ 1) * DRB, dn, rowb, lane);
        idun = S::template sel_resolve<IT, NP>(bl, seln, s2, lane, ba.err, s2 < B);
        cur ^= 1;
    }
}

// dynamic LDS of a workgroup: the tables, then per wave two images (and two dR rows)
template <typename S>
static inline size_t gather_lds(int nb, bool bwd) {
    return S::NTAB * GC_MAXF * sizeof(long long) + (size_t)GC_WAVES * (2 * (size_t)(16 * nb * BI_ROWB) + (bwd ? 2 * (size_t)BI_DRB : 0));
}

template <typename S, int NB, typename IT>
void launch_fwd(const typename S::Args& ba, const float* x, long long x_ld, long long B, int F, int self, float* R, long long ldr, hipStream_t st) {
    const size_t lds = gather_lds<S>(NB, false);
    dlrm_lds_limit<gather_fwd_kernel<S, NB, IT>>(lds);
    hipLaunchKernelGGL((gather_fwd_kernel<S, NB, IT>), dim3((unsigned)gather_grid(B, lds)), dim3(64 * GC_WAVES), lds, st, ba, x, x_ld, B, F,
                       self, R, ldr);
}

template <typename S, int NB, typename IT>
void launch_bwd(const typename S::Args& ba, const float* x, long long x_ld, long long B, int F, int self, const float* dR, long long ldr, float* dx,
                long long dx_ld, float* dE, long long dE_ld, hipStream_t st) {
    const size_t lds = gather_lds<S>(NB, true);
    dlrm_lds_limit<gather_bwd_kernel<S, NB, IT>>(lds);
    hipLaunchKernelGGL((gather_bwd_kernel<S, NB, IT>), dim3((unsigned)gather_grid(B, lds)), dim3(64 * GC_WAVES), lds, st, ba, x, x_ld, B, F,
                       self, dR, ldr, dx, dx_ld, dE, dE_ld);
}

// the instantiation of a call: NB from F, the id type from idx_bits
template <typename S>
void gather_fwd(const typename S::Args& ba, const float* x, long long x_ld, long long B, int F, int self, float* R, long long ldr, int idx_bits,
                hipStream_t st) {
    if (F <= 16) {
        if (idx_bits == 64) launch_fwd<S, 1, long long>(ba, x, x_ld, B, F, self, R, ldr, st);
        else                launch_fwd<S, 1, int>(ba, x, x_ld, B, F, self, R, ldr, st);
    } else {
        if (idx_bits == 64) launch_fwd<S, 2, long long>(ba, x, x_ld, B, F, self, R, ldr, st);
        else                launch_fwd<S, 2, int>(ba, x, x_ld, B, F, self, R, ldr, st);
    }
}

template <typename S>
void gather_bwd(const typename S::Args& ba, const float* x, long long x_ld, long long B, int F, int self, const float* dR, long long ldr, float* dx,
                long long dx_ld, float* dE, long long dE_ld, int idx_bits, hipStream_t st) {
    if (F <= 16) {
        if (idx_bits == 64) launch_bwd<S, 1, long long>(ba, x, x_ld, B, F, self, dR, ldr, dx, dx_ld, dE, dE_ld, st);
        else                launch_bwd<S, 1, int>(ba, x, x_ld, B, F, self, dR, ldr, dx, dx_ld, dE, dE_ld, st);
    } else {
        if (idx_bits == 64) launch_bwd<S, 2, long long>(ba, x, x_ld, B, F, self, dR, ldr, dx, dx_ld, dE, dE_ld, st);
        else                launch_bwd<S, 2, int>(ba, x, x_ld, B, F, self, dR, ldr, dx, dx_ld, dE, dE_ld, st);
    }
}

}  // namespace
