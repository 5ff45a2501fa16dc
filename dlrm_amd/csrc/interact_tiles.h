// interact_tiles.h — what the pairwise-dot interaction kernels that work on a per-wave LDS image share, gfx950: the D = 128 kernels of
// interact.hip (interact_fwd_dma_kernel) and the fused lookup + interaction kernels of gather_pipeline.h (D = 128) call tile_fwd_mfma; the
// kernels of interact_narrow.h (D = 16 / 32 / 64) take pair_pos and the typedefs from here and keep a copy of the loop (with the helper the
// compiler lays 20 of them out differently: profiles/fused_pipeline/resources.md).  Every contract between those kernels is BIT IDENTITY,
// which holds because the order in which the products of a pair are summed is written once, here.  The helper knows nothing of who calls it:
// how the image got into LDS, its row pitch and swizzle, waits, scheduling fences and stores are the caller's.
#pragma once
#include "common.h"

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
// pointers that round-trip through LDS as integers lose their address space; tag them global so the loads / stores are global_* (not
// flat_*, which also count on lgkmcnt — every LDS wait then waits for them)
typedef __attribute__((address_space(1))) char gchar;
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) floatx2 gfloatx2;
typedef __attribute__((address_space(1))) floatx4 gfloatx4;

// position of the pair (i, j), j <= i, in the flattened interaction output.  `mode` is a mode word: bit 0 = pairs include the
// diagonal (--arch-interaction-itself), bit 1 = torchrec order — torch.triu_indices(F, F, offset=1), i.e. pair (j, i) of the
// upper triangle enumerated row by row (torchrec InteractionArch) — instead of the reference's tril order (dlrm_s_pytorch.py:499-501).
__device__ __forceinline__ int pair_pos(int i, int j, int F, int mode) {
    if (mode & 2) return j * F - j * (j + 1) / 2 + (i - j - 1);
    return ((mode & 1) ? i * (i + 1) / 2 : i * (i - 1) / 2) + j;
}

// forward, Z = T . T^T over the lower-triangular tile pairs (r, c), c <= r, pair index r (r + 1) / 2 + c; NB = 16-row tiles of the image,
// NS = 16-column steps of a row (D / 16).  fr[r][s]: columns 16 s + 4 g .. + 3 (in whatever k order the image has, the same for every row)
// of image row 16 r + li.  The tile pairs advance together, one k-substep at a time: consecutive MFMAs are independent, the two accumulators
// of a pair (even / odd substeps, summed at the end — the summation order of every version of these kernels) are NPAIR issues apart
template <int NB, int NS>
__device__ __forceinline__ void tile_fwd_mfma(floatx4 (&acc)[NB * (NB + 1) / 2][2], const float4 (&fr)[NB][NS]) {
#pragma unroll
    for (int p = 0; p < NB * (NB + 1) / 2; ++p) { acc[p][0] = (floatx4){0.f, 0.f, 0.f, 0.f}; acc[p][1] = (floatx4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int r = 0; r < NB; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) {
                    const float av = e == 0 ? fr[r][s].x : e == 1 ? fr[r][s].y : e == 2 ? fr[r][s].z : fr[r][s].w;
                    const float bv = e == 0 ? fr[c][s].x : e == 1 ? fr[c][s].y : e == 2 ? fr[c][s].z : fr[c][s].w;
                    acc[r * (r + 1) / 2 + c][e & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[r * (r + 1) / 2 + c][e & 1], 0, 0, 0);
                }
        }
    }
}

}  // namespace
