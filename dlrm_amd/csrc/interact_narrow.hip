// interact_narrow.hip — fused lookup + pairwise-dot interaction, forward AND backward, over fp32 tables of D = 16 / 32 / 64, gfx950.
//
// Replaces, for batches with ONE lookup per bag and no per-sample weights: dlrm_emb_fwd + dlrm_interact_fwd (forward) and dlrm_interact_bwd
//   over the pooled [B, T*D] buffer (backward) at the widths where those are the GENERIC interaction kernels (interact.hip:
//   interact_fwd_kernel / interact_bwd_kernel<NB>), which stage a sample through registers in dependent load -> ds_write rounds between two
//   workgroup barriers.  The pooled buffer is neither written nor read; the backward fetches the rows again.
//
// Contract (include/dlrm_hip.h):
//   forward : R is BIT-IDENTICAL to dlrm_emb_fwd (psw_host = NULL) into a feature buffer + dlrm_interact_fwd, modes 0 / 1 / 2;
//   backward: dx, dE are BIT-IDENTICAL to dlrm_interact_bwd over (x, that buffer); dE[b, t*D : (t+1)*D] is the gradient row of table t.
//   * element = fmaf(1.0f, W[id], +0.0f) — the lookup's arithmetic from a zero accumulator (emb.hip), so -0.0 becomes +0.0; an
//     out-of-range id gives a row of +0.0 and is reported; its gradient row is written like any other;
//   * forward products = the generic kernel's: v_mfma_f32_16x16x4_f32, lane group g = lane >> 4 supplies columns 16 s + 4 g .. + 3 of
//     step s, components x, y, z, w go to acc0, acc1, acc0, acc1 for s = 0 .. D/16 - 1, result acc0 + acc1;
//   * backward products = the generic kernel's: S = dZ + dZ^T (diagonal 2 dR with self pairs), k = feature 4 kk + g for kk = 0 .. 4 NB - 1
//     (the zero features up to 16 NB are multiplied too: 0 * 0 added to -0.0 gives +0.0), even kk to acc0, odd kk to acc1, result
//     acc0 + acc1; feature 0 adds dR[:, d] and takes the DLRM_INTERACT_RELU_X mask as `!(x > 0) -> 0`.
//   Every output element is its own chain of MFMA partial sums, so WHICH lane holds a column is free: the backward gives a lane the D/16
//   adjacent columns (D/16) li .. of every row it owns, one store of 4 / 8 / 16 bytes instead of D/16 four-byte stores.
//
// Row fetch: a row of D floats is 4 D bytes; a lane owns 4 columns = ONE 16-byte load, D/4 lanes cover a row, a wave fetches 256/D rows per
//   pass, ceil((16 NB - 1) / (256/D)) passes per sample.  Lane f (1 <= f < F) owns feature f's selector: it loads idx[f][s] and off[f][s],
//   checks them and hands the row number to the D/4 lanes of that row by lane shuffle.  Feature 0 (x) is one float4 load in lanes 0 .. D/4-1;
//   the backward's dR row (D + P floats, at most 592) is at most three 16-byte loads per lane.
//
// LDS image of a sample: [16 NB rows][D + 4 floats] (the generic forward's row pitch: b128 fragment reads of 16 rows are conflict free); rows
//   F.. are zeroed once and never written.
//
// Pipeline (per wave, four waves per workgroup, no barrier in the sample loop, two images per wave): at the top of sample n the rows (and x,
//   and the dR row) of sample n + 1 are issued into registers from selectors that were loaded during sample n - 1, then the selectors of
//   sample n + 2 are issued; sample n is multiplied from image[cur]; only then are the registers written into image[cur ^ 1] and the
//   selectors checked.  Look-ahead past the last sample is clamped to B - 1.  Every memory operation is an ordinary global load / store or
//   LDS access that the compiler counts: no inline-asm loads, no LDS-DMA, no hand-placed waits.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no static LDS, the dynamic LDS of a workgroup is what
//   narrow_lds() returns): the table below.  Scratch is 0 everywhere: the kernarg pointer tables are copied to LDS with
//   compile-time kernarg offsets, and optional loads are assignments under `if`, never a ?: between a load and a constant.
//                                                    VGPRs (int / long long ids)  AGPRs  SGPRs  scratch  dynamic LDS
//   interact_fwd_narrow_kernel<F32Rows, 16, 1, IT>       58 /  58                  8     90      0      11264 B
//   interact_fwd_narrow_kernel<F32Rows, 16, 2, IT>       86 /  86                 24     90      0      21504 B
//   interact_fwd_narrow_kernel<F32Rows, 32, 1, IT>       68 /  68                  8     90      0      19456 B
//   interact_fwd_narrow_kernel<F32Rows, 32, 2, IT>      102 / 106                 24     90      0      37888 B
//   interact_fwd_narrow_kernel<F32Rows, 64, 1, IT>       86 /  90                  8     90      0      35840 B
//   interact_fwd_narrow_kernel<F32Rows, 64, 2, IT>      142 / 150                 24     90      0      70656 B
//   interact_bwd_narrow_kernel<F32Rows, 16, 1, IT>       78 /  79                  8     90      0      19456 B
//   interact_bwd_narrow_kernel<F32Rows, 16, 2, IT>      144 / 145                  8     90      0      46080 B
//   interact_bwd_narrow_kernel<F32Rows, 32, 1, IT>       96 /  96                 16     90      0      27648 B
//   interact_bwd_narrow_kernel<F32Rows, 32, 2, IT>      168 / 170                 16     92      0      62464 B
//   interact_bwd_narrow_kernel<F32Rows, 64, 1, IT>      126 / 126                 32     90      0      44032 B
//   interact_bwd_narrow_kernel<F32Rows, 64, 2, IT>      232 / 234                 32     92      0      95232 B   (one workgroup per CU)
//   The launch keeps at most two workgroups (eight waves) per CU, so neither registers (512 per lane at one wave per SIMD, 256 at two) nor
//   LDS limits any instantiation below what the grid asks for.
//   The kernels live in interact_narrow.h, templated over a row source; this file instantiates them for fp32 rows (F32Rows) and
//   interact_narrow_rows.hip for bfloat16 and packed rows, interact_narrow_qr.hip for quotient-remainder tables.  The table was re-taken
//   after that split and after the selector side (OneArraySide) became part of the source: the figures did not change.  After the split
//   the device assembly of the fp32 instantiations was instruction for instruction what the untemplated kernels compiled to; with the
//   selector side it has the same instruction count and differs in symbol names and in the order / register numbers of the moves and
//   stores of the error report (dlrm_report_bad_index).
#include "interact_narrow.h"

extern "C" int dlrm_interact_gather_narrow_ok(int F, int D) {
    return narrow_shape_ok(F, D) ? 1 : 0;
}

extern "C" int dlrm_interact_fwd_gather_narrow(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                               const void* const* weight_host, const int64_t* rows_host,
                                               const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                               int self_interaction, float* R, int64_t ldr, int64_t* err,
                                               const int32_t* pred_flag, int pred_nonzero, void* stream) {
    GatherArgs na;
    // a lane's 4 columns are one 16-byte load; rows are 4 D bytes apart
    const int rc = gather_check_fwd(B, F, D, x, x_ld, weight_host && rows_host && index_host && offsets_host, idx_bits,
                                    dlrm_interact_gather_narrow_ok(F, D), self_interaction, R, ldr, [&] {
        return fill_args(na, F, weight_host, rows_host, index_host, offsets_host, err, pred_flag, pred_nonzero, 15u);
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 3;
    NARROW_DISPATCH(launch_fwd, F32Rows, na, x, (long long)x_ld, (long long)B, F, self, R, (long long)ldr, st);
    DLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int dlrm_interact_bwd_gather_narrow(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                               const void* const* weight_host, const int64_t* rows_host,
                                               const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                               int self_interaction, const float* dR, int64_t ldr,
                                               float* dx, int64_t dx_ld, float* dE, int64_t dE_ld, int64_t* err,
                                               const int32_t* pred_flag, int pred_nonzero, void* stream) {
    GatherArgs na;
    const int rc = gather_check_bwd(B, F, D, x, x_ld, weight_host && rows_host && index_host && offsets_host && dE, idx_bits,
                                    dlrm_interact_gather_narrow_ok(F, D), self_interaction, dR, ldr, dx, dx_ld, dE, dE_ld,
                                    (int64_t)(F - 1) * D, 0, [&] {
        return fill_args(na, F, weight_host, rows_host, index_host, offsets_host, err, pred_flag, pred_nonzero, 15u);
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 7;
    NARROW_DISPATCH(launch_bwd, F32Rows, na, x, (long long)x_ld, (long long)B, F, self, dR, (long long)ldr, dx, (long long)dx_ld, dE, (long long)dE_ld, st);
    DLRM_LAUNCH_CHECK();
    return 0;
}
