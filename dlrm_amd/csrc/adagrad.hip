// adagrad.hip — K4: fused EmbeddingBag backward + row-wise sparse Adagrad, its exact (per-element) twin, and the dense Adagrad step.
//
// Reference replaced: autograd EmbeddingBagBackward (sparse COO gradient) followed by RWSAdagrad.step's sparse
// branch (optim/rwsadagrad.py:117-143): coalesce the gradient (duplicates of a row summed), then per touched row r
//     mom[r] += mean_d(g_r[d]^2);   W[r,:] -= clr * g_r / (sqrt(mom[r]) + eps)
// and its dense branch (:145-148) for the MLP parameters:  sum += g*g;  w -= clr * g / (sqrt(sum) + eps).
//
// The update is non-linear in g_r, so a row's complete gradient must exist before it is applied: the walk over (table, row)-sorted
// lookups of sorted_walk.h (pass 1 per lane group, edge buffers, pass 2 for runs that cross a group boundary), with the row updates below
// as its policy.  Every sum has a fixed order: results are run-to-run deterministic (hot rows are re-associated per 64 lookups
// relative to the reference's strictly sequential coalesce).
//
// EXACT = true (dlrm_emb_bwd_adagrad) is torch.optim.Adagrad's sparse branch (the reference's --optimizer=adagrad,
// dlrm_s_pytorch.py:1343-1369) over the same walk: the accumulator is torch's state["sum"], [rows, D], and per touched row, per column
//     sum[r,d] += g_r[d]^2;   W[r,d] -= clr * g_r[d] / (sqrt(sum[r,d]) + eps)
// Sort, groups, edge buffers and fix-up ownership are the row-wise kernels' (one template, a flag): g_r has the same bits in both.
#include <stdlib.h>
#include "sorted_walk.h"

namespace {

struct AdagradArgs {
    float* state[DLRM_MAX_TABLES_PER_LAUNCH];      // row-wise accumulator ("momentum") of each table, [rows]; EXACT: state["sum"], [rows, D]
};

__device__ __forceinline__ void v_step(float4& w, float nclr_over_denom, const float4& g) {
    w.x = __builtin_fmaf(nclr_over_denom, g.x, w.x); w.y = __builtin_fmaf(nclr_over_denom, g.y, w.y);
    w.z = __builtin_fmaf(nclr_over_denom, g.z, w.z); w.w = __builtin_fmaf(nclr_over_denom, g.w, w.w);
}

// EXACT: s = sum + g*g in two roundings (torch: state_sum.add_(grad.pow(2)), no fma), then the row-wise / dense kernels' form of the step.
// (hipcc's __fmul_rn / __fadd_rn are plain * and +, which -ffp-contract=fast fuses into one fma: the pragma is what keeps them apart)
__device__ __forceinline__ void v_exact_step(float& w, float& s, const float& g, float clr, float eps) {
    {
#pragma clang fp contract(off)
        const float gg = g * g;
        s = s + gg;
    }
    w = __builtin_fmaf(-clr, g / (sqrtf(s) + eps), w);
}
__device__ __forceinline__ void v_exact_step(float4& w, float4& s, const float4& g, float clr, float eps) {
    v_exact_step(w.x, s.x, g.x, clr, eps); v_exact_step(w.y, s.y, g.y, clr, eps);
    v_exact_step(w.z, s.z, g.z, clr, eps); v_exact_step(w.w, s.w, g.w, clr, eps);
}

// mom[row] += mean(g^2); W[row,:] = fma(-clr, g / (sqrt(mom[row]) + eps), W[row,:]).  Called by all LPB lanes of a
// lane group together (same control flow), `acc` = the lane's columns of the row's coalesced gradient.
// EXACT: mom_r is the row of the [rows, D] accumulator; a lane owns the same columns of W, sum and g (no cross-lane step) and requests
// all of its W and sum vectors before any arithmetic.
template <int VEC, int LPB, int NCH, bool EXACT>
__device__ __forceinline__ void adagrad_apply(float* __restrict__ wrow, float* __restrict__ mom_r, int D, int lig,
                                              const typename Vec<VEC>::T (&acc)[NCH], float clr, float eps) {
    using VT = typename Vec<VEC>::T;
    if constexpr (EXACT) {
        VT w[NCH], s[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int col = (c * LPB + lig) * VEC;
            if (col < D) { v_gload(w[c], wrow + col); v_gload(s[c], mom_r + col); }
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int col = (c * LPB + lig) * VEC;
            if (col < D) {
                v_exact_step(w[c], s[c], acc[c], clr, eps);
                v_gstore(wrow + col, w[c]);
                v_gstore(mom_r + col, s[c]);
            }
        }
        return;
    }
    const float sq = group_sum_sq<VEC, LPB, NCH>(acc, D, lig);
    // (row and accumulator through GLOBAL pointers: sorted_common.h v_gload — generic ones made these flat instructions)
    const float m = *(const sc_gfloat*)mom_r + sq / (float)D;              // every lane reads the old value before lane 0 stores the new one
    const float denom = sqrtf(m) + eps;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int col = (c * LPB + lig) * VEC;
        if (col < D) {
            VT w;
            v_gload(w, wrow + col);
            VT q;
            if constexpr (VEC == 4) q = make_float4(acc[c].x / denom, acc[c].y / denom, acc[c].z / denom, acc[c].w / denom);
            else q = acc[c] / denom;
            if constexpr (VEC == 4) v_step(w, -clr, q); else w = __builtin_fmaf(-clr, q, w);
            v_gstore(wrow + col, w);
        }
    }
    if (lig == 0) *(sc_gfloat*)mom_r = m;
}

// the walk's row-update policy: row-wise (EXACT = false) or per-element Adagrad on the fp32 row `row` of table t
template <bool EXACT>
struct AdagradRows {
    float clr, eps;
    template <int VEC, int LPB, int NCH>
    __device__ __forceinline__ void apply(float* w, float* state, int, long long row, int D, int lig, const typename Vec<VEC>::T (&acc)[NCH]) const {
        adagrad_apply<VEC, LPB, NCH, EXACT>(w + row * D, state + row * (EXACT ? D : 1), D, lig, acc, clr, eps);
    }
};

template <int VEC, int LPB, int NCH, typename KT, int kC, bool EXACT>
__global__ __launch_bounds__(256) void adagrad_groups_kernel(SortedArgs sa, AdagradArgs aa, long long L, int D, int row_bits,
                                                             const KT* __restrict__ keys, const unsigned* __restrict__ vals,
                                                             const unsigned* __restrict__ bag_of,
                                                             const float* __restrict__ dout, long long dout_ld,
                                                             DlrmStep clr_, float eps, float* __restrict__ edge_first,
                                                             float* __restrict__ edge_last) {
    const float clr = clr_;              // (by value, or read from the device scalar: common.h DlrmStep)
    WALK_STAGE_TABLES(sa, aa);
    walk_groups<VEC, LPB, NCH, KT, kC>(wt, L, D, row_bits, keys, vals, bag_of, dout, dout_ld, AdagradRows<EXACT>{clr, eps}, edge_first,
                                       edge_last);
}

template <int VEC, int LPB, int NCH, typename KT, bool EXACT>
__global__ __launch_bounds__(256) void adagrad_fixup_kernel(SortedArgs sa, AdagradArgs aa, long long L, int D, int row_bits,
                                                            const KT* __restrict__ keys, DlrmStep clr_, float eps,
                                                            const float* __restrict__ edge_first,
                                                            const float* __restrict__ edge_last) {
    const float clr = clr_;              // (by value, or read from the device scalar: common.h DlrmStep)
    walk_fixup<VEC, LPB, NCH, KT>(sa, aa.state, L, D, row_bits, keys, AdagradRows<EXACT>{clr, eps}, edge_first, edge_last);
}

// both passes of one launch group
template <bool EXACT, typename KT, int V, int LP, int NC>
static int launch_adagrad(const WalkLaunch<KT>& w, const WalkCall& c, void* const* state_host, DlrmStep clr, float eps) {
    AdagradArgs aa;
    for (int k = 0; k < DLRM_MAX_TABLES_PER_LAUNCH; ++k) aa.state[k] = (float*)state_host[w.g->t0 + (k < w.g->n ? k : 0)];
    // gradient rows in flight per lane group (tuning builds: env DLRM_ADAGRAD_KC = 1 | 2 | 4 | 8, default 2: sorted_walk.h has the figures);
    // the exact update is built for the default only
    static const int kc = DLRM_TUNE_ENV("DLRM_ADAGRAD_KC", 2);
#define ADA_GROUPS(KC)                                                                                                                   \
    hipLaunchKernelGGL((adagrad_groups_kernel<V, LP, NC, KT, KC, EXACT>), w.grid, w.block, 0, c.st, w.sa, aa, (long long)w.g->L, c.D, w.g->row_bits, \
                       w.keys, w.vals, w.bag_of, c.dout, (long long)c.dout_ld, clr, eps, w.edge_first, w.edge_last)
    if constexpr (EXACT) ADA_GROUPS(2);
    else if (kc == 1) ADA_GROUPS(1);
    else if (kc == 2) ADA_GROUPS(2);
    else if (kc == 8) ADA_GROUPS((LP >= 8 ? 8 : 4));
    else ADA_GROUPS(4);
#undef ADA_GROUPS
    DLRM_LAUNCH_CHECK();
    hipLaunchKernelGGL((adagrad_fixup_kernel<V, LP, NC, KT, EXACT>), w.grid, w.block, 0, c.st, w.sa, aa, (long long)w.g->L, c.D, w.g->row_bits, w.keys,
                       clr, eps, (const float*)w.edge_first, (const float*)w.edge_last);
    DLRM_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void adagrad_dense_kernel(long long n, float* __restrict__ w, float* __restrict__ sum,
                                                            const float* __restrict__ g, DlrmStep clr_, float eps) {
    const float clr = clr_;              // (by value, or read from the device scalar: common.h DlrmStep)
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float gi = g[i];
        const float s = __builtin_fmaf(gi, gi, sum[i]);          // addcmul_(grad, grad, value=1)
        sum[i] = s;
        w[i] = __builtin_fmaf(-clr, gi / (sqrtf(s) + eps), w[i]); // addcdiv_(grad, std, value=-clr)
    }
}

}  // namespace

extern "C" int64_t dlrm_emb_adagrad_workspace_bytes(int T, int D, const int64_t* nnz_host, const int64_t* rows_host) {
    return walk_workspace_bytes(T, D, nnz_host, rows_host);
}

namespace {

// both entry points: EXACT picks the accumulator layout and the apply step, `name` is the caller's symbol (messages)
template <bool EXACT>
static int emb_bwd_adagrad_any(const char* name, int T, int64_t B, int D, void* const* weight_host,
                               void* const* state_host, const int64_t* rows_host,
                               const void* const* indices_host, const void* const* offsets_host,
                               const int64_t* nnz_host, const void* const* psw_host, int idx_bits,
                               const float* dout, int64_t dout_ld, float lr, const float* lr_dev, float eps,
                               void* workspace, int64_t workspace_bytes, int64_t* err, void* stream) {
    if (T <= 0 || B <= 0 || D <= 0 || !weight_host || !state_host || !rows_host || !indices_host || !offsets_host || !nnz_host ||
        !dout || dout_ld < (int64_t)T * D)
        return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    hipStream_t st = (hipStream_t)stream;
    bool vec_ok = dlrm_aligned16(dout) && (dout_ld % 4 == 0);
    for (int t = 0; t < T; ++t) {
        if (!weight_host[t] || !state_host[t]) return DLRM_E_ARG;
        vec_ok = vec_ok && dlrm_aligned16(weight_host[t]);
        if (EXACT) vec_ok = vec_ok && dlrm_aligned16(state_host[t]);      // (a lane loads its columns of the [rows, D] accumulator as one vector)
    }
    const WalkCall c{T, B, D, weight_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, idx_bits, dout, dout_ld,
                     workspace, workspace_bytes, err, st};
    const DlrmStep clr = dlrm_step_pos(lr, lr_dev);
    return walk_update(name, c, vec_ok, [&](const auto& w, auto vec, auto lpb, auto nch) {
        using KT = typename std::decay_t<decltype(w)>::Key;
        return launch_adagrad<EXACT, KT, decltype(vec)::value, decltype(lpb)::value, decltype(nch)::value>(w, c, state_host, clr, eps);
    });
}

}  // namespace

#define DLRM_ADAGRAD_ARGS                                                                                                      \
    T, B, D, weight_host, state_host, rows_host, indices_host, offsets_host, nnz_host, psw_host, idx_bits, dout, dout_ld, lr, \
        lr_dev, eps, workspace, workspace_bytes, err, stream

extern "C" int dlrm_emb_bwd_rowwise_adagrad(int T, int64_t B, int D, void* const* weight_host,
                                            void* const* state_host, const int64_t* rows_host,
                                            const void* const* indices_host, const void* const* offsets_host,
                                            const int64_t* nnz_host, const void* const* psw_host, int idx_bits,
                                            const float* dout, int64_t dout_ld, float lr, const float* lr_dev, float eps,
                                            void* workspace, int64_t workspace_bytes, int64_t* err, void* stream) {
    return emb_bwd_adagrad_any<false>("dlrm_emb_bwd_rowwise_adagrad", DLRM_ADAGRAD_ARGS);
}

// state_host[t]: torch's state["sum"] of table t, contiguous fp32 [rows_host[t], D]
extern "C" int dlrm_emb_bwd_adagrad(int T, int64_t B, int D, void* const* weight_host,
                                    void* const* state_host, const int64_t* rows_host,
                                    const void* const* indices_host, const void* const* offsets_host,
                                    const int64_t* nnz_host, const void* const* psw_host, int idx_bits,
                                    const float* dout, int64_t dout_ld, float lr, const float* lr_dev, float eps,
                                    void* workspace, int64_t workspace_bytes, int64_t* err, void* stream) {
    return emb_bwd_adagrad_any<true>("dlrm_emb_bwd_adagrad", DLRM_ADAGRAD_ARGS);
}
#undef DLRM_ADAGRAD_ARGS

extern "C" int dlrm_adagrad_dense(int64_t n, float* w, float* sum, const float* g, float lr, const float* lr_dev, float eps, void* stream) {
    if (n <= 0 || !w || !sum || !g) return DLRM_E_ARG;
    long long nblk = (n + 255) / 256; if (nblk > 4096) nblk = 4096;
    hipLaunchKernelGGL(adagrad_dense_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (long long)n, w, sum, g, dlrm_step_pos(lr, lr_dev), eps);
    DLRM_LAUNCH_CHECK();
    return 0;
}
