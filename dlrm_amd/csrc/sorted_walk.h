// sorted_walk.h — the walk over (table, row)-sorted lookups that every Adagrad-style embedding update shares, once: pass 1 (groups), pass 2
// (fix-up), the edge buffers between them and the host side around them.  adagrad.hip (fp32 rows: row-wise and exact Adagrad) and
// emb_bf16.hip (bf16 rows: SGD and row-wise Adagrad with one rounding per row) wrap the two bodies in their kernels.
//
// The update is non-linear in a row's gradient g_r, so g_r must be complete before it is applied.  Lookups of all tables are sorted by
// (table, row) (sorted_common.h); a group of LPB lanes then owns kG = 64 consecutive sorted entries:
//   pass 1  walks its entries, sums each run of equal keys in input order (stable sort) and applies the update for every run that lies inside
//           the group; the partial sums of a run that continues from the previous group or into the next one go to an edge buffer (plain
//           stores, no atomics);
//   pass 2  one lane group per run that crosses a group boundary (owner = the group where the run starts) finds the run's end by binary
//           search in the sorted keys, adds the edge partials in order and applies the update.
// Every sum has a fixed order, and g_r is summed in fp32 with the lane geometry of emb_lookup.h's pick() whatever the table's row format:
// g_r has the same bits in every update built on the walk.
//
// What differs is a ROW-UPDATE POLICY, an object the wrapping kernel builds from its own arguments (step size, eps, rounding ...):
//   template <int VEC, int LPB, int NCH> apply(w, state, t, row, D, lig, acc)
//       w / state: table t's row storage and optimizer state as the launch group's argument blocks hold them; acc: the lane's columns of
//       g_r.  Called by all LPB lanes of a group together (same control flow).
// A new row format or optimizer supplies a policy, two thin __global__ wrappers and a launch lambda for walk_update().
// The groups wrapper stages the per-table arguments itself (WALK_STAGE_TABLES): read inside the inlined body, hipcc merged the kernarg loads
// of the 32 tables into s_load_dwordx16 groups held across the whole prologue, 16 more SGPRs per kernel than the same lines in the kernel.
#pragma once
#include "sorted_common.h"

namespace {

constexpr int kG = 64;          // sorted entries per lane group

// acc = v_add(acc, v_scale(psw, g)) is meant as two roundings (the reference scales the COO value, then coalesces).  __fmul_rn / __fadd_rn
// do not enforce that under hipcc (plain * and +: see group_sum_sq).  The compiled kernels do keep them apart (v_pk_mul_f32 / v_pk_add_f32,
// no fused form: in walk_groups a select between the scaled and the unscaled row stands between the product and the sum), and both updates
// share these lines, so they cannot drift apart; the weighted cases of the oracle tests are the check on the two roundings themselves.

__device__ __forceinline__ float4 v_add(const float4& a, const float4& b) {
    return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float v_add(const float& a, const float& b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float4 v_scale(float s, const float4& v) {
    return make_float4(__fmul_rn(s, v.x), __fmul_rn(s, v.y), __fmul_rn(s, v.z), __fmul_rn(s, v.w));
}
__device__ __forceinline__ float v_scale(float s, const float& v) { return __fmul_rn(s, v); }

// The sum of squares of a row's gradient over the lane group — the ONE definition behind every row-wise Adagrad accumulator, so that a bf16
// model's accumulators have the fp32 kernel's bits by construction.  Four columns per lane: every product and every sum is rounded on its
// own, (x^2 + y^2) + (z^2 + w^2) (hipcc's __fmul_rn / __fadd_rn are plain * and +, which -ffp-contract=fast may fuse: the pragma is what
// keeps them apart); one column per lane: fmaf(v, v, sq) chained over the chunks.  Then the xor tree over the group's lanes.
template <int VEC, int LPB, int NCH>
__device__ __forceinline__ float group_sum_sq(const typename Vec<VEC>::T (&acc)[NCH], int D, int lig) {
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int col = (c * LPB + lig) * VEC;
        if constexpr (VEC == 4) {
#pragma clang fp contract(off)
            if (col < D)
                sq = __fadd_rn(sq, __fadd_rn(__fadd_rn(__fmul_rn(acc[c].x, acc[c].x), __fmul_rn(acc[c].y, acc[c].y)),
                                             __fadd_rn(__fmul_rn(acc[c].z, acc[c].z), __fmul_rn(acc[c].w, acc[c].w))));
        } else {
            if (col < D) sq = __builtin_fmaf(acc[c], acc[c], sq);
        }
    }
#pragma unroll
    for (int o = LPB >> 1; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    return sq;
}

template <typename T> __device__ __forceinline__ T group_bcast(T v, int src_lane);
template <> __device__ __forceinline__ unsigned group_bcast<unsigned>(unsigned v, int src_lane) { return (unsigned)__shfl((int)v, src_lane, 64); }
template <> __device__ __forceinline__ unsigned long long group_bcast<unsigned long long>(unsigned long long v, int src_lane) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src_lane, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src_lane, 64);
    return ((unsigned long long)hi << 32) | lo;
}
template <> __device__ __forceinline__ float group_bcast<float>(float v, int src_lane) { return __shfl(v, src_lane, 64); }

// Pass 1.  A lookup's gradient row is found through a chain of dependent loads — sorted key, sorted value (= lookup position), bag of
// that position, row of dOut — and rounds 1-3 walked that chain once per ENTRY: 64 entries x 4 memory latencies per lane group, with one
// 512-byte row in flight per group (1.85 TB/s for the 14 M lookups of the MLPerf-v2 batch: latency-bound, not HBM-bound; more rows per step
// only lengthened the chains: DLRM_ADAGRAD_KC 1 / 2 / 4 = 5.28 / 5.55 / 5.8 ms).  Now the GROUP resolves all of its 64 entries at once: lane l
// loads the keys and values of entries l, l + LPB, ... (coalesced), gathers their bags (and pooling weights) — two latencies for the whole
// group — and the walk then takes (key, bag, weight) of entry j from lane j % LPB by a cross-lane read: the row loads depend on registers
// only and kC of them are in flight per group.  Same entries, same order, same sums: results are bit-identical to the old walk.
// Measured (round 4): emb_bwd_adagrad of the MLPerf-v2 batch 4.85 -> 3.62 ms, of the Terabyte batch 0.685 -> 0.56 ms.  (Also requesting the table
// row and accumulator of a run when it STARTS, so that its end waits for nothing, changed nothing — 3.69-3.76 ms: the walk is at ~0.7 of the copy
// rate on its real traffic by then, the rest of the category is the sort.)
// kC = gradient rows in flight per lane group: 2 everywhere (measured 3.62 / 3.68 / 3.98 ms for 2 / 4 / 8 on the MLPerf-v2 batch: with the
// group-level resolve the rows depend on registers only, so more in flight is more bandwidth — before it, 1 was best); the fp32 row-wise
// update alone has it as a tuning knob.
// per-table arguments are indexed by a lane-dependent table id: staged in LDS (a by-value kernel argument array indexed that way is
// copied to scratch memory by the compiler).  In the groups KERNEL, before the body: declares and fills `wt`
struct WalkTables { const long long* w; const long long* state; const long long* psw; const long long* base; const int* slot; };
#define WALK_STAGE_TABLES(sa, aa)                                                                                                        \
    __shared__ long long s_w[DLRM_MAX_TABLES_PER_LAUNCH], s_state[DLRM_MAX_TABLES_PER_LAUNCH], s_psw[DLRM_MAX_TABLES_PER_LAUNCH],        \
        s_base[DLRM_MAX_TABLES_PER_LAUNCH];                                                                                              \
    __shared__ int s_slot[DLRM_MAX_TABLES_PER_LAUNCH];                                                                                   \
    _Pragma("unroll") for (int k = 0; k < DLRM_MAX_TABLES_PER_LAUNCH; ++k)                                                               \
        if (threadIdx.x == k) {                                                                                                          \
            s_w[k] = (long long)(sa).w[k]; s_state[k] = (long long)(aa).state[k]; s_psw[k] = (long long)(sa).psw[k];                     \
            s_base[k] = (sa).base[k]; s_slot[k] = (sa).slot[k];                                                                          \
        }                                                                                                                                \
    __syncthreads();                                                                                                                     \
    const WalkTables wt = {s_w, s_state, s_psw, s_base, s_slot}

template <int VEC, int LPB, int NCH, typename KT, int kC, typename Upd>
__device__ __forceinline__ void walk_groups(const WalkTables& wt, long long L, int D,
                                            int row_bits, const KT* __restrict__ keys, const unsigned* __restrict__ vals,
                                            const unsigned* __restrict__ bag_of, const float* __restrict__ dout, long long dout_ld,
                                            const Upd& upd, float* __restrict__ edge_first, float* __restrict__ edge_last) {
    using VT = typename Vec<VEC>::T;
    constexpr int DP = NCH * LPB * VEC;                  // padded row length of the edge buffers
    constexpr int GPB = 256 / LPB;
    constexpr int NS = kG / LPB;                         // entries a lane resolves for its group (LPB is a power of two <= 64)
    static_assert(kG % LPB == 0 && LPB % kC == 0, "group geometry");
    const long long* s_w = wt.w; const long long* s_state = wt.state; const long long* s_psw = wt.psw; const long long* s_base = wt.base;
    const int* s_slot = wt.slot;
    const int g = threadIdx.x / LPB, lig = threadIdx.x % LPB;
    const int lane0 = (threadIdx.x & 63) & ~(LPB - 1);   // first lane of this group inside its wave
    const long long grp = (long long)blockIdx.x * GPB + g;
    const long long g0 = grp * kG;
    if (g0 >= L) return;
    const long long g_end = (g0 + kG < L) ? g0 + kG : L;
    const KT row_mask = (((KT)1) << row_bits) - 1;
    const bool cont_in = g0 > 0 && keys[g0 - 1] == keys[g0];
    const bool tail_cont = g0 + kG < L && keys[g0 + kG - 1] == keys[g0 + kG];

    // ---- resolve: entry g0 + s * LPB + lig for s = 0 .. NS-1
    KT e_key[NS];
    unsigned e_bag[NS];
    float e_sc[NS];                                      // pooling weight of the lookup; < 0 is never used as a marker: e_w says whether it applies
    bool e_w[NS];
    {
        unsigned pos[NS];
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) {
            const long long e = g0 + s_ * LPB + lig;
            const bool live = e < g_end;
            e_key[s_] = live ? keys[e] : (KT)0;
            pos[s_] = live ? vals[e] : 0u;
        }
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) {
            const bool live = g0 + s_ * LPB + lig < g_end;
            const int t = (int)(e_key[s_] >> row_bits);
            e_bag[s_] = live ? bag_of[pos[s_]] : DLRM_DEAD_BAG;
            const float* psw = (const float*)s_psw[t];
            e_w[s_] = live && psw != nullptr;
            e_sc[s_] = e_w[s_] ? psw[(long long)pos[s_] - s_base[t]] : 1.f;
        }
    }

    VT acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) v_zero(acc[c]);
    KT run_key = group_bcast<KT>(e_key[0], lane0);       // key of entry g0
    bool run_first = true, run_empty = true;

    auto finish = [&](bool is_last) {
        if (run_first && cont_in) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) *(VT*)(edge_first + grp * DP + (c * LPB + lig) * VEC) = acc[c];
        } else if (is_last && tail_cont) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) *(VT*)(edge_last + grp * DP + (c * LPB + lig) * VEC) = acc[c];
        } else {
            const int t = (int)(run_key >> row_bits);
            const long long row = (long long)(run_key & row_mask);
            upd.template apply<VEC, LPB, NCH>((float*)s_w[t], (float*)s_state[t], t, row, D, lig, acc);
        }
    };

#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) {
        const long long s0 = g0 + s_ * LPB;
        if (s0 >= g_end) break;
        for (int j0 = 0; j0 < LPB; j0 += kC) {
            if (s0 + j0 >= g_end) break;
            KT k[kC];
            VT gr[kC][NCH];
            float sc[kC];
            bool live[kC], weighted[kC];
#pragma unroll
            for (int j = 0; j < kC; ++j) {
                const int src = lane0 + j0 + j;
                live[j] = s0 + j0 + j < g_end;
                k[j] = group_bcast<KT>(e_key[s_], src);
                unsigned bag = group_bcast<unsigned>(e_bag[s_], src);
                sc[j] = group_bcast<float>(e_sc[s_], src);
                const bool w_ = __shfl((int)e_w[s_], src, 64) != 0;
                const int t = (int)(k[j] >> row_bits);
                const bool dead = bag == DLRM_DEAD_BAG;            // out-of-range lookup (expand_kernel): zero gradient
                if (dead) bag = 0u;
                weighted[j] = live[j] && w_ && !dead;
                const float* grow = dout + (long long)bag * dout_ld + (long long)s_slot[t] * D;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int col = (c * LPB + lig) * VEC;
                    v_zero(gr[j][c]);
                    if (live[j] && !dead && col < D) gr[j][c] = *(const VT*)(grow + col);
                }
            }
#pragma unroll
            for (int j = 0; j < kC; ++j) {
                if (!live[j]) break;
                if (k[j] != run_key) {
                    finish(false);
                    run_key = k[j]; run_first = false; run_empty = true;
                }
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const VT v = weighted[j] ? v_scale(sc[j], gr[j][c]) : gr[j][c];
                    acc[c] = run_empty ? v : v_add(acc[c], v);
                }
                run_empty = false;
            }
        }
    }
    finish(true);
}

// Pass 2.  One lane group per group index: acts only where a run starts in this group and continues into the next one
template <int VEC, int LPB, int NCH, typename KT, typename Upd>
__device__ __forceinline__ void walk_fixup(const SortedArgs& sa, float* const (&state)[DLRM_MAX_TABLES_PER_LAUNCH], long long L, int D,
                                           int row_bits, const KT* __restrict__ keys, const Upd& upd,
                                           const float* __restrict__ edge_first, const float* __restrict__ edge_last) {
    using VT = typename Vec<VEC>::T;
    constexpr int DP = NCH * LPB * VEC;
    constexpr int GPB = 256 / LPB;
    const int g = threadIdx.x / LPB, lig = threadIdx.x % LPB;
    const long long grp = (long long)blockIdx.x * GPB + g;
    const long long g0 = grp * kG;
    if (g0 + kG >= L) return;                                   // no next group: nothing continues
    const KT key = keys[g0 + kG - 1];
    if (key != keys[g0 + kG]) return;                           // last run ends inside this group
    if (g0 > 0 && keys[g0 - 1] == key) return;                  // the run began before this group: not the owner
    // run end = first position with keys[pos] != key  (keys are sorted: binary search in (g0 + kG, L])
    long long lo = g0 + kG + 1, hi = L;                         // keys[lo - 1] == key
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] == key) lo = mid + 1; else hi = mid;
    }
    const long long last_grp = (lo - 1) / kG;                   // group holding the run's last entry (> grp)
    VT acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] = *(const VT*)(edge_last + grp * DP + (c * LPB + lig) * VEC);
    long long j = grp + 1;
    for (; j + 7 <= last_grp; j += 8) {                         // 8 independent partial rows in flight
        VT p[8][NCH];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int c = 0; c < NCH; ++c) p[u][c] = *(const VT*)(edge_first + (j + u) * DP + (c * LPB + lig) * VEC);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int c = 0; c < NCH; ++c) acc[c] = v_add(acc[c], p[u][c]);
    }
    for (; j <= last_grp; ++j)
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = v_add(acc[c], *(const VT*)(edge_first + j * DP + (c * LPB + lig) * VEC));
    const KT row_mask = (((KT)1) << row_bits) - 1;
    const int t = (int)(key >> row_bits);
    const long long row = (long long)(key & row_mask);
    upd.template apply<VEC, LPB, NCH>(sa.w[t], state[t], t, row, D, lig, acc);
}

// ---- host side ---------------------------------------------------------------------------------
// edge buffers use the widest padded row any shape of this D can have (vector path: D rounded up; scalar path likewise)
static size_t edge_row_floats(int D) {
    Shape a, b;
    size_t m = 0;
    if (pick(D, true, &a) == 0) m = (size_t)a.dp;
    if (pick(D, false, &b) == 0 && (size_t)b.dp > m) m = (size_t)b.dp;
    return m;
}

struct WalkLayout { Layout sort; size_t edge_first, edge_last, total; };

static int walk_layout(size_t L, bool wide, int key_bits, int D, WalkLayout* lo, int n, const int64_t* nnz, const int64_t* rows) {
    int rc = make_layout(L, wide, key_bits, &lo->sort, n, nnz, rows);
    if (rc) return rc;
    const size_t groups = (L + kG - 1) / kG;
    const size_t row = edge_row_floats(D);
    if (row == 0) return DLRM_E_RANGE;
    size_t o = lo->sort.total;
    lo->edge_first = o; o += align256(groups * row * sizeof(float));
    lo->edge_last = o;  o += align256(groups * row * sizeof(float));
    lo->total = o;
    return 0;
}

// One launch group of at most 32 tables: its size and key width, and where its sorted lookups and edge buffers lie in the workspace
struct WalkGroup {
    int t0, n;
    size_t L;
    int row_bits, key_bits;
    WalkLayout lo;
};
// false: the group has no lookups
static bool walk_group(int T, int t0, const int64_t* nnz_host, const int64_t* rows_host, WalkGroup* g) {
    g->t0 = t0; g->n = (T - t0 < DLRM_MAX_TABLES_PER_LAUNCH) ? T - t0 : DLRM_MAX_TABLES_PER_LAUNCH;
    g->L = 0; long long max_rows = 1;
    for (int k = 0; k < g->n; ++k) { g->L += (size_t)nnz_host[t0 + k]; if (rows_host[t0 + k] > max_rows) max_rows = rows_host[t0 + k]; }
    g->row_bits = bits_for(max_rows); g->key_bits = g->row_bits + bits_for(g->n);
    return g->L != 0;
}

// the workspace every update built on the walk needs: the largest launch group's
static int64_t walk_workspace_bytes(int T, int D, const int64_t* nnz_host, const int64_t* rows_host) {
    if (T <= 0 || D <= 0 || !nnz_host || !rows_host) return 0;
    size_t worst = 0;
    for (int t0 = 0; t0 < T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        WalkGroup g;
        if (!walk_group(T, t0, nnz_host, rows_host, &g)) continue;
        if (walk_layout(g.L, g.key_bits > 32, g.key_bits, D, &g.lo, g.n, nnz_host + t0, rows_host + t0) != 0) return -1;
        if (g.lo.total > worst) worst = g.lo.total;
    }
    return (int64_t)worst;
}

// the caller's arguments the walk's host side passes on
struct WalkCall {
    int T; int64_t B; int D;
    void* const* weight_host; const int64_t* rows_host; const void* const* indices_host; const void* const* offsets_host;
    const int64_t* nnz_host; const void* const* psw_host; int idx_bits; const float* dout; int64_t dout_ld;
    void* workspace; int64_t workspace_bytes; int64_t* err; hipStream_t st;
};
// what a launch lambda gets: the group, its sorted lookups and edge buffers, and the grid of both passes
template <typename KT>
struct WalkLaunch {
    using Key = KT;
    const WalkGroup* g; SortedArgs sa;
    const KT* keys; const unsigned* vals; const unsigned* bag_of; float* edge_first; float* edge_last;
    dim3 grid, block;
};

template <typename KT, typename Launch>
static int walk_run(const WalkCall& c, const WalkGroup& g, bool vec_ok, Launch& launch) {
    int ids[DLRM_MAX_TABLES_PER_LAUNCH];
    for (int k = 0; k < g.n; ++k) ids[k] = g.t0 + k;
    char* ws = (char*)c.workspace;
    WalkLaunch<KT> w;
    int rc = expand_and_sort<KT>(g.n, ids, c.B, c.weight_host, c.rows_host, c.indices_host, c.offsets_host, c.nnz_host, c.psw_host, c.idx_bits, ws,
                                 g.lo.sort, g.L, g.row_bits, g.key_bits, c.st, &w.sa, c.err);
    if (rc) return rc;
    w.g = &g;
    w.keys = (const KT*)(ws + g.lo.sort.keys_out);
    w.vals = (const unsigned*)(ws + g.lo.sort.vals_out);
    w.bag_of = (const unsigned*)(ws + g.lo.sort.bag_of);
    w.edge_first = (float*)(ws + g.lo.edge_first);
    w.edge_last = (float*)(ws + g.lo.edge_last);
    Shape s;
    rc = pick(c.D, vec_ok, &s);
    if (rc) return rc;
    const size_t groups = (g.L + kG - 1) / kG;
    const int gpb = 256 / s.lpb;
    w.grid = dim3((unsigned)((groups + gpb - 1) / gpb), 1, 1); w.block = dim3(256);
    return dispatch_shape(s, [&](auto vec, auto lpb, auto nch) { return launch(w, vec, lpb, nch); });
}

// The host side of an update, after the entry point's own argument checks: per launch group the keys are sized, the workspace laid out and
// checked, the lookups expanded and sorted and the lane geometry picked; launch(WalkLaunch<KT>, VEC, LPB, NCH) then enqueues the policy's
// groups kernel and fix-up kernel and returns 0 or an error code.
template <typename Launch>
static int walk_update(const char* name, const WalkCall& c, bool vec_ok, Launch launch) {
    for (int t0 = 0; t0 < c.T; t0 += DLRM_MAX_TABLES_PER_LAUNCH) {
        WalkGroup g;
        if (!walk_group(c.T, t0, c.nnz_host, c.rows_host, &g)) continue;
        if (g.L >= ((size_t)1 << 32)) return DLRM_E_RANGE;
        const bool wide = g.key_bits > 32;
        int rc = walk_layout(g.L, wide, g.key_bits, c.D, &g.lo, g.n, c.nnz_host + t0, c.rows_host + t0);
        if (rc) return rc;
        if (!c.workspace || !dlrm_aligned16(c.workspace) || (size_t)c.workspace_bytes < g.lo.total) {
            fprintf(stderr, "libdlrm_hip: %s: workspace too small (%lld < %zu bytes)\n", name, (long long)c.workspace_bytes, g.lo.total);
            return DLRM_E_ARG;
        }
        rc = wide ? walk_run<unsigned long long>(c, g, vec_ok, launch) : walk_run<unsigned>(c, g, vec_ok, launch);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace
